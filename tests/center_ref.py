"""Centred framing restated -- TEST INFRASTRUCTURE ONLY (a plain module, not a conftest; no HIP at import).

The rule of include/mfcc_hip.h ("centring"), written with ``np.pad`` instead of the index rule, the closed forms of its
geometry, and a float64 ``torch.stft(center=True)`` power reference computed on the CPU.

``torch.stft`` centres a window shorter than ``n_fft`` inside the transform (``(n_fft - win_length) // 2`` zeros in front);
the library puts the frame at the start of the transform and zeros behind it.  The two differ by a circular shift of the
transform's input, which changes the phase of every bin and not its power; what has to agree is WHICH samples a frame
holds, and that is ``PL = n_fft // 2 - (n_fft - L) // 2``.
"""
from __future__ import annotations

import numpy as np

MODES = ("reflect", "zeros")

# (nfft, hop, frame length) of the host tests
FRAMINGS = [(512, 160, 400), (512, 160, 401), (512, 170, 512), (256, 80, 199), (64, 21, 64)]


def left_pad(nfft, L):
    return nfft // 2 - (nfft - L) // 2


def frames(n, nfft, hop, L, mode="reflect"):
    if (mode == "reflect" and n <= left_pad(nfft, L)) or n == 0:
        return 0
    return 1 + n // hop


def padded_len(n, nfft, hop, L, mode="reflect"):
    f = frames(n, nfft, hop, L, mode)
    return (f - 1) * hop + L if f else 0


def lengths(nfft, hop, L):
    """The sample counts of the host tests: both sides of every threshold of the rule."""
    pl = left_pad(nfft, L)
    out = [pl + 1, L - 1, L, L + 1]
    for k in (1, 5, 17):
        out += [k * hop - 1, k * hop, k * hop + 1]
    return sorted({n for n in out if n > pl})


def corpus_lengths(nfft, hop, L):
    """The length list of the plan and ragged tests: no frame (0, 1, PL), one frame, and the hop's residues."""
    pl = left_pad(nfft, L)
    return [0, 1, pl, pl + 1, L, 5 * hop - 1, 5 * hop, 33 * hop + 7]


def pad(x, nfft, hop, L, mode="reflect"):
    """The padded signal of int16 ``x`` by ``np.pad``; empty where the signal gives no frame."""
    x = np.asarray(x)
    n = len(x)
    np_ = padded_len(n, nfft, hop, L, mode)
    if not np_:
        return np.zeros(0, x.dtype)
    pl = left_pad(nfft, L)
    right = np_ - pl - n
    if right >= 0:
        return np.pad(x, (pl, right), mode="reflect" if mode == "reflect" else "constant")
    # the last frame ends inside the signal (a frame longer than two hops): pad the left, cut the right
    return np.pad(x, (pl, 0), mode="reflect" if mode == "reflect" else "constant")[:np_]


def torch_accepts(n, nfft):
    """``torch.stft(center=True, pad_mode="reflect")`` refuses a signal it cannot reflect by ``n_fft // 2``."""
    return n > nfft // 2


def stft_power(x, nfft, hop, L, window):
    """float64 ``(frames, nfft // 2 + 1)``: ``|torch.stft(x, center=True, pad_mode="reflect")|**2`` with ``window``
    (``L`` values) in float64, on the CPU."""
    import torch
    X = torch.stft(torch.from_numpy(np.asarray(x, dtype=np.float64)), n_fft=nfft, hop_length=hop, win_length=L,
                   window=torch.from_numpy(np.asarray(window, dtype=np.float64)), center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    return (X.real ** 2 + X.imag ** 2).numpy().T.copy()


def chain_power(p, nfft, hop, L, window):
    """float64 ``(frames, nfft // 2 + 1)``: the library's uncentred chain without pre-emphasis on the padded signal
    ``p`` -- frame ``t`` = ``p[t hop : t hop + L] * window``, zeros up to ``nfft``, ``|rfft|**2``."""
    p = np.asarray(p, dtype=np.float64)
    if len(p) < L:
        return np.zeros((0, nfft // 2 + 1))
    nf = (len(p) - L) // hop + 1
    idx = np.arange(L)[None, :] + hop * np.arange(nf)[:, None]
    fr = np.zeros((nf, nfft))
    fr[:, :L] = p[idx] * np.asarray(window, dtype=np.float64)[None, :]
    X = np.fft.rfft(fr, axis=1)
    return X.real ** 2 + X.imag ** 2
