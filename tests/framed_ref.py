"""float64 reference of the float path with a frame length below nfft -- TEST INFRASTRUCTURE ONLY (a plain module).

Contract (include/mfcc_hip.h: mfcc_hip_create_framed).  For frame length ``L``, ``hop <= L <= nfft`` and ``L >= 2``:

* frame ``f`` is samples ``[f * hop, f * hop + L)`` of the pre-emphasised stream;
* it is multiplied by the periodic Hamming window of length ``L``, ``w[i] = 0.54 - 0.46 cos(2 pi i / L)``
  (``get_window("hamm", L, fftbins=True)``), and zero-padded at the end to ``nfft``;
* from the FFT on the chain is the notebook's: mel points, ``power_scale``, DCT depend on ``nfft`` as before;
* frame counts: notebook ``(n - L) // hop + 1`` (0 if ``n < L``), stream ``(n - L) // hop + 2`` (1 if ``n < L``).

Every stage is a function of ``oracle/mfcc_float.py``; with ``L = nfft`` the result is ``mfcc_notebook`` bit for bit.
The bound is ``oracle.error_bound.bound_from_stages`` on these stages, the comparison ``oracle.error_bound.check``.
"""
from __future__ import annotations

import numpy as np

import logmel_bound as lb
from oracle import error_bound as eb
from oracle import mfcc_float as mf


def num_frames(n, L, hop, pad_mode="notebook"):
    if pad_mode == "notebook":
        return 0 if n < L else (n - L) // hop + 1
    return 1 if n < L else (n - L) // hop + 2


def framed_notebook(x, L, hop, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0):
    """(frames, n_mel) float64 cepstra of the stream ``x`` in notebook framing and the stages dict ``power``,
    ``filters``, ``mel``, ``logmel``, ``dct_basis`` that ``eb.bound_from_stages`` reads."""
    if not (hop <= L <= nfft and L >= 2):
        raise ValueError("need hop <= L <= nfft and L >= 2: L %d, hop %d, nfft %d" % (L, hop, nfft))
    emphasis = mf.pre_emphasis(np.asarray(x))
    framed = mf.frame_audio(emphasis, nfft=L, hop=hop)                  # (frames, L)
    win = framed * mf.hamming_window(L)
    padded = np.zeros((len(win), nfft))
    padded[:, :L] = win
    fft = mf.fft_frames(padded, nfft)
    power = mf.power_spectrum(fft, power_scale) if len(fft) else np.zeros((0, nfft // 2 + 1))
    filters = mf.mel_filterbank(nfft, n_mel, sample_rate)
    mel = np.dot(filters, np.transpose(power))
    with np.errstate(divide="ignore"):
        logmel = np.log2(mel)
    basis = mf.dct_basis(n_mel, n_mel)
    cep = np.ascontiguousarray(np.dot(basis, logmel).T)
    return cep, dict(power=power, filters=filters, mel=mel.T, logmel=logmel.T, dct_basis=basis)


def _frames_source(x, L, hop, pad_mode, halo):
    """``eb._frames_source`` with the frame length in place of nfft."""
    x = np.asarray(x)
    if halo:            # sample 0 is history only: put it one hop into a longer stream, drop that stream's frame 0
        x = np.concatenate([np.zeros(hop - 1, dtype=x.dtype), x])
    if pad_mode == "stream":
        nf = num_frames(len(x), L, hop, "stream")
        x = np.concatenate([x, np.zeros((nf - 1) * hop + L - len(x), dtype=x.dtype)])
    elif pad_mode != "notebook":
        raise ValueError(pad_mode)
    return x, int(bool(halo))


def reference_and_bound(pcm, model, L, hop, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0, n_cep=13,
                        pad_mode="notebook", halo=0, output="cepstra", lifter=0.0):
    """float64 reference and per-value bound of int16 ``pcm`` (n,) or (channels, n) for the arithmetic ``model`` of
    ``eb.MODELS``.  ``output="logmel"``: the log-mel rows under the log-mel bound of tests/logmel_bound.py, built on
    these stages: the identity as the DCT basis, plus that module's absolute term for the log and its further charge for
    a bf16 x 2-split mel contraction, whose error a log-mel value sees undiluted (both are explained there).
    ``lifter``: the cepstra (not log-mel rows) and their bound times ``1 + (lifter / 2) sin(pi k / lifter)``."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        rb = [reference_and_bound(c, model, L, hop, nfft, n_mel, sample_rate, power_scale, n_cep, pad_mode, halo, output,
                                  lifter) for c in pcm]
        return np.stack([r for r, _ in rb]), np.stack([b for _, b in rb])
    x, drop = _frames_source(pcm, L, hop, pad_mode, halo)
    cep, st = framed_notebook(x, L, hop, nfft, n_mel, sample_rate, power_scale)
    st = dict(st, power=st["power"][drop:], mel=st["mel"][drop:], logmel=st["logmel"][drop:])
    if output == "logmel":
        ref, n_cep = st["logmel"], n_mel
    else:
        ref = mf.lifter(cep[drop:, :n_cep], lifter) if lifter else cep[drop:, :n_cep]
    if len(ref) == 0:
        return ref, np.zeros_like(ref)
    if output == "logmel":
        return ref, lb.bound_from_stages(st, model)      # per band: an empty filter pins its own column only
    return ref, eb.bound_from_stages(st, model, n_cep, lifter)


def check(got, ref, bound, what=""):
    return eb.check(got, ref, bound, what)
