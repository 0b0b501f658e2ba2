"""float64 reference of the float path with a FRONT -- a window function and a pre-emphasis pair -- TEST INFRASTRUCTURE
ONLY (a plain module, not a conftest).

Contract (include/mfcc_hip.h: mfcc_hip_create_fronted).  A front is ``(window kind, periodic flag, (num, den))``:

* the window over the frame length ``L`` with ``D = L`` (periodic) or ``D = L - 1`` (symmetric), in float64::

      hamming      0.54 - 0.46 cos(2 pi i / D)
      hann         0.5 - 0.5 cos(2 pi i / D)
      povey        (0.5 - 0.5 cos(2 pi i / D)) ** 0.85
      blackman     0.42 - 0.5 cos(2 pi i / D) + 0.08 cos(4 pi i / D)
      rectangular  1

* pre-emphasis ``y[i] = x[i] - (num / den) x[i-1]``, ``x[-1]`` the history sample (0 at a stream's start);
* everything behind the window is the chain of tests/framed_ref.py: zero-padding to ``nfft``, FFT, power, bank, log2, DCT.

This module is the float64 staging of ``framed_ref.framed_notebook`` with the window vector and the pair as arguments.
With the default front (Hamming, periodic, 31/32) it takes the very calls of ``oracle/mfcc_float.py`` that framed_ref
takes, so its stages are framed_ref's and its power is ``spectrum_ref.reference`` bit for bit (tests/test_front_host.py
asserts both).  The cepstral and log-mel bounds are ``oracle.error_bound.bound_from_stages`` /
``logmel_bound.bound_from_stages`` on these stages; power rows are held under ``spectrum_ref.bound`` and band energies
under tests/fbank_ref.py, unchanged.
"""
from __future__ import annotations

import numpy as np
import scipy.fft

import logmel_bound as lb
import spectrum_ref as sr
from oracle import error_bound as eb
from oracle import mfcc_float as mf

# (window, periodic, (num, den)): the fronts under test.  (rectangular, 63/64) has num + den = 127, the fused kernels'
# limit; (97, 100) is beyond it and runs the generic kernels
DEFAULT = ("hamming", True, (31, 32))
FRONTS = [
    DEFAULT,
    ("hann", True, (0, 1)),
    ("povey", False, (32, 33)),
    ("hamming", False, (97, 100)),
    ("blackman", False, (0, 1)),
    ("rectangular", True, (63, 64)),
]
KINDS = ["hamming", "hann", "povey", "blackman", "rectangular"]
FUSED_SUM = 127


def front_id(front):
    return "%s_%s_%d_%d" % (front[0], "per" if front[1] else "sym", front[2][0], front[2][1])


def front_kw(front):
    """The keyword arguments of ``mfcc_amd.MFCC`` / ``get_table`` for a front."""
    return dict(window=front[0], window_periodic=front[1], preemph=front[2])


def is_default(front):
    return front[0] == "hamming" and bool(front[1]) and tuple(front[2]) == (31, 32)


def fused_pair(front):
    return front[2][0] + front[2][1] <= FUSED_SUM


def window(kind, L, periodic=True):
    """float64 ``(L,)``, from the contract's formulas.  The default (Hamming, periodic) is the notebook's own call,
    ``get_window("hamm", L, fftbins=True)``: the function the library has had all along."""
    if kind == "hamming" and periodic:
        return mf.hamming_window(L)
    D = float(L if periodic else L - 1)
    i = np.arange(L, dtype=np.float64)
    c1 = np.cos(2.0 * np.pi * i / D)
    if kind == "hamming":
        return 0.54 - 0.46 * c1
    if kind == "hann":
        return 0.5 - 0.5 * c1
    if kind == "povey":
        return np.maximum(0.5 - 0.5 * c1, 0.0) ** 0.85
    if kind == "blackman":
        return 0.42 - 0.5 * c1 + 0.08 * np.cos(4.0 * np.pi * i / D)
    if kind == "rectangular":
        return np.ones(L)
    raise ValueError(kind)


def pre_emphasis(x, num, den):
    """float64 ``y[i] = x[i] - (num / den) x[i-1]``, ``y[0] = x[0]``.  31/32 is the notebook's expression itself; any
    other pair is ``(den x[i] - num x[i-1]) / den``: an exact integer and one division."""
    x = np.asarray(x)
    if (num, den) == (31, 32):
        return mf.pre_emphasis(x)
    xi = x.astype(np.int64)
    e = den * xi - num * np.concatenate([[0], xi[:-1]])
    return e.astype(np.float64) / float(den)


def fronted_notebook(x, front, L, hop, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0, filters=None):
    """``framed_ref.framed_notebook`` with the front's window and pair: (frames, n_mel) float64 cepstra of the stream
    ``x`` in notebook framing and the stages dict ``power``, ``filters``, ``mel``, ``logmel``, ``dct_basis`` that
    ``eb.bound_from_stages`` reads.  ``filters``: a matrix in place of the notebook bank (an HTK bank, melbank_ref)."""
    if not (hop <= L <= nfft and L >= 2):
        raise ValueError("need hop <= L <= nfft and L >= 2: L %d, hop %d, nfft %d" % (L, hop, nfft))
    kind, periodic, (num, den) = front
    emphasis = pre_emphasis(np.asarray(x), num, den)
    framed = mf.frame_audio(emphasis, nfft=L, hop=hop)                  # (frames, L)
    win = framed * window(kind, L, periodic)
    padded = np.zeros((len(win), nfft))
    padded[:, :L] = win
    fft = mf.fft_frames(padded, nfft)
    power = mf.power_spectrum(fft, power_scale) if len(fft) else np.zeros((0, nfft // 2 + 1))
    if filters is None:
        filters = mf.mel_filterbank(nfft, n_mel, sample_rate)
    n_mel = len(filters)
    mel = np.dot(filters, np.transpose(power))
    with np.errstate(divide="ignore"):
        logmel = np.log2(mel)
    basis = mf.dct_basis(n_mel, n_mel)
    with np.errstate(invalid="ignore"):
        cep = np.ascontiguousarray(np.dot(basis, logmel).T)
    return cep, dict(power=power, filters=filters, mel=mel.T, logmel=logmel.T, dct_basis=basis)


def reference_and_bound(pcm, model, front, L, hop, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0, n_cep=13,
                        pad_mode="notebook", halo=0, output="cepstra", filters=None):
    """float64 reference and per-value bound of int16 ``pcm`` (n,) or (channels, n) for the arithmetic ``model`` of
    ``eb.MODELS``: ``framed_ref.reference_and_bound`` on the fronted stages."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        rb = [reference_and_bound(c, model, front, L, hop, nfft, n_mel, sample_rate, power_scale, n_cep, pad_mode, halo,
                                  output, filters) for c in pcm]
        return np.stack([r for r, _ in rb]), np.stack([b for _, b in rb])
    x, drop = sr._source(pcm, L, hop, pad_mode, halo)
    cep, st = fronted_notebook(x, front, L, hop, nfft, n_mel, sample_rate, power_scale, filters)
    st = dict(st, power=st["power"][drop:], mel=st["mel"][drop:], logmel=st["logmel"][drop:])
    if output == "logmel":
        ref, n_cep = st["logmel"], len(st["filters"])
    else:
        ref = cep[drop:, :n_cep]
    if len(ref) == 0:
        return ref, np.zeros_like(ref)
    if output == "logmel":
        return ref, lb.bound_from_stages(st, model)
    return ref, eb.bound_from_stages(st, model, n_cep)


def power_reference(pcm, front, nfft=512, hop=170, L=None, power_scale=None, pad_mode="notebook", halo=0):
    """float64 ``(channels?, frames, nfft // 2 + 1)`` power of int16 ``pcm``: ``spectrum_ref.reference`` with the front."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        return np.stack([power_reference(c, front, nfft, hop, L, power_scale, pad_mode, halo) for c in pcm])
    L = nfft if L is None else L
    scale = sr.power_scale_of(nfft) if power_scale is None else float(power_scale)
    x, drop = sr._source(pcm, L, hop, pad_mode, halo)
    if len(x) < L:
        return np.zeros((0, nfft // 2 + 1))
    kind, periodic, (num, den) = front
    framed = mf.frame_audio(pre_emphasis(x, num, den), nfft=L, hop=hop)
    win = framed * window(kind, L, periodic)
    padded = np.zeros((len(win), nfft))
    padded[:, :L] = win
    return np.asarray(mf.power_spectrum(mf.fft_frames(padded, nfft), scale), dtype=np.float64)[drop:]


def emphasised_frames(pcm, front, nfft, hop, L, pad_mode, halo):
    """int64 ``(frames, L)``: ``den x[i] - num x[i - 1]`` of every frame's own samples, exact."""
    num, den = front[2]
    x, drop = sr._source(np.asarray(pcm), L, hop, pad_mode, halo)
    if len(x) < L:
        return np.zeros((0, L), np.int64)
    x = x.astype(np.int64)
    e = den * x - num * np.concatenate([[0], x[:-1]])
    nf = (len(x) - L) // hop + 1
    idx = np.arange(L)[None, :] + hop * np.arange(nf)[:, None]
    return e[idx][drop:]


def table_f32(front, L):
    """The kernels' window table: ``w / den`` in float64, rounded once to fp32."""
    return (window(front[0], L, front[1]) / float(front[2][1])).astype(np.float32)


def zero_frames(pcm, front, nfft, hop, L, pad_mode, halo):
    """Boolean ``(channels?, frames)``: frames whose windowed pre-emphasised samples are all zero (a window that is exactly
    0 at a frame's edge takes that sample out)."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        return np.stack([zero_frames(c, front, nfft, hop, L, pad_mode, halo) for c in pcm])
    L = nfft if L is None else L
    live = table_f32(front, L) != 0
    return ~((emphasised_frames(pcm, front, nfft, hop, L, pad_mode, halo) != 0) & live[None, :]).any(axis=1)


def restatement_f32(pcm, front, nfft=512, hop=170, L=None, power_scale=None, pad_mode="notebook", halo=0):
    """``spectrum_ref.restatement_f32`` with the front, as the kernels state it: the exact integer ``e`` as fp32 (``|e| <
    2^23``) times the fp32 table that carries ``1 / den``, ``scipy.fft.rfft`` on float32, the power in fp32."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        return np.stack([restatement_f32(c, front, nfft, hop, L, power_scale, pad_mode, halo) for c in pcm])
    L = nfft if L is None else L
    scale = sr.power_scale_of(nfft) if power_scale is None else float(power_scale)
    e = emphasised_frames(pcm, front, nfft, hop, L, pad_mode, halo)
    assert np.abs(e).max(initial=0) < 2 ** 23
    padded = np.zeros((len(e), nfft), np.float32)
    padded[:, :L] = e.astype(np.float32) * table_f32(front, L)[None, :]
    X = scipy.fft.rfft(padded, axis=1)
    if X.dtype != np.complex64:
        raise AssertionError("scipy.fft.rfft of float32 returned %s, not complex64" % X.dtype)
    inv = np.float32(1.0 / (scale * scale))
    p = (X.real * X.real + X.imag * X.imag) * inv
    assert p.dtype == np.float32
    return p


def measure(front, wav_pcm, configs=None):
    """``spectrum_ref.measure`` with the front: {config: (worst ratio of the fp32 restatement at C_SPEC = 1, kind)} over
    ``sr.input_list`` under ``sr.FRAMINGS``, at the two 512 shapes also the steady-state batch of an MI355X, at 512 / 170
    the whole golden wav."""
    table = {}

    def worst_of(x, nfft, hop, L, pad_mode, halo, names):
        ref = power_reference(x, front, nfft, hop, L, pad_mode=pad_mode, halo=halo)
        r = sr.ratios(restatement_f32(x, front, nfft, hop, L, pad_mode=pad_mode, halo=halo), ref, sr.bound(ref, 1.0))
        per_ch = r.reshape(len(x), -1).max(axis=1)
        k = int(np.argmax(per_ch))
        return float(per_ch[k]), names[k % len(names)]

    for nfft, hop, L in (sr.CONFIGS if configs is None else configs):
        x = sr.input_list(nfft, hop, L, wav_pcm)
        found = [worst_of(x, nfft, hop, L, pad_mode, halo, sr.KINDS) for pad_mode, halo in sr.FRAMINGS]
        if nfft == 512:
            _, frames, nch = sr.steady_shape(sr.MI355X_CUS)
            found.append(worst_of(sr.batch_inputs(nfft, hop, L, wav_pcm, nch, frames), nfft, hop, L, "notebook", 0, sr.KINDS))
        if (nfft, hop, L) == (512, 170, 512):
            found.append(worst_of(np.asarray(wav_pcm)[None, :], nfft, hop, L, "notebook", 0, ["golden wav"]))
        table[(nfft, hop, L)] = max(found)
    return table
