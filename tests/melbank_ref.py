"""float64 reference of the float path with an HTK-style mel bank -- TEST INFRASTRUCTURE ONLY (a plain module).

Contract (include/mfcc_hip.h: mfcc_hip_create_banked), restated here independently of the C++.  All of it float64:

* ``mel(f) = 1127 ln(1 + f / 700)``;
* edges ``e_j = mel(low) + j (mel(high) - mel(low)) / (n_mel + 1)`` for ``j = 0 .. n_mel + 1``;
* bin ``k`` lies at ``m_k = mel(k * sample_rate / nfft)`` for ``k = 0 .. nfft / 2``;
* ``W[j][k] = max(0, min((m_k - e_j) / (e_{j+1} - e_j), (e_{j+2} - m_k) / (e_{j+2} - e_{j+1})))``, no area
  normalisation, rounded once to fp32;
* ``0 <= low < high <= sample_rate / 2`` (``high`` 0 or None: ``sample_rate / 2``), ``1 <= n_mel <= 64``.

Everything outside the matrix is the chain of tests/framed_ref.py: pre-emphasis, frames of ``L`` samples under the
periodic Hamming window zero-padded to ``nfft``, ``power_scale``, log2, the orthonormal DCT-II.  The bound is
``oracle.error_bound.bound_from_stages`` on these stages, the comparison ``oracle.error_bound.check``; log-mel rows take
the terms of tests/logmel_bound.py, as framed_ref does.
"""
from __future__ import annotations

import math

import numpy as np

import framed_ref as fr
import logmel_bound as lb
from oracle import error_bound as eb
from oracle import mfcc_float as mf


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def htk_matrix(nfft, n_mel, sample_rate, low=0.0, high=None):
    """(n_mel, nfft / 2 + 1) float64 holding the fp32-rounded weights.  ``math.log`` is the C library's logarithm, one
    correctly ordered float64 operation after another: the table of the library is expected to match bit for bit."""
    high = float(sample_rate) / 2.0 if not high else float(high)
    if not (0.0 <= low < high <= float(sample_rate) / 2.0 and 1 <= n_mel <= 64):
        raise ValueError("bank (%r, %r, %r, %r)" % (n_mel, low, high, sample_rate))
    ml, mh = mel(float(low)), mel(high)
    e = [ml + j * (mh - ml) / (n_mel + 1) for j in range(n_mel + 2)]
    m = [mel(k * float(sample_rate) / nfft) for k in range(nfft // 2 + 1)]
    w = np.zeros((n_mel, nfft // 2 + 1))
    for j in range(n_mel):
        for k, mk in enumerate(m):
            w[j, k] = max(0.0, min((mk - e[j]) / (e[j + 1] - e[j]), (e[j + 2] - mk) / (e[j + 2] - e[j + 1])))
    return w.astype(np.float32).astype(np.float64)


def banked_notebook(x, filters, L, hop, nfft=512, power_scale=512.0):
    """``framed_ref.framed_notebook`` with ``filters`` in place of ``mf.mel_filterbank``: (frames, n_mel) float64
    cepstra and the stages dict that ``eb.bound_from_stages`` reads."""
    if not (hop <= L <= nfft and L >= 2):
        raise ValueError("need hop <= L <= nfft and L >= 2: L %d, hop %d, nfft %d" % (L, hop, nfft))
    n_mel = len(filters)
    emphasis = mf.pre_emphasis(np.asarray(x))
    framed = mf.frame_audio(emphasis, nfft=L, hop=hop)                  # (frames, L)
    win = framed * mf.hamming_window(L)
    padded = np.zeros((len(win), nfft))
    padded[:, :L] = win
    fft = mf.fft_frames(padded, nfft)
    power = mf.power_spectrum(fft, power_scale) if len(fft) else np.zeros((0, nfft // 2 + 1))
    mel_e = np.dot(filters, np.transpose(power))
    with np.errstate(divide="ignore"):
        logmel = np.log2(mel_e)
    basis = mf.dct_basis(n_mel, n_mel)
    with np.errstate(invalid="ignore"):
        cep = np.ascontiguousarray(np.dot(basis, logmel).T)
    return cep, dict(power=power, filters=filters, mel=mel_e.T, logmel=logmel.T, dct_basis=basis)


_MATRICES = {}


def matrix(nfft, n_mel, sample_rate, low, high):
    key = (nfft, n_mel, sample_rate, float(low), float(high or 0.0))
    if key not in _MATRICES:
        w = htk_matrix(nfft, n_mel, sample_rate, low, high)
        w.setflags(write=False)
        _MATRICES[key] = w
    return _MATRICES[key]


def reference_and_bound(pcm, model, L, hop, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0, n_cep=13,
                        pad_mode="notebook", halo=0, output="cepstra", low=0.0, high=None, lifter=0.0):
    """float64 reference and per-value bound of int16 ``pcm`` (n,) or (channels, n) for the arithmetic ``model`` of
    ``eb.MODELS`` (named by the caller: ``bf16x2/fp32`` for mfcc_fused512_h160_mb_kernel, ``fp32/fp32`` for the generic
    kernel).  ``output="logmel"``: the log-mel rows under the log-mel bound, as in framed_ref; ``lifter``: the cepstra
    times ``1 + (lifter / 2) sin(pi k / lifter)``, as in framed_ref."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        rb = [reference_and_bound(c, model, L, hop, nfft, n_mel, sample_rate, power_scale, n_cep, pad_mode, halo, output,
                                  low, high, lifter) for c in pcm]
        return np.stack([r for r, _ in rb]), np.stack([b for _, b in rb])
    x, drop = fr._frames_source(pcm, L, hop, pad_mode, halo)
    cep, st = banked_notebook(x, matrix(nfft, n_mel, sample_rate, low, high), L, hop, nfft, power_scale)
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
