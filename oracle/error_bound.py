"""Per-coefficient error bound of the float contract -- TEST INFRASTRUCTURE ONLY.

The float contract's headline measure, max|got - ref| / max|ref|, lets every coefficient of every frame
drift by 1e-4 of the loudest frame's c0 (~5e-3 absolute on speech): a kernel that is wrong in one frame
per 16-frame tile passes it.  On ill-conditioned inputs (a DC offset with dither, a band that is a single
FFT bin) the same measure is too strict instead, and the suite used to set such bands aside by hand.

This module gives each coefficient of each frame its OWN bound, carried stage by stage through the
float64 oracle's intermediate values (:func:`oracle.mfcc_float.mfcc_notebook` with ``return_stages``),
for a declared model of the kernel's arithmetic:

* FFT, per bin:      e = C_FFT * u * rms(X) * log2(nfft)        u = 2^-24, rms over the frame's full spectrum
* mel band energy:   dE_b = sum_k W_bk (2 |X_k| e + e^2) + s_mel E_b
* log-mel:           dL_b = -log2(1 - dE_b / E_b)                (= dE_b / (E_b ln 2) to first order; no bound
                                                                  when dE_b >= E_b)
* coefficient:       B_fk = sum_b |D_kb| dL_b + (s_dct + C_ACC u) sum_b |D_kb| |L_b|, times the lifter weight

``s_mel`` / ``s_dct`` are 2^-17 for a contraction on bf16 x 2-split operands (W = Wh + Wl, P = Ph + Pl,
products Wh Ph + Wh Pl + Wl Ph with fp32 accumulation: what is dropped, Wl Pl and the two split
residuals, is <= 1.5 * 2^-17 of each non-negative product) and u for an fp32 one.  C_FFT and C_ACC are
fixed by this analysis, the same for every kernel and every test; they are not tuned per input.

Frames with a silent band (E_b = 0 and nothing that could make it non-zero: an all-zero frame) get no bound:
their -inf / NaN pattern must equal the oracle's exactly (bound NaN).  A frame with a band whose error bound
reaches its energy (dE_b >= E_b: a band that is float64 roundoff of an exact zero, such as every band away from
DC of a constant input) is not constrained at all (bound +inf): either arithmetic may give -inf there, or not.
``mfcc_amd`` and ``bench.py`` never import this module.
"""
from __future__ import annotations

import numpy as np

from oracle import mfcc_float as mf

U = 2.0 ** -24            # fp32 unit roundoff
C_FFT = 1.0               # FFT error per bin in units of u * rms(X) * log2(nfft)
C_ACC = 8.0               # log2, DCT accumulation and output rounding, in units of u * sum_b |D_kb| |L_b|
S_BF16X2 = 2.0 ** -17     # relative error of a bf16 x 2-split contraction of non-negative (mel) or any (DCT) terms
S_FP32 = U

# Declared arithmetic of each float kernel (mel contraction, DCT), read from its source.
MODELS = {
    "bf16x2/bf16x2": ("bf16x2", "bf16x2"),   # mfcc_fused512_w12_kernel
    "bf16x2/fp32": ("bf16x2", "fp32"),       # mfcc_fused512_kernel (four-wave form); fused 1024 w12bf / bf16
    "fp32/fp32": ("fp32", "fp32"),           # fused 1024 w12 / f32; every generic kernel
}
KERNEL_MODEL = {
    "mfcc_fused512_w12_kernel": "bf16x2/bf16x2",
    "mfcc_fused512_kernel": "bf16x2/fp32",
    "mfcc_fused1024_w12bf_kernel": "bf16x2/fp32",
    "mfcc_fused1024_w12_kernel": "fp32/fp32",
    # mfcc_fused1024_kernel is the eight-wave form of EITHER contraction (MFCC_HIP_FUSED1024=bf16 / f32): the
    # caller declares which; generic kernels: see model_of()
}


def model_of(kernel_name: str, fused1024_form: str | None = None) -> str:
    """The declared model of a kernel, by the name the library reports (``MFCC.kernel_name()``)."""
    if kernel_name in KERNEL_MODEL:
        return KERNEL_MODEL[kernel_name]
    if kernel_name == "mfcc_fused1024_kernel":
        if fused1024_form not in ("bf16", "f32"):
            raise ValueError("mfcc_fused1024_kernel runs either contraction: name the form (bf16 / f32)")
        return "bf16x2/fp32" if fused1024_form == "bf16" else "fp32/fp32"
    if kernel_name.endswith("generic_kernel"):
        return "fp32/fp32"
    raise KeyError("no declared arithmetic model for kernel %r" % kernel_name)


def _scale(kind):
    return S_BF16X2 if kind == "bf16x2" else S_FP32


def bound_from_stages(st, model, n_cep, lifter=0.0):
    """(frames, n_cep) bound from the oracle's float64 stages of one channel; NaN rows = frames with a silent band."""
    mel_kind, dct_kind = MODELS[model]
    power = np.asarray(st["power"], dtype=np.float64)          # (frames, nfft/2 + 1), after power_scale
    W = np.asarray(st["filters"], dtype=np.float64)            # (n_mel, nfft/2 + 1)
    E = np.asarray(st["mel"], dtype=np.float64)                # (frames, n_mel)
    L = np.asarray(st["logmel"], dtype=np.float64)
    D = np.abs(np.asarray(st["dct_basis"], dtype=np.float64)[:n_cep])
    nfft = 2 * (power.shape[1] - 1)
    if len(power) == 0:
        return np.zeros((0, n_cep))
    # rms over the full nfft-bin spectrum (bins 1 .. nfft/2 - 1 appear twice)
    full = power[:, 0] + power[:, -1] + 2.0 * power[:, 1:-1].sum(axis=1)
    rms = np.sqrt(full / nfft)
    e = C_FFT * U * rms * np.log2(nfft)                          # (frames,)
    dE = (np.sqrt(power) * (2.0 * e[:, None])) @ W.T + (e * e)[:, None] * W.sum(axis=1)[None, :] \
        + _scale(mel_kind) * E
    silent = ((E <= 0) & (dE <= 0)).any(axis=1)               # an all-zero frame: E_b = 0 in any arithmetic
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E > 0, dE / np.where(E > 0, E, 1.0), np.where(dE > 0, np.inf, 0.0))
        dL = np.where(r < 1.0, -np.log2(np.maximum(1.0 - r, 1e-300)), np.inf)
        absL = np.where(np.isfinite(L), np.abs(L), 0.0)
    B = dL @ D.T + (_scale(dct_kind) + C_ACC * U) * (absL @ D.T)
    if lifter:
        B = B * np.abs(1.0 + (lifter / 2.0) * np.sin(np.pi * np.arange(n_cep) / lifter))[None, :]
    B[(r >= 1.0).any(axis=1)] = np.inf                         # a band's energy could be 0: log-mel undetermined
    B[silent] = np.nan
    return B


def _frames_source(x, nfft, hop, pad_mode, halo):
    """The sample stream whose notebook framing gives the kernel's frames (``frames_to_drop`` leading ones)."""
    x = np.asarray(x)
    if halo:            # sample 0 is history only: put it one hop into a longer stream, drop that stream's frame 0
        x = np.concatenate([np.zeros(hop - 1, dtype=x.dtype), x])
    if pad_mode == "stream":
        nf = mf.num_frames_stream(len(x), nfft, hop)
        x = np.concatenate([x, np.zeros((nf - 1) * hop + nfft - len(x), dtype=x.dtype)])
    elif pad_mode != "notebook":
        raise ValueError(pad_mode)
    return x, int(bool(halo))


def reference_and_bound(pcm, model, n_cep=13, pad_mode="notebook", lifter=0.0, halo=0, **notebook_kw):
    """float64 oracle and per-coefficient bound for int16 ``pcm`` of shape (n,) or (channels, n).

    ``notebook_kw`` go to :func:`oracle.mfcc_float.mfcc_notebook` (nfft, hop, n_mel, sample_rate,
    power_scale).  ``halo=1``: sample 0 of every channel is pre-emphasis history only (the device path's
    ``halo``).  Returns ``(ref, bound)``, both float64 (channels?, frames, n_cep)."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        rb = [reference_and_bound(c, model, n_cep, pad_mode, lifter, halo, **notebook_kw) for c in pcm]
        return np.stack([r for r, _ in rb]), np.stack([b for _, b in rb])
    if model not in MODELS:
        raise KeyError(model)
    nfft = notebook_kw.get("nfft", 512)
    hop = notebook_kw.get("hop", 170)
    x, drop = _frames_source(pcm, nfft, hop, pad_mode, halo)
    out, st = mf.mfcc_notebook(x, return_stages=True, **notebook_kw)
    st = dict(st, power=st["power"][drop:], mel=st["mel"][drop:], logmel=st["logmel"][drop:])
    ref = mf.lifter(out[drop:, :n_cep], lifter) if lifter else out[drop:, :n_cep]
    if len(ref) == 0:
        return ref, np.zeros_like(ref)
    return ref, bound_from_stages(st, model, n_cep, lifter)


def ratios(got, ref, bound):
    """|got - ref| / bound where a bound applies (NaN elsewhere), after the -inf / NaN pattern check."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    if got.shape != ref.shape or ref.shape != bound.shape:
        raise AssertionError("shape %s, oracle %s, bound %s" % (got.shape, ref.shape, bound.shape))
    fin = np.isfinite(ref)
    bad = (np.isfinite(got) != fin) | (~fin & ~np.isnan(ref) & (got != ref)) | (np.isnan(ref) & ~np.isnan(got))
    bad &= ~np.isposinf(bound)                                   # frames the model cannot pin down at all
    if bad.any():
        idx = np.argwhere(bad)[0]
        raise AssertionError("-inf / NaN pattern differs from the oracle at %d place(s); first %s: got %r, oracle %r"
                             % (int(bad.sum()), tuple(int(i) for i in idx), got[tuple(idx)], ref[tuple(idx)]))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(fin & np.isfinite(bound), np.abs(got - ref) / bound, np.nan)
    return r


def unbounded_frames(bound):
    """Frames of ``bound`` (..., frames, n_cep) that the model leaves unconstrained (see the module docstring)."""
    return np.isposinf(np.asarray(bound)).all(axis=-1)


def max_ratio(got, ref, bound):
    r = ratios(got, ref, bound)
    return float(np.nanmax(r)) if np.isfinite(r).any() else 0.0


def check(got, ref, bound, what=""):
    """Assert the -inf / NaN pattern and |got - ref| <= bound everywhere; returns the largest ratio.

    The failure message names the worst (channel, frame, coefficient) and gives a histogram of the failing
    frames by frame % 16 (the tile column of the fused kernels)."""
    r = ratios(got, ref, bound)
    r3 = r.reshape((-1,) + r.shape[-2:]) if r.ndim >= 2 else r.reshape(1, 1, -1)
    worst = float(np.nanmax(r3)) if np.isfinite(r3).any() else 0.0
    if worst > 1.0:
        c, f, k = (int(i) for i in np.unravel_index(np.nanargmax(r3), r3.shape))
        g3 = np.asarray(got, np.float64).reshape(r3.shape)
        f3 = np.asarray(ref, np.float64).reshape(r3.shape)
        b3 = np.asarray(bound, np.float64).reshape(r3.shape)
        over = r3 > 1.0
        fail_frames = np.argwhere(over.any(axis=2))[:, 1]
        hist = np.bincount(fail_frames % 16, minlength=16)
        coefs = np.bincount(np.argwhere(over)[:, 2], minlength=r3.shape[2])
        raise AssertionError(
            "%s: %d coefficient(s) over their bound in %d frame(s); worst ratio %.3g at (channel %d, frame %d, coef %d): "
            "got %.9g, oracle %.9g, bound %.3g; failing frames by frame %% 16: %s; failing coefficients: %s"
            % (what or "error bound", int(over.sum()), len(fail_frames), worst, c, f, k, g3[c, f, k], f3[c, f, k],
               b3[c, f, k], hist.tolist(), coefs.tolist()))
    return worst


def check_stream(got, pcm, model, n_cep=13, chunk=8000, what="", **notebook_kw):
    """check() of one long channel (notebook framing), the oracle run on ``chunk`` frames at a time: a chunk after the
    first starts one sample early, with ``halo=1``, so that its first frame has its pre-emphasis history.  Returns
    the largest ratio."""
    nfft = notebook_kw.get("nfft", 512)
    hop = notebook_kw.get("hop", 170)
    worst = 0.0
    for f0 in range(0, len(got), chunk):
        f1 = min(len(got), f0 + chunk)
        lo = 0 if f0 == 0 else hop * f0 - 1
        ref, bound = reference_and_bound(pcm[lo:hop * (f1 - 1) + nfft], model, n_cep, halo=int(f0 > 0), **notebook_kw)
        if len(ref) != f1 - f0:
            raise AssertionError("%s: frames %d..%d, oracle has %d" % (what, f0, f1, len(ref)))
        worst = max(worst, check(got[f0:f1], ref, bound, "%s frames %d..%d" % (what, f0, f1)))
    return worst
