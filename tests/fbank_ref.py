"""float64 reference and per-element error bound of the filterbank output (``MFCC.filterbank``) -- TEST INFRASTRUCTURE
ONLY (a plain module, not a conftest).

Reference.  ``E_ref = spectrum_ref.reference(...) @ W.T`` in float64: the power-spectrum reference of
tests/spectrum_ref.py contracted with the caller's matrix.

Bound per element, energy domain, with ``nnz_j`` the non-zero weights of band ``j``::

    B_E = W @ spectrum_ref.bound(P_ref)  +  G_j * E_ref            G_j = (nnz_j + 1) * 2^-24

The first term carries the per-bin spectrum bound (``C_SPEC = 8``, unchanged) through the non-negative weights.  ``G`` is
the contraction's own charge and is not tuned: both kernels sum ``fmaf(W[j][k], P[k], acc)`` in fp32 over the band's bins,
a chain of ``nnz_j`` roundings on non-negative terms, each at most ``2^-24`` of a running sum that never exceeds ``E``
(zeros inside a band's range add nothing); the ``+ 1`` covers the second-order terms of the chain.  The fused
512 kernel contracts in fp32 as well (kernel_fbank.hpp) when the packed weights fit its LDS, and is then held to the same
``G``.  A matrix that does not fit (:func:`form_of`) runs the kernel's bf16-split MFMA form and is held to
``G_j = 3 * 2^-17 + nnz_j * 2^-24``.

:func:`restatement_f32` and :func:`contract_bf16` restate the two arithmetics on the CPU (``spectrum_ref.restatement_f32``,
then the fp32 fma chain in ascending bin order, or the hi / lo split with the lo x lo term dropped and fp32 accumulation);
tests/test_fbank_host.py holds each to ``B_E / 2``.

Log scales, ``y_ref = c log2(max(E_ref, floor))``::

    |y - y_ref| <= c (log2(max(E_ref, floor) + B_E) - log2(max(E_ref - B_E, floor))) + c 2^-21 + 2^-23 |y_ref|

``2^-21`` is ``LOG2_ABS`` of tests/logmel_bound.py (v_log_f32); ``2^-23 |y_ref|`` covers the multiply by ``c`` and the
result's rounding.

Conditions (conditions, not tolerances).  An element enters the log comparison only when ``B_E <= E_ref / 4`` or ``E_ref
<= floor``; :func:`check_log` returns how many it set aside and the tests assert 0 on their inputs.  Exact results: an
all-zero frame and an empty band give ``+0.0`` in ENERGY scale, and in a log scale ``-inf`` (floor 0) or ONE value -- the
same bits in every such element -- within ``c 2^-21 + 2^-23 |y|`` of ``c log2(floor)``.  The checks refuse a NaN, a
negative energy and a shape mismatch, as ``spectrum_ref.check`` does.
"""
from __future__ import annotations

import numpy as np

import logmel_bound as lb
import spectrum_ref as sr

U = 2.0 ** -24
MAX_BANDS = 128
SCALES = {"energy": 0.0, "log2": 1.0, "ln": float(np.float32(np.log(2.0))), "log10": float(np.float32(np.log10(2.0)))}


# ---- matrices
def htk_weights(n_bands, nfft=512, samplerate=16000, fmin=0.0, fmax=None):
    """The HTK matrix in float64, rounded once to float32: ``(n_bands, nfft // 2 + 1)`` (include/mfcc_hip.h:
    ``mfcc_hip_create_banked``).  Written from the contract, not from the library."""
    fmax = samplerate / 2.0 if fmax is None else fmax
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)      # noqa: E731
    ml, mh = float(mel(fmin)), float(mel(fmax))
    e = ml + np.arange(n_bands + 2, dtype=np.float64) * (mh - ml) / float(n_bands + 1)
    m = mel(np.arange(nfft // 2 + 1, dtype=np.float64) * float(samplerate) / float(nfft))
    up = (m[None, :] - e[:-2, None]) / (e[1:-1] - e[:-2])[:, None]
    dn = (e[2:, None] - m[None, :]) / (e[2:] - e[1:-1])[:, None]
    v = np.minimum(up, dn)
    return np.where(v > 0.0, v, 0.0).astype(np.float32)


def edge_band(nfft=512):
    """One band with weight on bins 0 and nfft / 2 only."""
    w = np.zeros((1, nfft // 2 + 1), np.float32)
    w[0, 0], w[0, -1] = 0.75, 1.5
    return w


def dense_random(n_bands=128, nfft=512, seed=3):
    """Every weight positive: every bin of every band counts."""
    return np.random.default_rng(seed).uniform(0.05, 1.0, (n_bands, nfft // 2 + 1)).astype(np.float32)


def selections(nfft=512):
    """Matrices with one 1.0 per band that together pick every bin ``0 .. nfft / 2`` (the last one wraps around)."""
    bins = nfft // 2 + 1
    out = []
    for a in range(0, bins, MAX_BANDS):
        idx = (a + np.arange(min(MAX_BANDS, bins))) % bins
        w = np.zeros((len(idx), bins), np.float32)
        w[np.arange(len(idx)), idx] = 1.0
        out.append((idx, w))
    return out


def nnz(W):
    return (np.asarray(W) != 0).sum(axis=1)


def band_ranges(W):
    """(first non-zero bin, bins up to the last non-zero one) per band; (0, 0) for an empty band."""
    W = np.asarray(W)
    first, count = np.zeros(len(W), int), np.zeros(len(W), int)
    for j, row in enumerate(W):
        k = np.flatnonzero(row)
        if len(k):
            first[j], count[j] = k[0], k[-1] - k[0] + 1
    return first, count


K_WLDS = 3072             # fbank_plan.hpp: kWLds, the packed weights the fused kernel's fp32 form holds in LDS
FUSED = "mfcc_fbank512_kernel"
BLOCK, STEP, STEPS = 16, 32, 9


def form_of(W, kernel):
    """Which arithmetic contracts ``W``: ``"bf16"`` in the fused kernel when the bands' ranges add up to more than
    ``K_WLDS`` bins (its MFMA form), else ``"f32"``."""
    return "bf16" if kernel == FUSED and int(band_ranges(W)[1].sum()) > K_WLDS else "f32"


def g_of(W, form="f32"):
    """The contraction's charge per band: ``(nnz_j + 1) * 2^-24`` for the fp32 fma chain, ``3 * 2^-17 + nnz_j * 2^-24``
    for the bf16-split MFMA form (oracle/error_bound.py charges 2^-17 for the split, tests/logmel_bound.py adds
    ``BF16X2_MEL_EXTRA`` 2^-16 for a single band; the accumulation adds the rest)."""
    if form == "bf16":
        return 3.0 * 2.0 ** -17 + nnz(W) * U
    assert form == "f32"
    return (nnz(W) + 1.0) * U


def set_masks(W):
    """Brute force: bit ``s`` of block ``b`` is set when any of the block's 16 bands has a non-zero weight on the bins
    ``32 s .. 32 s + 31``."""
    W = np.asarray(W)
    masks = [0] * (MAX_BANDS // BLOCK)
    for j, k in zip(*np.nonzero(W)):
        masks[j // BLOCK] |= 1 << (k // STEP)
    return masks


def wide_selections(nfft=512):
    """:func:`selections` with a second 1.0 per band half a spectrum away: ``(idx, idx2, W)``.  Every band's range is at
    least 128 bins, so the fused kernel contracts these on its MFMA form."""
    bins = nfft // 2 + 1
    out = []
    for idx, w in selections(nfft):
        idx2 = (idx + bins // 2) % bins
        w = w.copy()
        w[np.arange(len(idx)), idx2] = 1.0
        out.append((idx, idx2, w))
    return out


# ---- reference and bound
def energy_ref_and_bound(p_ref, W, form="f32"):
    """``(E_ref, B_E)`` of a float64 power reference ``(..., frames, bins)`` and a matrix ``(n_bands, bins)``; ``form``:
    the arithmetic of the contraction (:func:`form_of`)."""
    W64 = np.asarray(W, dtype=np.float64)
    p_ref = np.asarray(p_ref, dtype=np.float64)
    e_ref = p_ref @ W64.T
    return e_ref, sr.bound(p_ref) @ W64.T + g_of(W, form) * e_ref


def reference_and_bound(pcm, W, nfft, hop, L, pad_mode="notebook", halo=0, form="f32"):
    return energy_ref_and_bound(sr.reference(pcm, nfft, hop, L, pad_mode=pad_mode, halo=halo), W, form)


def pinned_mask(zero_frames, W):
    """Boolean ``(..., frames, n_bands)``: the elements with an exact result -- all-zero frames and empty bands."""
    zero_frames = np.asarray(zero_frames, dtype=bool)
    return zero_frames[..., None] | (nnz(W) == 0)


def assert_not_blind(b_e, pinned, what=""):
    """``B_E`` is finite, 0 exactly in the pinned elements and positive everywhere else."""
    b_e = np.asarray(b_e)
    if b_e.shape != pinned.shape:
        raise AssertionError("%s: bound %s, pinned %s" % (what, b_e.shape, pinned.shape))
    if not np.isfinite(b_e).all() or (b_e < 0).any():
        raise AssertionError("%s: a bound that is negative or not finite" % what)
    if not np.array_equal(b_e == 0.0, pinned):
        raise AssertionError("%s: %d live element(s) with bound 0, %d pinned one(s) with a positive bound"
                             % (what, int(((b_e == 0) & ~pinned).sum()), int(((b_e != 0) & pinned).sum())))


def check_energy(got, e_ref, b_e, what="", limit=1.0):
    """ENERGY scale: the refusals of ``spectrum_ref.ratios`` (shape, NaN, negative or -0.0, anything but +0.0 where the
    bound is 0) and ``|got - E_ref| <= limit * B_E``; returns the worst ratio."""
    r = sr.ratios(got, e_ref, b_e)
    worst = float(r.max()) if r.size else 0.0
    if worst > limit:
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
        over = r > limit
        raise AssertionError("%s: %d element(s) over %.3g x their bound; worst ratio %.3g at %s: got %.9g, reference %.9g, "
                             "bound %.3g; failing bands: %s"
                             % (what or "filterbank", int(over.sum()), limit, worst, idx, float(np.asarray(got)[idx]),
                                float(e_ref[idx]), float(b_e[idx]), sorted(set(np.argwhere(over)[:, -1].tolist()))[:32]))
    return worst


def log_ref_and_bound(e_ref, b_e, scale, floor):
    """``(y_ref, bound, kept)`` of a log scale; ``kept``: the elements that enter the comparison."""
    c = SCALES[scale]
    floor = float(np.float32(floor))
    with np.errstate(divide="ignore", invalid="ignore"):
        top = np.maximum(e_ref, floor)
        y_ref = c * np.log2(top)
        lo = np.maximum(e_ref - b_e, floor)
        spread = np.log2(top + b_e) - np.log2(lo)
        bound = c * spread + c * lb.LOG2_ABS + 2.0 ** -23 * np.abs(y_ref)
    kept = (b_e <= e_ref / 4.0) | (e_ref <= floor)
    return y_ref, bound, kept


def check_log(got, e_ref, b_e, scale, floor, what="", limit=1.0):
    """A log scale: ``(worst ratio, elements set aside)``.  Pinned elements (``B_E == 0``) must all hold the same bits:
    ``-inf`` with floor 0, else a value within ``c 2^-21 + 2^-23 |y|`` of ``c log2(floor)``."""
    got = np.asarray(got)
    if got.shape != e_ref.shape or got.dtype != np.float32:
        raise AssertionError("%s: shape %s %s, reference %s" % (what, got.shape, got.dtype, e_ref.shape))
    if np.isnan(got).any():
        raise AssertionError("%s: %d NaN value(s)" % (what, int(np.isnan(got).sum())))
    y_ref, bound, kept = log_ref_and_bound(e_ref, b_e, scale, floor)
    pinned = b_e == 0.0
    if pinned.any():
        vals = np.unique(got[pinned].view(np.uint32))
        if len(vals) != 1:
            raise AssertionError("%s: all-zero frames and empty bands hold %d different values" % (what, len(vals)))
        v = float(vals.view(np.float32)[0])
        c, f = SCALES[scale], float(np.float32(floor))
        if f == 0.0:
            if v != -np.inf:
                raise AssertionError("%s: log of an exact 0 with floor 0 is %r, not -inf" % (what, v))
        else:
            want = c * np.log2(f)
            if not abs(v - want) <= c * lb.LOG2_ABS + 2.0 ** -23 * abs(want):
                raise AssertionError("%s: log of the floor is %r, not %r" % (what, v, want))
    live = kept & ~pinned
    if np.isinf(got[live]).any():
        raise AssertionError("%s: %d infinite value(s) in live elements" % (what, int(np.isinf(got[live]).sum())))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(live, np.abs(got.astype(np.float64) - y_ref) / np.where(live, bound, 1.0), 0.0)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= limit:
        idx = tuple(int(i) for i in np.unravel_index(int(np.nanargmax(r)), r.shape))
        raise AssertionError("%s: %d element(s) over %.3g x their log bound; worst %.3g at %s: got %.9g, reference %.9g, bound %.3g"
                             % (what, int((r > limit).sum()), limit, worst, idx, float(got[idx]), float(y_ref[idx]),
                                float(bound[idx])))
    return worst, int((~kept & ~pinned).sum())


def check(got, e_ref, b_e, scale, floor, what="", limit=1.0):
    """Either scale: ``(worst ratio, elements set aside)`` (ENERGY sets nothing aside)."""
    if scale == "energy":
        return check_energy(got, e_ref, b_e, what, limit), 0
    return check_log(got, e_ref, b_e, scale, floor, what, limit)


# ---- the arithmetic, restated
def contract_f32(p32, W):
    """The kernels' contraction on the CPU: per band ``acc = fma(W[j][k], P[k], acc)`` in fp32 from +0.0, ``k`` ascending
    over the band's bins.  The product of two fp32 values is exact in float64, so ``float32(w * p + acc)`` is the fused
    multiply-add up to a double rounding; a zero weight leaves ``acc`` as it is, so the loop may run over every bin."""
    p32 = np.asarray(p32, dtype=np.float32)
    W32 = np.asarray(W, dtype=np.float32)
    acc = np.zeros(p32.shape[:-1] + (len(W32),), np.float32)
    first, count = band_ranges(W32)
    k0, k1 = (int(first[count > 0].min()), int((first + count).max())) if (count > 0).any() else (0, 0)
    for k in range(k0, k1):
        acc = (p32[..., k:k + 1].astype(np.float64) * W32[:, k].astype(np.float64) + acc).astype(np.float32)
    return acc


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even, as v_cvt_pk_bf16_f32), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def contract_bf16(p32, W):
    """The MFMA form on the CPU: weights and power each split into bf16 ``hi + lo`` (``lo`` = the bf16 of what ``hi``
    lost), the ``lo x lo`` term dropped; per K step of 32 bins three products ``Wh Ph``, ``Wh Pl``, ``Wl Ph`` (bf16
    products are exact in float64), each summed over the step and added to the fp32 accumulator."""
    p32 = np.asarray(p32, dtype=np.float32)
    W32 = np.asarray(W, dtype=np.float32)
    wh = bf16_round(W32)
    wl = bf16_round(W32 - wh)
    ph = bf16_round(p32)
    pl = bf16_round(p32 - ph)
    acc = np.zeros(p32.shape[:-1] + (len(W32),), np.float32)
    for s in range(STEPS):
        k = slice(STEP * s, min(STEP * (s + 1), W32.shape[1]))
        for a, b in ((wh, ph), (wh, pl), (wl, ph)):
            acc = (acc + b[..., k].astype(np.float64) @ a[:, k].astype(np.float64).T).astype(np.float32)
    return acc


def restatement_f32(pcm, W, nfft, hop, L, pad_mode="notebook", halo=0):
    return contract_f32(sr.restatement_f32(pcm, nfft, hop, L, pad_mode=pad_mode, halo=halo), W)


def scale_f32(e32, scale, floor):
    """``c * log2(max(E, floor))`` in fp32 with NumPy's log2 (the kernels use v_log_f32, 1 ulp)."""
    if scale == "energy":
        return e32
    with np.errstate(divide="ignore"):
        return (np.float32(SCALES[scale]) * np.log2(np.maximum(e32, np.float32(floor)))).astype(np.float32)
