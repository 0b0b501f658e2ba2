"""NumPy restatement of the energy VAD rule of include/mfcc_hip.h (Kaldi's ComputeVadEnergy) and the rule by which a
GPU result is compared with it -- TEST INFRASTRUCTURE ONLY (a plain module, not a conftest).

The rule, per segment of T rows, on ``e_t`` = one column of the raw rows::

    F        = the finite e_t
    theta    = float64(threshold) + float64(scale) * mean(F)        mean in float64; scale 0: no mean is taken;
                                                                    scale != 0 and F empty: every frame unvoiced
    above_t  = isfinite(e_t) and float64(e_t) > theta
    num, den = above frames / all frames of [t - ctx, t + ctx] clipped to [0, T)
    voiced_t = float32(num) >= float32(den) * float32(p)            one fp32 multiply

The set-aside rule.  The library adds the finite values in another order than ``np.sum`` does, so the two float64 means
may differ by up to ``n * 2^-53`` relative and a frame whose ``e_t`` lies that close to theta may fall on the other side.
A frame is *undecided* when ``|e_t - theta| <= 2^-30 * (|threshold| + scale * max|F|)`` -- far above that difference for
any segment under 2^23 rows.  Frames within ``ctx`` of an undecided frame may differ from this reference; every other frame
must match it exactly.  The share of frames set aside this way may not exceed ``MAX_SET_ASIDE`` of the frames of a case:
zero frames for any case under a million frames, and ``compare`` fails when it is exceeded.
"""
from __future__ import annotations

import numpy as np

DEFAULTS = dict(energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6)   # Kaldi's
MAX_SET_ASIDE = 1e-6
_MARGIN = 2.0 ** -30


def segment(e, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
    """One segment: ``e`` (T,) -> (voiced uint8 (T,), may_differ bool (T,), theta)."""
    e32 = np.asarray(e, dtype=np.float32)
    e = e32.astype(np.float64)
    T = len(e)
    thr, scale = np.float64(np.float32(energy_threshold)), np.float64(np.float32(energy_mean_scale))
    ctx, p = int(frames_context), np.float32(proportion_threshold)
    fin = np.isfinite(e)
    if scale == 0.0:
        theta = thr
    elif not fin.any():
        theta = np.float64(np.inf)
    else:
        theta = thr + scale * (np.sum(e[fin], dtype=np.float64) / np.float64(fin.sum()))
    with np.errstate(invalid="ignore"):
        above = fin & (e > theta)
    cs = np.concatenate([[0], np.cumsum(above, dtype=np.int64)])
    t = np.arange(T)
    a, b = np.maximum(t - ctx, 0), np.minimum(t + ctx, T - 1) + 1
    num, den = cs[b] - cs[a], b - a
    voiced = (num.astype(np.float32) >= den.astype(np.float32) * p).astype(np.uint8)
    # undecided frames and the frames whose window holds one
    if fin.any() and np.isfinite(theta):
        margin = _MARGIN * (abs(thr) + scale * np.abs(e[fin]).max())
        und = fin & (np.abs(np.where(fin, e, 0.0) - theta) <= margin)
    else:
        und = np.zeros(T, bool)
    cu = np.concatenate([[0], np.cumsum(und, dtype=np.int64)])
    may_differ = (cu[b] - cu[a]) > 0
    return voiced, may_differ, theta


def vad(rows, offsets=None, column=0, **params):
    """``rows`` (R, W) (or a column (R,)), segment k = rows ``offsets[k]:offsets[k + 1]`` (one segment without offsets)
    -> (voiced uint8 (R,), may_differ bool (R,)); rows outside the segments: voiced 0, may_differ False."""
    rows = np.asarray(rows)
    col = rows if rows.ndim == 1 else rows[:, column]
    if offsets is None:
        offsets = [0, len(col)]
    voiced = np.zeros(len(col), np.uint8)
    may = np.zeros(len(col), bool)
    for a, b in zip(offsets[:-1], offsets[1:]):
        a, b = int(a), int(b)
        if b > a:
            voiced[a:b], may[a:b], _ = segment(col[a:b], **params)
    return voiced, may


def compare(got, rows, offsets=None, column=0, what="", **params):
    """``got`` (R,) uint8 against the reference under the set-aside rule.  Returns (set-aside share, voiced share)."""
    got = np.asarray(got)
    ref, may = vad(rows, offsets, column, **params)
    assert got.shape == ref.shape and got.dtype == np.uint8, (what, got.shape, got.dtype, ref.shape)
    assert int(got.max(initial=0)) <= 1, "%s: a byte that is neither 0 nor 1" % what
    off = [0, len(ref)] if offsets is None else offsets
    frames = int(off[-1]) - int(off[0])
    share = float(may.sum()) / max(frames, 1)
    assert share <= MAX_SET_ASIDE, "%s: %d of %d frames set aside (%.3g > %.3g)" % (what, may.sum(), frames, share,
                                                                                    MAX_SET_ASIDE)
    bad = np.flatnonzero((got != ref) & ~may)
    assert len(bad) == 0, "%s: %d frame(s) differ from the reference, first at row %d: got %d, reference %d" % (
        what, len(bad), bad[0], got[bad[0]], ref[bad[0]])
    return share, float(ref[int(off[0]):int(off[-1])].mean()) if frames else 0.0
