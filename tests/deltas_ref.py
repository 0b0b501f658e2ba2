"""float64 NumPy reference of the delta pass (include/mfcc_hip.h: mfcc_hip_set_deltas / mfcc_hip_deltas_dev) and the
bounds the GPU result is held to -- TEST INFRASTRUCTURE ONLY (never imported by mfcc_amd or bench.py).

Per segment of L rows and column j, with window N and r = 1 / (2 sum_{n=1..N} n^2):
    D_t = r * sum_{n=1..N} n (s_{c(t+n)} - s_{c(t-n)}),   c(i) = min(max(i, 0), L - 1)   (HTK's edge rule)
and DD is the same formula on D.  A row of a segment expands to [s | D | DD (order 2)].

Stage bound.  The GPU computes one stage on fp32 inputs a_n = s_{c(t+n)}, b_n = s_{c(t-n)} as
    acc = 0; for n = 1..N: acc = fmaf(n, a_n - b_n, acc);  D = acc * fl(r)
One rounding per difference (N), one per fma (N, the first of which is exact but counted), fl(r) and the product
(2): to first order (N + 3) u r sum_n n (|a_n| + |b_n|) with u = 2^-24, every rounded partial sum being at most
r sum_n n (|a_n| + |b_n|) / r.  The bound takes (N + 4) u to cover the second-order terms:
    |D_gpu - D_64(s_gpu)| <= (N + 4) 2^-24 r sum_n n (|s_{c(t+n)}| + |s_{c(t-n)}|)
DD is held to the same bound against D_64 applied to the GPU's own D rows.

End-to-end bound, with B the per-coefficient bound of oracle.error_bound.reference_and_bound on the static rows:
    B_D(t)  = r sum_n n (B_{c(t+n)} + B_{c(t-n)}) + stage bound evaluated at |ref| + B
    B_DD(t) = the same with B_D in place of B, evaluated at |D_ref| + B_D
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def scale(window):
    return 1.0 / (2.0 * sum(n * n for n in range(1, window + 1)))


def _segments(offsets):
    off = [int(v) for v in offsets]
    return [(a, b) for a, b in zip(off[:-1], off[1:]) if b > a]


def _taps(L, window):
    """(n, index of t + n, index of t - n) for n = 1..window, clamped to [0, L)."""
    t = np.arange(L)
    return [(n, np.clip(t + n, 0, L - 1), np.clip(t - n, 0, L - 1)) for n in range(1, window + 1)]


def delta(rows, offsets, window):
    """One stage in float64 over the segments of ``rows`` (R, W); rows outside the segments are 0."""
    x = np.asarray(rows, dtype=np.float64)
    d = np.zeros_like(x)
    r = scale(window)
    with np.errstate(invalid="ignore"):
        for a, b in _segments(offsets):
            s = x[a:b]
            acc = np.zeros_like(s)
            for n, p, q in _taps(b - a, window):
                acc += n * (s[p] - s[q])
            d[a:b] = acc * r
    return d


def deltas(rows, offsets, order=2, window=2):
    """The expanded float64 rows [s | D | DD] (R, W * (1 + order)) of ``rows`` (R, W)."""
    x = np.asarray(rows, dtype=np.float64)
    parts = [x]
    d = delta(x, offsets, window)
    parts.append(d)
    if order == 2:
        parts.append(delta(d, offsets, window))
    return np.concatenate(parts, axis=1)


def nonfinite_after(bad, offsets, window):
    """Which D elements are non-finite, given which of its inputs are: any of the 2N clamped neighbours."""
    bad = np.asarray(bad, dtype=bool)
    out = np.zeros_like(bad)
    for a, b in _segments(offsets):
        m = bad[a:b]
        acc = np.zeros_like(m)
        for _n, p, q in _taps(b - a, window):
            acc |= m[p] | m[q]
        out[a:b] = acc
    return out


def finite_pattern(rows, offsets, order=2, window=2):
    """The finite pattern the expanded rows must have (True = finite)."""
    bad = ~np.isfinite(np.asarray(rows))
    parts = [bad]
    d = nonfinite_after(bad, offsets, window)
    parts.append(d)
    if order == 2:
        parts.append(nonfinite_after(d, offsets, window))
    return ~np.concatenate(parts, axis=1)


def emulate32(rows, offsets, order=2, window=2):
    """The specified fp32 sequence on the CPU (the fma as the float64 sum of the exact product n * (a - b) and acc,
    rounded to fp32): what the kernel computes, up to a rare double rounding in that emulated fma."""
    x = np.asarray(rows, dtype=np.float32)
    r32 = np.float32(scale(window))

    def stage(s_all):
        out = np.zeros_like(s_all)
        with np.errstate(invalid="ignore", over="ignore"):
            for a, b in _segments(offsets):
                s = s_all[a:b]
                acc = np.zeros_like(s)
                for n, p, q in _taps(b - a, window):
                    diff = s[p] - s[q]                                               # fp32
                    acc = (np.float64(n) * diff.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
                out[a:b] = acc * r32
        return out

    parts = [x, stage(x)]
    if order == 2:
        parts.append(stage(parts[1]))
    return np.concatenate(parts, axis=1)


def stage_bound(s, offsets, window):
    """(N + 4) 2^-24 r sum_n n (|s_{c(t+n)}| + |s_{c(t-n)}|) over the segments of ``s`` (R, W), float64."""
    return (window + 4) * U * delta_abs(s, offsets, window)


def delta_abs(s, offsets, window):
    """r sum_n n (|s_{c(t+n)}| + |s_{c(t-n)}|): the stage applied to magnitudes, every term added."""
    x = np.abs(np.asarray(s, dtype=np.float64))
    out = np.zeros_like(x)
    r = scale(window)
    with np.errstate(invalid="ignore"):
        for a, b in _segments(offsets):
            m = x[a:b]
            acc = np.zeros_like(m)
            for n, p, q in _taps(b - a, window):
                acc += n * (m[p] + m[q])
            out[a:b] = acc * r
    return out


def _within(got, ref, bound, fin, what):
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        r = np.where(fin, np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)), 0.0)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= 1.0:
        i = np.unravel_index(int(np.nanargmax(np.where(np.isnan(r), np.inf, r))), r.shape)
        raise AssertionError("%s: |got - ref| exceeds the bound %.3gx at %s: got %r, ref %r, bound %g"
                             % (what, worst, i, got[i], ref[i], bound[i]))
    return worst


def _rows_in(offsets, R):
    m = np.zeros(R, dtype=bool)
    for a, b in _segments(offsets):
        m[a:b] = True
    return m


def check_stage(got, rows, offsets, order=2, window=2, what=""):
    """``got`` (R, W (1 + order)) against the static ``rows`` (R, W) it was computed from, over the rows of the
    segments: the static columns bit for bit, the finite pattern exactly, D within the stage bound of D_64(rows) and
    DD within the stage bound of D_64(got's own D).  Returns the worst error / bound ratio."""
    rows = np.asarray(rows, dtype=np.float32)
    R, W = rows.shape
    got = np.asarray(got, dtype=np.float32).reshape(R, W * (1 + order))
    seg = _rows_in(offsets, R)
    if not np.array_equal(got[seg, :W].view(np.uint32), rows[seg].view(np.uint32)):
        raise AssertionError("%s: the static columns differ from the static rows" % what)
    want = finite_pattern(rows, offsets, order, window)[seg]
    have = np.isfinite(got[seg])
    if not np.array_equal(have, want):
        raise AssertionError("%s: the finite pattern differs at %d place(s)" % (what, int((have != want).sum())))
    fin = np.isfinite(got)
    d_gpu = got[:, W:2 * W]
    worst = _within(d_gpu, delta(rows, offsets, window), stage_bound(rows, offsets, window), fin[:, W:2 * W] & seg[:, None],
                    what + " D")
    if order == 2:
        worst = max(worst, _within(got[:, 2 * W:], delta(d_gpu, offsets, window), stage_bound(d_gpu, offsets, window),
                                   fin[:, 2 * W:] & seg[:, None], what + " DD"))
    return worst


def end_to_end_bound(ref, B, offsets, order=2, window=2):
    """Per-element bound (R, W (1 + order)) of the GPU's expanded rows against deltas(ref): B on the statics, then
    B_D and B_DD as in the module docstring."""
    ref = np.asarray(ref, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    parts = [B]
    B_d = delta_abs(B, offsets, window) + stage_bound(np.abs(ref) + B, offsets, window)
    parts.append(B_d)
    if order == 2:
        d_ref = delta(ref, offsets, window)
        parts.append(delta_abs(B_d, offsets, window) + stage_bound(np.abs(d_ref) + B_d, offsets, window))
    return np.concatenate(parts, axis=1)


def check_end_to_end(got, ref, B, offsets, order=2, window=2, what=""):
    """|got - deltas(ref)| <= end_to_end_bound element by element; every bound must be finite (no frame unbounded)."""
    b = end_to_end_bound(ref, B, offsets, order, window)
    if not np.isfinite(b).all():
        raise AssertionError("%s: %d element(s) have no finite bound" % (what, int((~np.isfinite(b)).sum())))
    z = deltas(ref, offsets, order, window)
    got = np.asarray(got, dtype=np.float64).reshape(z.shape)
    if not np.isfinite(got).all():
        raise AssertionError("%s: non-finite values where the reference is finite" % what)
    return _within(got, z, b, np.ones(z.shape, dtype=bool), what)
