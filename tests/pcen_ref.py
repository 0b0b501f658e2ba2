"""References for PCEN (include/mfcc_hip.h: mfcc_hip_set_pcen / mfcc_hip_pcen_dev).

``pcen_f64``    the definition: a sequential float64 recurrence per column, no tiles
``pcen_tiled``  a NumPy fp32 restatement of the tile form the kernels compute (fmaf through float64: the product of two
                fp32 values is exact there)
``check``       |got - ref| <= C * (|ref| + delta^r), written with <= so that delta = 0 works

Rows are log2 energies ``[frames][width]``; a non-finite entry counts as E = 0.  Segment ``k`` is rows
``off[k]:off[k + 1]``.  The parameters are taken as the fp32 values the library sees.
"""
import math

import numpy as np

TILE = 128
DEFAULTS = (0.025, 0.98, 2.0, 0.5, 1e-6)                     # s, alpha, delta, r, eps (Wang et al. 2017)
# the parameter sets of the tests: the defaults, a fast strong-bias set, s = 1 (M = E), and a slow set without bias or root
PARAM_SETS = [DEFAULTS, (0.04, 0.8, 10.0, 0.25, 1e-6), (1.0, 0.98, 2.0, 0.5, 1e-6), (0.005, 1.0, 0.0, 1.0, 1e-3)]

# The bound's constant.  Worst |tiled - f64| / (|f64| + delta^r) of the restatement over PARAM_SETS on the golden
# recording's log-mel rows with silent entries (golden_rows below; tests/test_pcen_host.py measures it again): 1.54e-6
# (per set: 8.4e-7, 3.2e-7, 1.9e-7, 1.54e-6).  The device's log2
# and exp2 may each be an ulp off and r * log2(u) reaches magnitudes near 40, so the tests allow 8 times that; the float
# contract of the project, 1e-4, is the ceiling.
MEASURED = 1.54e-6
C = 8 * MEASURED
assert C <= 1e-4


def f32(v):
    return float(np.float32(v))


def golden_rows(golden_dir):
    """The golden recording's log-mel rows (1046 x 32, log2 energies) as fp32 with silent entries: 2 % of all entries,
    band 5 in frame 0 (C_0 = 0) and band 7 over 200 frames."""
    import os
    x = np.load(os.path.join(golden_dir, "f2bjrop_float64_logmel32.npy")).astype(np.float32)
    rng = np.random.default_rng(0)
    x[rng.random(x.shape) < 0.02] = -np.inf
    x[0, 5] = -np.inf
    x[300:500, 7] = -np.inf
    return x


def constants(s, delta, r):
    """(decay[TILE], a, delta_r) as mfcc_hip_pcen_constants defines them: float64 pow, rounded once."""
    d = 1.0 - f32(s)
    decay = np.array([math.pow(d, k + 1.0) for k in range(TILE)]).astype(np.float32)
    return decay, np.float32(d), np.float32(math.pow(f32(delta), f32(r)))


def _segs(x, off):
    x = np.asarray(x)
    assert x.ndim == 2
    if off is None:
        off = [0, len(x)]
    return x, [int(o) for o in off]


def pcen_f64(x, off=None, s=DEFAULTS[0], alpha=DEFAULTS[1], delta=DEFAULTS[2], r=DEFAULTS[3], eps=DEFAULTS[4]):
    """The definition in float64.  Rows outside the segments come back as they are."""
    x, off = _segs(x, off)
    s, alpha, delta, r, eps = (f32(v) for v in (s, alpha, delta, r, eps))
    y = np.array(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        E = np.where(np.isfinite(x), np.exp2(np.asarray(x, dtype=np.float64)), 0.0)
    for a, b in zip(off[:-1], off[1:]):
        M = None
        for t in range(a, b):
            M = E[t].copy() if M is None else (1.0 - s) * M + s * E[t]
            y[t] = (E[t] / (eps + M) ** alpha + delta) ** r - delta ** r
    return y


def _fmaf(a, b, c):
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def pcen_tiled(x, off=None, s=DEFAULTS[0], alpha=DEFAULTS[1], delta=DEFAULTS[2], r=DEFAULTS[3], eps=DEFAULTS[4]):
    """The tile form in fp32, operation for operation (NumPy's log2 / exp2 in place of the hardware's)."""
    x, off = _segs(x, off)
    x = np.asarray(x, dtype=np.float32)
    decay, a_, d_r = constants(s, delta, r)
    s, alpha, delta, r, eps = (np.float32(v) for v in (s, alpha, delta, r, eps))
    y = x.copy()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        E = np.where(np.isfinite(x), np.exp2(x), np.float32(0)).astype(np.float32)
        for a, b in zip(off[:-1], off[1:]):
            if b <= a:
                continue
            C_i = E[a].copy()
            L = np.zeros(x.shape[1], dtype=np.float32)
            for t in range(a, b):
                k = (t - a) % TILE
                if k == 0:
                    L[:] = 0
                L = _fmaf(a_, L, s * E[t])
                M = _fmaf(decay[k], C_i, L)
                g = np.log2(eps + M)
                q = np.exp2(-alpha * g)
                u = _fmaf(E[t], q, delta)
                y[t] = np.exp2(r * np.log2(u)) - d_r
                if k == TILE - 1:
                    C_i = M
    return y


def error(got, ref, delta, r, rows=None):
    """Worst |got - ref| / (|ref| + delta^r) over ``rows`` (a mask or slice; default all); a zero denominator demands
    got == ref and counts as 0.  Asserts that every value is finite."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), "non-finite PCEN output"
    den = np.abs(ref) + f32(delta) ** f32(r)
    diff = np.abs(got - ref)
    assert np.all(diff[den == 0] == 0), "a value that must be exactly 0 is not"
    return float(np.max(diff[den > 0] / den[den > 0])) if np.any(den > 0) else 0.0


def check(got, ref, delta, r, rows=None, c=C, what=""):
    """|got - ref| <= c (|ref| + delta^r) everywhere; returns the worst ratio for reports."""
    got64 = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref, dtype=np.float64)
    if rows is not None:
        got64, ref64 = got64[rows], ref64[rows]
    e = error(got64, ref64, delta, r)
    bad = np.abs(got64 - ref64) > c * (np.abs(ref64) + f32(delta) ** f32(r))
    assert not np.any(bad), "%s: %d values outside the bound, worst %.3g of allowed %.3g" % (what, int(bad.sum()), e, c)
    return e
