"""float64 NumPy reference of sliding-window normalization (include/mfcc_hip.h: mfcc_hip_set_normalize_window,
mfcc_hip_normalize_sliding_dev) and the per-element bound the GPU result is held to -- TEST INFRASTRUCTURE ONLY.

Row t of a segment of T rows is standardized with the statistics of rows [a, b) of the same segment (``window``
below: the rule of Kaldi's SlidingWindowCmn), per column over the finite values of those rows: mu = mean, sigma =
population std, sigma' = 1 where sigma < 10 * 2^-52 -- ``normalize_ref.stats`` on rows [a, b).  MEAN: y = x - mu;
MEAN_VAR: y = (x - mu) / sigma'.  Non-finite x stay as they are and are left out of every window that covers them.

Two evaluations of that definition.  ``method="direct"`` calls ``normalize_ref.stats`` on rows [a, b) of every row:
O(T N W), the definition itself, for the CPU tests.  ``method="tree"`` (the default) gives the same numbers in
O(T W log T), for full-size results and long windows: (n, mean, M2) of every aligned block of 2^j rows, built bottom
up with the pairwise update of Chan, Golub and LeVeque, and every window combined from the at most 2 log2 T blocks
that tile it with the same update.  No sum of x or x^2 is formed and no two large numbers are subtracted: like the
direct form it keeps the variance of a column of 1e4 + 1e-2 noise.  tests/test_normalize_sliding_host.py holds the
two forms together.

The bound is ``normalize_ref.bound`` unchanged, 2^-22 (|mu| + |x - mu|) / sigma' with the row's own mu and sigma':
nothing in its derivation depends on which rows the statistics came from.
"""
from __future__ import annotations

import numpy as np

import normalize_ref as nr

MEAN, MEAN_VAR = nr.MEAN, nr.MEAN_VAR
_MODES = nr._MODES
_EPS10 = 10 * np.finfo(np.float64).eps


def window(t, T, N, M, center):
    """Rows [a, b) whose statistics standardize row t of a segment of T rows; a <= t < b."""
    if center:
        a = t - N // 2
        b = a + N
    else:
        a = t - N
        b = t + 1                       # Kaldi's causal window holds N + 1 frames
    if a < 0:
        b -= a
        a = 0
    if not center and b > t:
        b = max(t + 1, M)               # M only acts on the first frames of the causal form
    if b > T:
        a -= b - T
        b = T
        a = max(a, 0)
    return a, b


def windows(T, N, M, center):
    return [window(t, T, N, M, center) for t in range(T)]


def _windows_np(T, N, M, center):
    """``window`` for t = 0 .. T - 1 at once."""
    t = np.arange(T, dtype=np.int64)
    if center:
        a = t - N // 2
        b = a + N
    else:
        a = t - N
        b = t + 1
    neg = a < 0
    b = np.where(neg, b - a, b)
    a = np.where(neg, 0, a)
    if not center:
        b = np.maximum(t + 1, M)
    over = b > T
    a = np.where(over, np.maximum(a - (b - T), 0), a)
    b = np.where(over, T, b)
    return a, b


def _segment_direct(x, N, M, center):
    """(mu, sigma') per row of one segment x (T, width): normalize_ref.stats on rows [a, b).  mu is 0 for a column
    without a finite value in the window."""
    T = len(x)
    mu_r, sd_r = np.zeros_like(x), np.ones_like(x)
    last, mu_f, sd = None, None, None
    for t in range(T):
        ab = window(t, T, N, M, center)
        if ab != last:                  # consecutive rows of a short segment share their window
            mu, sd = nr.stats(x[ab[0]:ab[1]])
            mu_f = np.where(np.isfinite(mu), mu, 0.0)
            last = ab
        mu_r[t] = mu_f
        sd_r[t] = sd
    return mu_r, sd_r


def _chan(n1, m1, q1, n2, m2, q2):
    """(n, mean, M2) of the union of two sets; a set with n = 0 has mean = M2 = 0 and leaves the other unchanged."""
    n = n1 + n2
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(n > 0, n2 / n, 0.0)
    d = m2 - m1
    return n, m1 + d * f, q1 + q2 + d * d * (n1 * f)


def _segment_tree(x, N, M, center):
    T, W = x.shape
    fin = np.isfinite(x)
    size = 1
    while size < T:
        size *= 2
    n = np.zeros((size, W))
    m = np.zeros((size, W))
    n[:T] = fin
    m[:T] = np.where(fin, x, 0.0)
    levels = [(n, m, np.zeros((size, W)))]
    while len(levels[-1][0]) > 1:
        n, m, q = levels[-1]
        levels.append(_chan(n[0::2], m[0::2], q[0::2], n[1::2], m[1::2], q[1::2]))
    lo, hi = _windows_np(T, N, M, center)
    lo, hi = lo.copy(), hi.copy()
    an, am, aq = np.zeros((T, W)), np.zeros((T, W)), np.zeros((T, W))
    for n, m, q in levels:
        if not (lo < hi).any():
            break
        sel = np.nonzero((lo < hi) & (lo & 1 == 1))[0]
        if len(sel):
            idx = lo[sel]
            lo[sel] += 1
            an[sel], am[sel], aq[sel] = _chan(an[sel], am[sel], aq[sel], n[idx], m[idx], q[idx])
        sel = np.nonzero((lo < hi) & (hi & 1 == 1))[0]
        if len(sel):
            hi[sel] -= 1
            idx = hi[sel]
            an[sel], am[sel], aq[sel] = _chan(an[sel], am[sel], aq[sel], n[idx], m[idx], q[idx])
        lo >>= 1
        hi >>= 1
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(aq / an)
    sd = np.where(sd < _EPS10, 1.0, sd)
    sd = np.where(an > 0, sd, 1.0)
    return np.where(an > 0, am, 0.0), sd


def normalize(rows, offsets, mode="meanvar", window=600, min_window=100, center=True, method="tree"):
    """float64 result of ``rows`` (frames, width) with segments ``offsets`` (n + 1 row indices); also returns the
    per-row mu and sigma' (for the bound)."""
    mode = _MODES[mode]
    seg = {"tree": _segment_tree, "direct": _segment_direct}[method]
    x = np.asarray(rows, dtype=np.float64)
    z = x.copy()
    mu_r = np.zeros_like(x)
    sd_r = np.ones_like(x)
    for a, b in zip(offsets[:-1], offsets[1:]):
        a, b = int(a), int(b)
        if b <= a:
            continue
        mu, sd = seg(x[a:b], int(window), int(min_window), bool(center))
        if mode == MEAN:
            sd = np.ones_like(sd)
        fin = np.isfinite(x[a:b])
        with np.errstate(invalid="ignore"):
            z[a:b] = np.where(fin, (x[a:b] - mu) / sd, x[a:b])
        mu_r[a:b] = mu
        sd_r[a:b] = sd
    return z, mu_r, sd_r


bound = nr.bound


def check(got, rows, offsets, mode="meanvar", window=600, min_window=100, center=True, what="", method="tree"):
    """Assert the non-finite pattern of ``got`` equals that of ``rows`` (and those values are unchanged) and
    |got - z| <= bound element by element; returns the largest |got - z| / bound."""
    got = np.asarray(got).reshape(-1, np.asarray(rows).shape[-1])
    rows = np.asarray(rows).reshape(got.shape)
    z, mu, sd = normalize(rows, offsets, mode, window, min_window, center, method)
    fin = np.isfinite(rows)
    if not np.array_equal(np.isfinite(got), fin):
        raise AssertionError("%s: the finite pattern changed at %d place(s)" % (what, int((np.isfinite(got) != fin).sum())))
    nf = ~fin
    if not np.array_equal(got[nf].view(np.uint32), np.asarray(rows, dtype=np.float32)[nf].view(np.uint32)):
        raise AssertionError("%s: a non-finite value was changed" % what)
    b = bound(rows, mu, sd)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(np.float64) - z)
        r = np.where(fin, np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf)), 0.0)
    worst = float(r.max()) if r.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError("%s: |got - ref| exceeds the bound %.3gx at %s: got %r, ref %r, bound %g"
                             % (what, worst, i, got[i], z[i], b[i]))
    return worst
