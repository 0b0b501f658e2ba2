"""float64 NumPy reference of per-segment normalization (include/mfcc_hip.h: enum mfcc_hip_normalize) and the
per-element bound the GPU result is held to -- TEST INFRASTRUCTURE ONLY.

Per segment and column j, over the finite values F of the column: mu = mean(F), sigma = sqrt(mean((F - mu)^2))
(ddof 0, as ``sklearn.preprocessing.scale`` / ``np.std``), sigma' = 1 where sigma < 10 * 2^-52 (sklearn's
``_handle_zeros_in_scale``).  MEAN: y = x - mu; MEAN_VAR: y = (x - mu) / sigma'.  Non-finite x stay as they are.

Bound, for y computed as (x - mu32) * r32 with mu32 = fl(mu), r32 = fl(1 / sigma'): fl(mu) moves y by
2^-24 |mu| / sigma', the subtraction, fl(1 / sigma') and the product by 2^-24 |x - mu| / sigma' each (first order),
and the float64 statistics by far less.  2^-22 (|mu| + |x - mu|) / sigma' covers that with room to spare.
"""
from __future__ import annotations

import numpy as np

MEAN, MEAN_VAR = 1, 2
_MODES = {"mean": MEAN, "meanvar": MEAN_VAR, MEAN: MEAN, MEAN_VAR: MEAN_VAR}


def stats(seg):
    """(mu, sigma') per column of ``seg`` (rows, width) in float64; NaN mu for a column with no finite value."""
    x = np.asarray(seg, dtype=np.float64)
    fin = np.isfinite(x)
    n = fin.sum(axis=0)
    xs = np.where(fin, x, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = xs.sum(axis=0) / n
        d = np.where(fin, x - mu, 0.0)
        sd = np.sqrt((d * d).sum(axis=0) / n)
    sd = np.where(sd < 10 * np.finfo(np.float64).eps, 1.0, sd)
    sd = np.where(n > 0, sd, 1.0)
    return mu, sd


def normalize(rows, offsets, mode="meanvar"):
    """float64 result of ``rows`` (frames, width) with segments ``offsets`` (n + 1 row indices); also returns the
    per-row mu and sigma' (for the bound)."""
    mode = _MODES[mode]
    x = np.asarray(rows, dtype=np.float64)
    z = x.copy()
    mu_r = np.zeros_like(x)
    sd_r = np.ones_like(x)
    for a, b in zip(offsets[:-1], offsets[1:]):
        a, b = int(a), int(b)
        if b <= a:
            continue
        mu, sd = stats(x[a:b])
        if mode == MEAN:
            sd = np.ones_like(sd)
        mu_f = np.where(np.isfinite(mu), mu, 0.0)
        fin = np.isfinite(x[a:b])
        z[a:b] = np.where(fin, (x[a:b] - mu_f) / sd, x[a:b])
        mu_r[a:b] = mu_f
        sd_r[a:b] = sd
    return z, mu_r, sd_r


def bound(x, mu, sd):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return 2.0 ** -22 * (np.abs(mu) + np.abs(x - mu)) / sd


def check(got, rows, offsets, mode="meanvar", what=""):
    """Assert the non-finite pattern of ``got`` equals that of ``rows`` (and those values are unchanged) and
    |got - z| <= bound element by element; returns the largest |got - z| / bound."""
    got = np.asarray(got).reshape(-1, np.asarray(rows).shape[-1])
    rows = np.asarray(rows).reshape(got.shape)
    z, mu, sd = normalize(rows, offsets, mode)
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
