"""Delta coefficients without a GPU: the float64 reference of tests/deltas_ref.py against known answers and against an
independent formulation, its bounds against the emulated fp32 sequence, and the ABI's argument checks."""
import ctypes as C

import numpy as np
import pytest

import deltas_ref as dr
import mfcc_amd
from mfcc_amd import _lib as L


# ------------------------------------------------------------------- the reference against known answers
@pytest.mark.parametrize("window", [1, 2, 3, 8])
def test_ramp_gives_its_slope_and_zero_curvature(window):
    L_ = 6 * window + 7
    t = np.arange(L_, dtype=np.float64)
    rows = np.stack([2.5 * t - 7.0, -0.25 * t + 3.0], axis=1)
    z = dr.deltas(rows, [0, L_], 2, window)
    inner = slice(window, L_ - window)
    inner2 = slice(2 * window, L_ - 2 * window)
    np.testing.assert_allclose(z[inner, 2], 2.5, rtol=1e-13)
    np.testing.assert_allclose(z[inner, 3], -0.25, rtol=1e-13)
    np.testing.assert_allclose(z[inner2, 4:], 0.0, atol=1e-12)
    assert np.array_equal(z[:, :2], rows)


def test_constant_segment_gives_zeros():
    rows = np.full((17, 3), -4.25)
    z = dr.deltas(rows, [0, 5, 17], 2, 3)
    assert np.array_equal(z[:, 3:], np.zeros((17, 6)))


def test_short_segments_worked_by_hand():
    # 1 row: D = DD = 0
    z = dr.deltas(np.array([[3.0]]), [0, 1], 2, 2)
    assert np.array_equal(z, [[3.0, 0.0, 0.0]])
    # 2 rows, N = 2 (r = 1/10): both D = r (1 (s1 - s0) + 2 (s1 - s0)) = 0.3 (s1 - s0); DD of a constant D = 0
    z = dr.deltas(np.array([[1.0], [6.0]]), [0, 2], 2, 2)
    np.testing.assert_allclose(z[:, 1], [1.5, 1.5], rtol=1e-15)
    assert np.array_equal(z[:, 2], [0.0, 0.0])
    # 2N + 1 = 3 rows, N = 1 (r = 1/2): s = 1, 4, 9
    z = dr.deltas(np.array([[1.0], [4.0], [9.0]]), [0, 3], 2, 1)
    np.testing.assert_allclose(z[:, 1], [1.5, 4.0, 2.5], rtol=1e-15)
    np.testing.assert_allclose(z[:, 2], [1.25, 0.5, -0.75], rtol=1e-15)
    # 2N + 1 = 5 rows, N = 2 (r = 1/10): s = t^2
    z = dr.deltas(np.array([[0.0], [1.0], [4.0], [9.0], [16.0]]), [0, 5], 2, 2)
    np.testing.assert_allclose(z[:, 1], [0.9, 2.2, 4.0, 4.2, 3.1], rtol=1e-14)
    np.testing.assert_allclose(z[:, 2], [0.75, 0.97, 0.64, 0.09, -0.29], rtol=1e-13)


def _independent(rows, offsets, order, window):
    """np.pad(mode="edge") and a correlation per segment and column, applied twice for DD."""
    x = np.asarray(rows, dtype=np.float64)
    taps = np.arange(-window, window + 1, dtype=np.float64) / (2.0 * sum(n * n for n in range(1, window + 1)))

    def stage(v):
        out = np.zeros_like(v)
        for a, b in zip(offsets[:-1], offsets[1:]):
            if b <= a:
                continue
            for j in range(v.shape[1]):
                p = np.pad(v[a:b, j], window, mode="edge")
                out[a:b, j] = np.correlate(p, taps, mode="valid")
        return out

    d = stage(x)
    return np.concatenate([x, d] + ([stage(d)] if order == 2 else []), axis=1)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("window", [1, 2, 3, 8])
def test_reference_equals_an_independent_formulation(order, window):
    rng = np.random.default_rng(window * 10 + order)
    lens = [0, 1, 2, 3, 2 * window, 2 * window + 1, 4 * window + 3, 50, 0, 7]
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = rng.standard_normal((int(off[-1]), 5)) * 10
    np.testing.assert_allclose(dr.deltas(rows, off, order, window), _independent(rows, off, order, window),
                               rtol=1e-12, atol=1e-12)


def test_finite_pattern_follows_the_clamped_neighbours():
    rows = np.zeros((12, 1))
    rows[0, 0] = -np.inf                         # first row of a segment: every clamp below it reads it
    rows[8, 0] = np.nan
    pat = dr.finite_pattern(rows, [0, 6, 12], 2, 1)
    # D (N = 1): row t reads rows c(t - 1), c(t + 1)
    assert list(~pat[:6, 1]) == [True, True, False, False, False, False]
    assert list(~pat[6:, 1]) == [False, True, False, True, False, False]
    # DD reads D the same way
    assert list(~pat[:6, 2]) == [True, True, True, False, False, False]
    assert list(~pat[6:, 2]) == [True, False, True, False, True, False]


# ------------------------------------------------------------------- the stage bound
@pytest.mark.parametrize("window", [1, 2, 3, 4, 8])
def test_stage_bound_accepts_the_fp32_sequence_and_rejects_a_moved_value(window):
    rng = np.random.default_rng(100 + window)
    for trial in range(40):
        lens = [int(v) for v in rng.integers(0, 60, 6)] + [1, 2]
        off = np.concatenate([[0], np.cumsum(lens)])
        R = int(off[-1])
        rows = (rng.standard_normal((R, 4)) * rng.uniform(0.1, 100, 4)).astype(np.float32)
        rows[:, 3] = (1e4 + 1e-2 * rng.standard_normal(R)).astype(np.float32)
        for order in (1, 2):
            got = dr.emulate32(rows, off, order, window)
            assert dr.check_stage(got, rows, off, order, window, "trial %d" % trial) <= 1.0
    # a D value moved by 1e-4 relative is refused
    rows = (rng.standard_normal((40, 3)) * 5).astype(np.float32)
    got = dr.emulate32(rows, [0, 40], 2, window)
    i = int(np.argmax(np.abs(got[:, 3])))
    bad = got.copy()
    bad[i, 3] = np.float32(bad[i, 3] * (1 + 1e-4))
    with pytest.raises(AssertionError):
        dr.check_stage(bad, rows, [0, 40], 2, window)
    bad = got.copy()
    j = int(np.argmax(np.abs(got[:, 6])))
    bad[j, 6] = np.float32(bad[j, 6] * (1 + 1e-4))
    with pytest.raises(AssertionError):
        dr.check_stage(bad, rows, [0, 40], 2, window)


def test_end_to_end_bound_is_finite_and_covers_a_perturbation_within_B():
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((300, 13)) * 20
    B = np.abs(ref) * 1e-5 + 1e-6
    off = [0, 120, 300]
    got = dr.deltas(ref + 0.9 * B * rng.uniform(-1, 1, ref.shape), off, 2, 2).astype(np.float32)   # room for fp32
    assert dr.check_end_to_end(got, ref, B, off, 2, 2) <= 1.0
    with pytest.raises(AssertionError):
        dr.check_end_to_end(got, ref, np.where(np.arange(300)[:, None] == 7, np.inf, B), off, 2, 2)


# ------------------------------------------------------------------- the ABI without a GPU
def test_null_handle_and_symbols():
    lib = mfcc_amd.load_library()
    off = (C.c_size_t * 2)(0, 4)
    assert lib.mfcc_hip_set_deltas(None, 2, 2) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_deltas(None, 0, 2) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_deltas_dev(None, None, 13, None, off, 1, 2, 2) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_deltas_dev(None, None, 13, None, None, 0, 2, 2) == L.ERROR_INVALID_PARAM
    assert "mfcc_hip_set_deltas" in L.SYMBOLS and "mfcc_hip_deltas_dev" in L.SYMBOLS
    assert L.MAX_DELTA_WINDOW == 8
    assert lib.mfcc_hip_abi_version() == 2 and C.sizeof(L.Params) == 64


def test_header_declares_the_window_limit():
    import os
    src = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "mfcc_hip.h")).read()
    assert "#define MFCC_HIP_MAX_DELTA_WINDOW 8" in src
    assert "int  mfcc_hip_set_deltas(mfcc_hip_handle *h, int order, int window);" in src


@pytest.mark.parametrize("kw", [dict(deltas=3), dict(delta_window=0), dict(delta_window=9), dict(deltas=-1),
                                dict(deltas=1.0), dict(delta_window="2")])
def test_constructor_validates_the_keywords_before_the_device(kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(mfcc_amd.api, "make_params", no_device)
    with pytest.raises(ValueError):
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, **kw)
