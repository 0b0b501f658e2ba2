"""CPU-side checks of sliding-window normalization (``MFCC(normalize_window=...)``, ``mfcc_hip_set_normalize_window``,
``mfcc_hip_normalize_sliding_dev``): the window rule against known answers, the float64 reference of
tests/normalize_sliding_ref.py against the per-segment one and its two evaluations against each other, the bound
against the fp32 model, and the argument checks of the new entry points without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mfcc_amd
import normalize_ref as nr
import normalize_sliding_ref as sr
from mfcc_amd import _lib as L

# (T, N, M, center) -> [a, b) for t = 0 .. T - 1, computed by hand from the rule in include/mfcc_hip.h
KNOWN = [
    ((10, 4, 2, True), [(0, 4), (0, 4), (0, 4), (1, 5), (2, 6), (3, 7), (4, 8), (5, 9), (6, 10), (6, 10)]),
    ((10, 5, 2, True), [(0, 5), (0, 5), (0, 5), (1, 6), (2, 7), (3, 8), (4, 9), (5, 10), (5, 10), (5, 10)]),
    ((10, 4, 6, False), [(0, 6), (0, 6), (0, 6), (0, 6), (0, 6), (1, 6), (2, 7), (3, 8), (4, 9), (5, 10)]),
    ((10, 4, 1, False), [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 6), (2, 7), (3, 8), (4, 9), (5, 10)]),
    ((3, 600, 100, True), [(0, 3)] * 3),
    ((3, 600, 100, False), [(0, 3)] * 3),
    ((7, 3, 12, False), [(0, 7)] * 7),
]


@pytest.mark.parametrize("args,want", KNOWN)
def test_window_rule_known_answers(args, want):
    T, N, M, center = args
    assert sr.windows(T, N, M, center) == want
    a, b = sr._windows_np(T, N, M, center)
    assert list(zip(a.tolist(), b.tolist())) == want


@pytest.mark.parametrize("center", [True, False])
def test_windows_hold_their_row_and_never_move_back(center):
    for T in [1, 2, 5, 99, 100, 101, 700]:
        for N, M in [(1, 1), (2, 1), (7, 3), (100, 100), (600, 100), (16384, 100)]:
            w = sr.windows(T, N, M, center)
            for t, (a, b) in enumerate(w):
                assert 0 <= a <= t < b <= T
            assert all(w[t][0] <= w[t + 1][0] and w[t][1] <= w[t + 1][1] for t in range(T - 1))
            a, b = sr._windows_np(T, N, M, center)
            assert list(zip(a.tolist(), b.tolist())) == w


def _rows(rng, T, step=False):
    x = (rng.standard_normal((T, 6)) * rng.uniform(0.1, 50, 6) + rng.uniform(-100, 100, 6)).astype(np.float32)
    x[:, 1] = 7.25                                                   # constant column
    x[:, 2] = (1e4 + 1e-2 * rng.standard_normal(T)).astype(np.float32)
    x[rng.choice(T, max(T // 20, 1), replace=False), 3] = np.nan
    x[rng.choice(T, max(T // 30, 1), replace=False), 4] = -np.inf
    if step:                                                         # 0, then 1e4 + 1e-2 noise
        x[:T // 2, 5] = 0.0
        x[T // 2:, 5] = (1e4 + 1e-2 * rng.standard_normal(T - T // 2)).astype(np.float32)
    return x


@pytest.mark.parametrize("T", [600, 601, 3000])
def test_a_centered_window_of_twice_the_segment_is_the_per_segment_form(T):
    x = _rows(np.random.default_rng(T), T)
    for mode in ("mean", "meanvar"):
        want = nr.normalize(x, [0, T], mode)
        got = sr.normalize(x, [0, T], mode, window=2 * T, min_window=100, center=True, method="direct")
        for g, w in zip(got, want):
            assert np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize("N,M,center", [(1, 1, True), (2, 1, False), (7, 3, True), (50, 20, False), (600, 100, True),
                                        (600, 100, False), (16384, 100, True)])
def test_the_tree_evaluation_equals_the_direct_one(N, M, center):
    rng = np.random.default_rng(N + center)
    lens = [0, 1, 2, 3, 64, 65, 700, 0, 1301]
    off = np.concatenate([[0], np.cumsum(lens)])
    x = _rows(rng, int(off[-1]), step=True)
    x[off[6]:off[7], 0] = np.nan                                     # a column with no finite value in one segment
    for mode in ("mean", "meanvar"):
        zd, mud, sdd = sr.normalize(x, off, mode, N, M, center, method="direct")
        zt, mut, sdt = sr.normalize(x, off, mode, N, M, center, method="tree")
        fin = np.isfinite(x)
        assert np.array_equal(np.isfinite(zt), fin) and np.array_equal(np.isfinite(zd), fin)
        assert np.array_equal(zt[~fin], zd[~fin], equal_nan=True)
        b = sr.bound(x, mud, sdd)
        # the two float64 evaluations differ by rounding only: 2^-20 of a bound that is itself 2^-22 of the values
        assert (np.abs(zt - zd)[fin] <= 2.0 ** -20 * b[fin] + 1e-300).all()
        np.testing.assert_allclose(sdt, sdd, rtol=1e-9)
    # a constant column gives exactly 0 and a one-row segment gives 0 in every finite place, in both forms
    for z in (zd, zt):
        assert np.all(z[:, 1] == 0.0)
        one = z[int(off[1])]
        assert np.all(one[np.isfinite(one)] == 0.0)


@pytest.mark.parametrize("center", [True, False])
def test_bound_accepts_fp32_rounding_and_rejects_a_wrong_value(center):
    rng = np.random.default_rng(5)
    lens = [0, 1, 2, 7, 100, 939, 1, 50]
    off = np.concatenate([[0], np.cumsum(lens)])
    x = _rows(rng, int(off[-1]), step=True)
    kw = dict(window=60, min_window=10, center=center)
    z, mu, sd = sr.normalize(x, off, "meanvar", **kw)
    # what the kernel computes: (x - fl(mu)) * fl(1 / sigma') in fp32
    y = np.where(np.isfinite(x), (x - mu.astype(np.float32)) * (1.0 / sd).astype(np.float32), x).astype(np.float32)
    assert sr.check(y, x, off, "meanvar", **kw) <= 1.0
    bad = y.copy()
    i = int(np.argwhere(np.isfinite(bad[:, 0]))[-1, 0])
    bad[i, 0] += 1e-4 * max(1.0, abs(float(bad[i, 0])))
    with pytest.raises(AssertionError):
        sr.check(bad, x, off, "meanvar", **kw)
    nan_moved = y.copy()
    nan_moved[np.argwhere(np.isnan(x[:, 3]))[0, 0], 3] = 0.0
    with pytest.raises(AssertionError):
        sr.check(nan_moved, x, off, "meanvar", **kw)


def test_new_entry_points_check_their_arguments_without_a_gpu():
    lib = mfcc_amd.load_library()
    off = (C.c_size_t * 3)(0, 4, 8)
    assert lib.mfcc_hip_set_normalize_window(None, 600, 100, 1) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_normalize_window(None, 0, 1, 1) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_normalize_sliding_dev(None, None, 13, None, off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_normalize_sliding_dev(None, None, 13, None, None, 0, 0, 600, 100, 1) == L.ERROR_INVALID_PARAM
    assert "mfcc_hip_set_normalize_window" in L.SYMBOLS and "mfcc_hip_normalize_sliding_dev" in L.SYMBOLS
    assert L.MAX_NORMALIZE_WINDOW == 16384
    assert lib.mfcc_hip_abi_version() == 2 and C.sizeof(L.Params) == 64


def test_header_declares_the_entry_points_and_the_limit():
    src = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "mfcc_hip.h")).read()
    assert "#define MFCC_HIP_MAX_NORMALIZE_WINDOW 16384" in src
    assert "int  mfcc_hip_set_normalize_window(mfcc_hip_handle *h, int window, int min_window, int center);" in src
    assert "int  mfcc_hip_normalize_sliding_dev(mfcc_hip_handle *h, const void *d_in, int row_width, void *d_out," in src
    assert "#define MFCC_HIP_ABI_VERSION 2" in src


@pytest.mark.parametrize("kw", [dict(normalize_window=0), dict(normalize_window=-5), dict(normalize_window=1.5),
                                dict(normalize_window=True), dict(normalize_window=16_385),
                                dict(normalize_window=50, normalize_min_window=60),
                                dict(normalize_window=50, normalize_min_window=0),
                                dict(normalize_window=600, normalize_center="yes")])
def test_constructor_validates_the_keywords_before_the_device(kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(mfcc_amd.api, "make_params", no_device)
    with pytest.raises(ValueError):
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, normalize="mean", **kw)


def test_window_arguments_and_the_default_minimum():
    wa = mfcc_amd.api._window_args
    assert wa(None) == (0, 1, 1)
    assert wa(600) == (600, 100, 1) and wa(600, 100, False) == (600, 100, 0)
    assert wa(50) == (50, 50, 1)                       # the default minimum is clamped to the window
    assert wa(50, 20) == (50, 20, 1) and wa(16384, 16384) == (16384, 16384, 1)
    with pytest.raises(ValueError):
        wa(50, 60)


def test_a_valid_combination_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present (tests/test_gpu_normalize_sliding.py covers the handle)")
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, normalize="meanvar", normalize_window=600, normalize_center=False)
    assert e.value.code == L.ERROR_NOT_FOUND
