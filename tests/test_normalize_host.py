"""CPU-side checks of per-segment normalization (``MFCC(normalize=...)``, ``mfcc_hip_set_normalize``,
``mfcc_hip_normalize_dev``): the float64 reference of tests/normalize_ref.py is ``sklearn.preprocessing.scale`` per
segment, the new entry points check their arguments without a GPU, and the Python mode names map to the enum."""
import ctypes as C

import numpy as np
import pytest

import mfcc_amd
import normalize_ref as nr
from mfcc_amd import _lib as L


def _segments(rng):
    """Random rows (frames, 13) in segments of 0, 1, 2, 7, 100 and 939 rows, with NaN, -inf, constant columns and a
    column of 1e4 + 1e-2 noise."""
    lens = [0, 1, 2, 7, 100, 939, 1, 50]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = (rng.standard_normal((int(off[-1]), 13)) * rng.uniform(0.1, 50, 13) + rng.uniform(-100, 100, 13)).astype(np.float32)
    x[:, 3] = 7.25                                                   # constant column
    x[:, 5] = (1e4 + 1e-2 * rng.standard_normal(len(x))).astype(np.float32)
    nan_rows = rng.choice(len(x), 40, replace=False)
    x[nan_rows, 7] = np.nan
    x[rng.choice(len(x), 20, replace=False), 9] = -np.inf
    x[off[4]:off[5], 11] = np.nan                                    # a column with no finite value in one segment
    return x, off


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_is_sklearn_scale_per_segment(seed):
    skp = pytest.importorskip("sklearn.preprocessing")
    x, off = _segments(np.random.default_rng(seed))
    z, _, _ = nr.normalize(x, off, "meanvar")
    zm, _, _ = nr.normalize(x, off, "mean")
    for a, b in zip(off[:-1], off[1:]):
        if b <= a:
            continue
        seg = x[a:b].astype(np.float64)
        seg = np.where(np.isinf(seg), np.nan, seg)                  # sklearn accepts NaN, not inf: both are left out
        with np.errstate(invalid="ignore", divide="ignore"), _quiet():
            ref = skp.scale(seg, axis=0)
            refm = skp.scale(seg, axis=0, with_std=False)
        fin = np.isfinite(x[a:b])
        assert np.array_equal(np.isfinite(z[a:b]), fin)
        np.testing.assert_allclose(z[a:b][fin], ref[fin], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(zm[a:b][fin], refm[fin], rtol=1e-9, atol=1e-7)
        # the non-finite values themselves are kept
        assert np.array_equal(z[a:b][~fin].astype(np.float32).view(np.uint32), x[a:b][~fin].view(np.uint32))
    # a constant column gives exactly 0, a one-row segment gives 0 in every finite place
    assert np.all(z[:, 3] == 0.0)
    one = int(off[1])
    assert np.all(z[one][np.isfinite(z[one])] == 0.0)


class _quiet:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *a):
        return self._w.__exit__(*a)


def test_bound_accepts_fp32_rounding_and_rejects_a_wrong_value():
    rng = np.random.default_rng(5)
    x, off = _segments(rng)
    z, mu, sd = nr.normalize(x, off)
    # what the kernel computes: (x - fl(mu)) * fl(1 / sigma') in fp32
    y = np.where(np.isfinite(x), (x - mu.astype(np.float32)) * (1.0 / sd).astype(np.float32), x).astype(np.float32)
    assert nr.check(y, x, off) <= 1.0
    bad = y.copy()
    i = int(np.argwhere(np.isfinite(bad[:, 0]))[-1, 0])
    bad[i, 0] += 1e-4 * max(1.0, abs(float(bad[i, 0])))
    with pytest.raises(AssertionError):
        nr.check(bad, x, off)
    nan_moved = y.copy()
    nan_moved[np.argwhere(np.isnan(x[:, 7]))[0, 0], 7] = 0.0
    with pytest.raises(AssertionError):
        nr.check(nan_moved, x, off)


def test_new_entry_points_check_their_arguments_without_a_gpu():
    lib = mfcc_amd.load_library()
    off = (C.c_size_t * 3)(0, 4, 8)
    assert lib.mfcc_hip_set_normalize(None, 0) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_normalize(None, 2) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_normalize_dev(None, None, 13, off, 2, 2) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_normalize_dev(None, None, 13, None, 0, 0) == L.ERROR_INVALID_PARAM
    assert (L.NORMALIZE_NONE, L.NORMALIZE_MEAN, L.NORMALIZE_MEAN_VAR) == (0, 1, 2)
    assert lib.mfcc_hip_abi_version() == 2 and C.sizeof(L.Params) == 64
    assert "mfcc_hip_set_normalize" in L.SYMBOLS and "mfcc_hip_normalize_dev" in L.SYMBOLS
    assert not [s for s in L.SYMBOLS if "logmel" in s]


def test_header_declares_the_enum():
    import os
    src = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "mfcc_hip.h")).read()
    for name, v in [("MFCC_HIP_NORMALIZE_NONE", 0), ("MFCC_HIP_NORMALIZE_MEAN", 1), ("MFCC_HIP_NORMALIZE_MEAN_VAR", 2)]:
        assert "%s = %d" % (name, v) in src
    assert "#define MFCC_HIP_ABI_VERSION 2" in src


def test_python_mode_names():
    assert mfcc_amd.normalize_mode(None) == L.NORMALIZE_NONE
    assert mfcc_amd.normalize_mode("none") == L.NORMALIZE_NONE
    assert mfcc_amd.normalize_mode("mean") == L.NORMALIZE_MEAN
    assert mfcc_amd.normalize_mode("meanvar") == L.NORMALIZE_MEAN_VAR
    for bad in ["var", "MEANVAR", 2, [], "cmvn"]:
        with pytest.raises(ValueError):
            mfcc_amd.normalize_mode(bad)


def test_constructor_validates_the_keyword_before_the_device():
    import torch
    with pytest.raises(ValueError):
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, normalize="zscore")
    if torch.cuda.is_available():
        pytest.skip("GPU present (tests/test_gpu_normalize.py covers the handle)")
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, normalize="meanvar")
    assert e.value.code == L.ERROR_NOT_FOUND
