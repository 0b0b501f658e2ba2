"""Energy VAD without a GPU: the reference of tests/vad_ref.py against answers worked by hand, its set-aside rule, the
argument validator of the Python layer and the ABI's argument checks through the loaded library."""
import ctypes as C
import os

import numpy as np
import pytest

import vad_ref as vr
import mfcc_amd
from mfcc_amd import _lib as L
from mfcc_amd.api import _vad_args

INF = np.inf


def _v(e, thr, scale, ctx, p):
    return list(vr.segment(np.array(e, np.float32), thr, scale, ctx, p)[0])


# ------------------------------------------------------------------- the reference against answers worked by hand
def test_context_0_is_the_threshold_itself():
    assert _v([1, 10, 3, 8], 5.0, 0.0, 0, 0.6) == [0, 1, 0, 1]
    assert _v([5, 5.0001], 5.0, 0.0, 0, 0.6) == [0, 1]                      # strictly above


def test_context_1_and_the_shrinking_denominator():
    # above = 0 1 0 1; windows: [0,1] [0,2] [1,3] [2,3] -> num / den = 1/2 1/3 2/3 1/2
    assert _v([1, 10, 3, 8], 5.0, 0.0, 1, 0.6) == [0, 0, 1, 0]             # 1 >= 1.2, 1 >= 1.8, 2 >= 1.8, 1 >= 1.2
    assert _v([1, 10, 3, 8], 5.0, 0.0, 1, 0.5) == [1, 0, 1, 1]             # 1 >= 1.0, 1 >= 1.5, 2 >= 1.5, 1 >= 1.0


def test_context_5_wider_than_the_segment():
    # every window is the whole segment: num / den = 2 / 4
    assert _v([1, 10, 3, 8], 5.0, 0.0, 5, 0.5) == [1, 1, 1, 1]
    assert _v([1, 10, 3, 8], 5.0, 0.0, 5, 0.6) == [0, 0, 0, 0]
    # 12 rows, above only at 0: row t sees it while t <= 5; den = min(t + 5, 11) - max(t - 5, 0) + 1
    e = [9] + [0] * 11
    assert _v(e, 5.0, 0.0, 5, 0.125) == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]    # den 6 7 8 9 10 11: 1 >= den / 8


def test_mean_scale_and_a_minus_inf_frame():
    # F = {10, 2}: mean 6, theta = 0 + 1 * 6; the -inf is left out of the mean and is never above
    assert _v([-INF, 10, 2], 0.0, 1.0, 0, 0.6) == [0, 1, 0]
    assert vr.segment(np.array([-INF, 10, 2], np.float32), 0.0, 1.0, 0, 0.6)[2] == 6.0
    # ... but counts in the denominator of its neighbours: window of row 1 = 3 rows, 1 above
    assert _v([-INF, 10, 2], 0.0, 1.0, 1, 0.4) == [1, 0, 1]                # 1/2, 1/3, 1/2 against 0.4
    assert _v([np.nan, 10, 2], 0.0, 1.0, 0, 0.6) == [0, 1, 0]


def test_empty_f():
    assert _v([-INF, np.nan, -INF], 5.0, 0.5, 1, 0.6) == [0, 0, 0]
    assert _v([-INF, np.nan], -1e30, 0.0, 0, 0.6) == [0, 0]                 # scale 0: still never above


def test_scale_0_takes_no_mean():
    assert vr.segment(np.array([1e30, 7], np.float32), 6.0, 0.0, 0, 0.6)[2] == 6.0
    assert _v([1e30, 7, 5], 6.0, 0.0, 0, 0.6) == [1, 1, 0]


def test_segments_of_0_and_1_rows_and_offsets():
    rows = np.array([[0, 7.0], [0, 1.0], [0, 9.0], [0, 2.0]], np.float32)
    # segments: [], [7], [1, 9], rows 3.. outside; theta = 0 + 0.5 * mean
    v, may = vr.vad(rows, [0, 0, 1, 3], column=1, energy_threshold=0.0, energy_mean_scale=0.5)
    assert list(v) == [1, 0, 1, 0] and not may.any()
    assert _v([7], 5.0, 0.5, 0, 0.6) == [0]                                 # theta 8.5
    assert _v([7], 5.0, 0.5, 64, 0.6) == [0]
    assert _v([], 5.0, 0.5, 3, 0.6) == []


def test_set_aside_rule():
    e = np.array([4.0, 6.0, 5.0, 1.0, 9.0, 1.0, 1.0], np.float32)
    v, may, theta = vr.segment(e, 5.0, 0.0, 1, 0.6)
    assert theta == 5.0 and list(may) == [0, 1, 1, 1, 0, 0, 0]              # row 2 sits on theta: its window may differ
    got = v.copy()
    got[2] ^= 1
    rows = e[:, None]
    with pytest.raises(AssertionError, match="set aside"):                   # 3 of 7 frames is far above the cap
        vr.compare(got, rows, None, 0, energy_threshold=5.0, energy_mean_scale=0.0, frames_context=1)
    e[2] = 5.5
    v = vr.segment(e, 5.0, 0.0, 1, 0.6)[0]
    assert vr.compare(v, e[:, None], None, 0, energy_threshold=5.0, energy_mean_scale=0.0, frames_context=1)[0] == 0.0
    bad = v.copy()
    bad[4] ^= 1
    with pytest.raises(AssertionError, match="differ"):
        vr.compare(bad, e[:, None], None, 0, energy_threshold=5.0, energy_mean_scale=0.0, frames_context=1)


def test_golden_wav_sets_nothing_aside(golden_dir):
    """The figures of DESIGN.md section 4.9 for the golden file's float64 C0, rounded to fp32."""
    c0 = np.load(os.path.join(golden_dir, "f2bjrop_float64_cep32.npy"))[:, 0].astype(np.float32)
    v, may, theta = vr.segment(c0, **vr.DEFAULTS)
    assert not may.any() and 0.09 < np.abs(c0 - theta).min() < 0.11 and 0.89 < v.mean() < 0.91
    v, may, theta = vr.segment(c0, 0.0, 1.0, 5, 0.6)
    assert not may.any() and 7e-4 < np.abs(c0 - theta).min() < 8e-4 and 0.48 < v.mean() < 0.50


# ------------------------------------------------------------------- the Python validator
def test_vad_args_accepts():
    assert _vad_args() == (L.VAD_OFF, 0, 5.0, 0.5, 0, 0.6)
    assert _vad_args("select", 3, -2, 0, 64, 0.999, width=4) == (L.VAD_SELECT, 3, -2.0, 0.0, 64, 0.999)
    assert _vad_args("select", np.int64(1), np.float32(1.5), 1, np.int32(5), 0.01)[1:5] == (1, 1.5, 1.0, 5)


@pytest.mark.parametrize("kw", [dict(mode="on"), dict(mode=1), dict(column=-1), dict(column=1.0), dict(column=True),
                                dict(column=13, width=13), dict(energy_threshold=np.nan), dict(energy_threshold=INF),
                                dict(energy_threshold="5"), dict(energy_threshold=1e39), dict(energy_mean_scale=-0.1),
                                dict(energy_mean_scale=INF), dict(frames_context=-1), dict(frames_context=65),
                                dict(frames_context=1.0), dict(proportion_threshold=0.0), dict(proportion_threshold=1.0),
                                dict(proportion_threshold=np.nan), dict(proportion_threshold=1e-50)])
def test_vad_args_rejects(kw):
    with pytest.raises(ValueError):
        _vad_args(**kw)


@pytest.mark.parametrize("kw", [dict(vad="on"), dict(vad="select", vad_frames_context=65),
                                dict(vad="select", vad_proportion_threshold=1.0), dict(vad_energy_mean_scale=-1),
                                dict(vad_column=-1)])
def test_constructor_validates_the_keywords_before_the_device(kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(mfcc_amd.api, "make_params", no_device)
    with pytest.raises(ValueError):
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, **kw)


# ------------------------------------------------------------------- the ABI without a GPU
def test_symbols_and_constants():
    for name in ("mfcc_hip_set_vad", "mfcc_hip_vad_dev", "mfcc_hip_select_dev"):
        assert name in L.SYMBOLS
    assert (L.VAD_OFF, L.VAD_SELECT, L.MAX_VAD_CONTEXT) == (0, 1, 64)
    lib = mfcc_amd.load_library()
    assert lib.mfcc_hip_abi_version() == 2 and C.sizeof(L.Params) == 64


def test_null_handle_and_bad_arguments_give_invalid_param():
    lib = mfcc_amd.load_library()
    off = (C.c_size_t * 2)(0, 4)
    oo = (C.c_size_t * 2)(7, 7)
    assert lib.mfcc_hip_set_vad(None, L.VAD_SELECT, 0, 5.0, 0.5, 0, 0.6) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_vad(None, L.VAD_OFF, 0, 5.0, 0.5, 0, 0.6) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_vad_dev(None, None, 13, 0, off, 1, 5.0, 0.5, 0, 0.6, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_vad_dev(None, None, 13, 0, None, 0, 5.0, 0.5, 0, 0.6, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_select_dev(None, None, 13, None, off, 1, None, 4, oo) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_select_dev(None, None, 13, None, None, 0, None, 0, None) == L.ERROR_INVALID_PARAM
    assert list(oo) == [7, 7]


def test_header_declares_the_entry_points(golden_dir):
    src = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "mfcc_hip.h")).read()
    assert "#define MFCC_HIP_MAX_VAD_CONTEXT 64" in src and "#define MFCC_HIP_ABI_VERSION 2" in src
    assert "MFCC_HIP_VAD_OFF = 0" in src and "MFCC_HIP_VAD_SELECT = 1" in src
    for decl in ("int  mfcc_hip_set_vad(mfcc_hip_handle *h, int mode, int column, float energy_threshold,",
                 "int  mfcc_hip_vad_dev(mfcc_hip_handle *h, const void *d_rows, int row_width, int column,",
                 "int  mfcc_hip_select_dev(mfcc_hip_handle *h, const void *d_in, int row_width, const void *d_voiced,"):
        assert decl in src
    assert "1 / ln 2" in src and "SYNCHRONIZES" in src
