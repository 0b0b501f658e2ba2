"""Centred framing on the CPU (include/mfcc_hip.h "centring"): the geometry against its closed form
and against ``torch.stft``'s frame count, ``mfcc_hip_center_host`` against the ``np.pad`` restatement of
tests/center_ref.py, the refusals, the exports, and the float64 chain on the padded signal against ``torch.stft`` power:
the frames of a centred handle are the frames of ``torch.stft(center=True)``, not frames like them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mfcc_amd
from mfcc_amd import _lib as L
import center_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, SMALL = L.SUCCESS, L.ERROR_INVALID_PARAM, L.ERROR_BUFFER_SMALL
MODE = {"reflect": L.CENTER_REFLECT, "zeros": L.CENTER_ZEROS}
NEW = ["mfcc_hip_center_geometry", "mfcc_hip_center_host", "mfcc_hip_center_dev", "mfcc_hip_set_center", "mfcc_hip_center"]
IDS = ["%d_%d_%d" % f for f in cr.FRAMINGS]


def _geometry(nfft, hop, flen, mode, n):
    p = mfcc_amd.make_params(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    f, left, padded = C.c_size_t(9), C.c_size_t(9), C.c_size_t(9)
    rc = L.load().mfcc_hip_center_geometry(C.byref(p), flen, MODE[mode], n, C.byref(f), C.byref(left), C.byref(padded))
    return rc, f.value, left.value, padded.value


def _signal(n, seed=5):
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


def test_every_new_declaration_is_declared_exported_and_typed():
    src = open(os.path.join(ROOT, "include", "mfcc_hip.h")).read()
    assert re.search(r"enum mfcc_hip_center \{ MFCC_HIP_CENTER_OFF = 0, MFCC_HIP_CENTER_REFLECT = 1, MFCC_HIP_CENTER_ZEROS = 2 \}", src)
    assert re.search(r"#define\s+MFCC_HIP_ABI_VERSION\s+2\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfcc_hip_[a-z0-9_]+)\s*\(", code))
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
    assert (L.CENTER_OFF, L.CENTER_REFLECT, L.CENTER_ZEROS) == (0, 1, 2)
    assert L.load().mfcc_hip_abi_version() == 2 == L.ABI_VERSION
    assert C.sizeof(L.Params) == 64
    assert L.load().mfcc_hip_center(None) == L.CENTER_OFF
    assert L.load().mfcc_hip_set_center(None, L.CENTER_REFLECT) == INVALID


@pytest.mark.parametrize("nfft,hop,flen", cr.FRAMINGS, ids=IDS)
def test_geometry_is_the_closed_form_and_torch_stft_s_frame_count(nfft, hop, flen):
    import torch
    pl = cr.left_pad(nfft, flen)
    assert pl == (flen + 1) // 2
    window = np.ones(flen)
    for n in cr.lengths(nfft, hop, flen):
        for mode in cr.MODES:
            rc, f, left, padded = _geometry(nfft, hop, flen, mode, n)
            assert rc == OK and left == pl
            assert f == 1 + n // hop == cr.frames(n, nfft, hop, flen, mode), (n, mode)
            assert padded == (f - 1) * hop + flen
            assert mfcc_amd.num_frames(n, nfft=nfft, hop=hop, win_length=flen, center=mode) == f
            # the handle's own framing of the padded signal gives exactly these frames
            assert mfcc_amd.num_frames(padded, nfft=nfft, hop=hop, win_length=flen) == f
        if cr.torch_accepts(n, nfft):
            assert cr.stft_power(np.zeros(n), nfft, hop, flen, window).shape == (1 + n // hop, nfft // 2 + 1)
    # the thresholds: no frame where the signal cannot be reflected / where there is none
    for n in (0, 1, pl):
        assert _geometry(nfft, hop, flen, "reflect", n)[1:] == (0, pl, 0)
        assert mfcc_amd.num_frames(n, nfft=nfft, hop=hop, win_length=flen, center=True) == 0
    assert _geometry(nfft, hop, flen, "zeros", 0)[1:] == (0, pl, 0)
    assert _geometry(nfft, hop, flen, "zeros", 1)[1:] == (1, pl, flen)
    assert torch.__version__                                   # the reference is this torch's


def test_geometry_refusals():
    p = mfcc_amd.make_params(nfft=512, hop=160)
    lib = L.load()
    f = C.c_size_t(0)
    assert lib.mfcc_hip_center_geometry(None, 400, L.CENTER_REFLECT, 10, C.byref(f), None, None) == INVALID
    for mode in (L.CENTER_OFF, 3, -1):
        assert lib.mfcc_hip_center_geometry(C.byref(p), 400, mode, 10, C.byref(f), None, None) == INVALID
    assert lib.mfcc_hip_center_geometry(C.byref(p), 100, L.CENTER_REFLECT, 10, C.byref(f), None, None) == INVALID   # below the hop
    assert lib.mfcc_hip_center_geometry(C.byref(p), 0, L.CENTER_REFLECT, 1000, None, None, None) == OK
    assert lib.mfcc_hip_center_geometry(C.byref(p), 0, L.CENTER_REFLECT, 1000, C.byref(f), None, None) == OK and f.value == 7
    with pytest.raises(ValueError):
        mfcc_amd.num_frames(100, center="edge")
    with pytest.raises(ValueError):
        mfcc_amd.center_pad(np.zeros(10, np.int16), mode=None)


@pytest.mark.parametrize("mode", cr.MODES)
@pytest.mark.parametrize("nfft,hop,flen", cr.FRAMINGS, ids=IDS)
def test_center_host_is_the_np_pad_restatement(nfft, hop, flen, mode):
    for n in cr.lengths(nfft, hop, flen):
        x = _signal(n, seed=n)
        got = mfcc_amd.center_pad(x, mode, nfft=nfft, hop=hop, win_length=flen)
        want = cr.pad(x, nfft, hop, flen, mode)
        assert got.dtype == np.int16 and got.shape == want.shape == (cr.padded_len(n, nfft, hop, flen, mode),)
        assert np.array_equal(got, want), (n, mode)


def test_center_host_short_signals_small_buffers_and_null_pointers():
    lib = L.load()
    p = mfcc_amd.make_params(nfft=512, hop=160)
    pl = cr.left_pad(512, 400)
    x = _signal(1000)
    out = np.full(2000, -7, np.int16)
    n_out = C.c_size_t(99)
    for n in (0, 1, pl):                                       # reflect: nothing to reflect, no frame
        assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_REFLECT, L.ptr(x), n, L.ptr(out), 0, C.byref(n_out)) == OK
        assert n_out.value == 0 and (out == -7).all()
        assert mfcc_amd.center_pad(x[:n], "reflect", nfft=512, hop=160, win_length=400).size == 0
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_ZEROS, None, 0, None, 0, C.byref(n_out)) == OK and n_out.value == 0
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_ZEROS, L.ptr(x), 1, L.ptr(out), 400, C.byref(n_out)) == OK
    assert n_out.value == 400 and out[pl] == x[0] and not out[:pl].any() and not out[pl + 1:400].any()
    out[:] = -7
    want = cr.padded_len(1000, 512, 160, 400)
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_REFLECT, L.ptr(x), 1000, L.ptr(out), want - 1, C.byref(n_out)) == SMALL
    assert n_out.value == want and (out == -7).all()
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_REFLECT, None, 1000, L.ptr(out), 2000, C.byref(n_out)) == INVALID
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_REFLECT, L.ptr(x), 1000, None, 2000, C.byref(n_out)) == INVALID
    assert lib.mfcc_hip_center_host(None, 400, L.CENTER_REFLECT, L.ptr(x), 1000, L.ptr(out), 2000, None) == INVALID
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_OFF, L.ptr(x), 1000, L.ptr(out), 2000, None) == INVALID
    assert (out == -7).all()
    assert lib.mfcc_hip_center_host(C.byref(p), 400, L.CENTER_REFLECT, L.ptr(x), 1000, L.ptr(out), 2000, None) == OK
    assert np.array_equal(out[:want], cr.pad(x, 512, 160, 400)) and (out[want:] == -7).all()


@pytest.mark.parametrize("nfft,hop,flen", cr.FRAMINGS, ids=IDS)
def test_chain_on_the_padded_signal_is_torch_stft_power(nfft, hop, flen):
    """Equal shapes, and every element within 1e-12 of its frame's largest bin (measured: 6.3e-16 at worst; an offset
    wrong by one sample gives more than 1e-3)."""
    window = mfcc_amd.window("hann", flen).astype(np.float64)
    worst = 0.0
    for n in cr.lengths(nfft, hop, flen):
        if not cr.torch_accepts(n, nfft):
            continue
        x = _signal(n, seed=100 + n)
        p = mfcc_amd.center_pad(x, "reflect", nfft=nfft, hop=hop, win_length=flen)
        got = cr.chain_power(p, nfft, hop, flen, window)
        ref = cr.stft_power(x, nfft, hop, flen, window)
        assert got.shape == ref.shape == (1 + n // hop, nfft // 2 + 1)
        top = ref.max(axis=1, keepdims=True)
        assert (top > 0).all()
        err = float((np.abs(got - ref) / top).max())
        worst = max(worst, err)
        assert err <= 1e-12, (n, err)
        # not blind: the same chain one sample off is far outside
        off = cr.chain_power(np.concatenate([p[1:], p[:1]]), nfft, hop, flen, window)
        assert float((np.abs(off - ref) / top).max()) > 1e-3
    print("worst |chain - torch.stft| / max bin at %d/%d/%d: %.3g" % (nfft, hop, flen, worst))


def test_python_keyword_values():
    assert [mfcc_amd.api.center_mode(v) for v in (None, False, "off", True, "reflect", "zeros")] == [0, 0, 0, 1, 1, 2]
    for bad in (1, 0, "edge", 2.0):
        with pytest.raises(ValueError):
            mfcc_amd.api.center_mode(bad)
