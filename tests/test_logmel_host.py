"""CPU-side checks of the log-mel output mode (``output="logmel"``): the parameter block carries it, the library
validates it, the ABI stays what it was, and the Python layer sizes rows by it."""
import ctypes as C

import pytest

import mfcc_amd
from mfcc_amd import _lib as L


def _num_frames(p, n=5000):
    out = C.c_size_t(0)
    rc = L.load().mfcc_hip_num_frames(C.byref(p), n, C.byref(out))
    return rc, out.value


def test_logmel_params_are_accepted():
    for kw in [dict(), dict(nfft=1024, nfilters=40), dict(nfft=256, nfilters=64, nceptrums=13),
               dict(nfilters=16, nceptrums=16, samplerate=48000)]:
        p = mfcc_amd.make_params(output="logmel", **kw)
        assert p.output == L.OUTPUT_LOGMEL and list(p.reserved) == [0, 0, 0, 0]
        rc, nf = _num_frames(p)
        assert rc == L.SUCCESS, kw
        assert nf == mfcc_amd.num_frames(5000, **kw)
    assert mfcc_amd.make_params().output == L.OUTPUT_CEPSTRA
    assert mfcc_amd.make_params(output="cepstra").output == L.OUTPUT_CEPSTRA


def test_logmel_invalid_combinations_are_rejected():
    for kw in [dict(output=2), dict(output=-1), dict(output="logmel", lifter=22),
               dict(output="logmel", nceptrums=0), dict(output="logmel", nceptrums=33)]:
        rc, _ = _num_frames(mfcc_amd.make_params(**kw))
        assert rc == L.ERROR_INVALID_PARAM, kw
    # the lifter stays legal for cepstra
    assert _num_frames(mfcc_amd.make_params(lifter=22))[0] == L.SUCCESS
    with pytest.raises(KeyError):
        mfcc_amd.make_params(output="mel")


def test_params_struct_and_symbol_set_unchanged():
    assert C.sizeof(L.Params) == 64
    assert L.Params.output.offset == 44 and L.Params.reserved.offset == 48
    p = L.Params()
    assert L.load().mfcc_hip_default_params(C.byref(p)) == 0
    assert p.struct_size == 64 and p.output == 0
    # a non-zero reserved word is still refused
    p = mfcc_amd.make_params(output="logmel")
    p.reserved[3] = 1
    assert _num_frames(p)[0] == L.ERROR_INVALID_PARAM
    assert "mfcc_hip_output" not in L.SYMBOLS and len([s for s in L.SYMBOLS if "logmel" in s]) == 0


def test_logmel_tables_build_without_a_gpu():
    # the host-side table builders take the same parameter block
    w = mfcc_amd.get_table(L.TABLE_MEL_DENSE_F32, output="logmel")
    assert w.size == 32 * 257


def test_num_features_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present (tests/test_gpu_logmel.py covers the handle)")
    # the handle cannot be created here: the parameters pass validation and the library stops at the device
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, output="logmel")
    assert e.value.code == L.ERROR_NOT_FOUND
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, output="logmel", lifter=22)
    assert e.value.code == L.ERROR_INVALID_PARAM
    # what the constructor sets before it asks for the device
    m = mfcc_amd.MFCC.__new__(mfcc_amd.MFCC)
    m.nfilters, m.nceptrums, m.output = 40, 13, "logmel"
    assert m.num_features == 40
    m.output = "cepstra"
    assert m.num_features == 13
