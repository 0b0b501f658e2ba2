"""Host side of the mel bank as a property of a handle (mfcc_hip_create_banked, mfcc_hip_get_table_banked,
mfcc_hip_mel_bank_of): the ABI, the NULL / NOTEBOOK bank against the framed tables byte for byte, the HTK matrix against
the float64 reference of tests/melbank_ref.py, its refusals, the tables an HTK bank does not have, the Python argument
checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import melbank_ref as mr
import mfcc_amd
from mfcc_amd import _lib as L

NEW = ["mfcc_hip_create_banked", "mfcc_hip_get_table_banked", "mfcc_hip_mel_bank_of"]
TABLES = [L.TABLE_WINDOW_F32, L.TABLE_MEL_POINTS_I32, L.TABLE_MEL_DENSE_F32, L.TABLE_DCT_F32, L.TABLE_FX_CURVE_I32,
          L.TABLE_FX_TWIDDLE_I32, L.TABLE_FX_MEL_DENSE_U32]
# (n_mel, low, high, sample rate); high 0: sample_rate / 2
BANKS = [(23, 20, 0, 16000), (40, 20, 0, 16000), (64, 125, 7500, 16000), (64, 0, 0, 16000), (40, 0, 0, 8000),
         (23, 20, 0, 48000)]


def _bank(kind=L.MEL_HTK, low=0.0, high=0.0, size=None, reserved=None):
    b = L.MelBank()
    b.struct_size = C.sizeof(L.MelBank) if size is None else size
    b.kind, b.low_hz, b.high_hz = kind, low, high
    if reserved is not None:
        b.reserved[reserved] = 1
    return b


def _table(p, flen, bank, which):
    """(return code, bytes) of mfcc_hip_get_table_banked; bank None: NULL"""
    lib = L.load()
    n = C.c_size_t(0)
    ref = C.byref(bank) if bank is not None else None
    rc = lib.mfcc_hip_get_table_banked(C.byref(p), flen, ref, which, None, 0, C.byref(n))
    if rc:
        return rc, b""
    buf = np.empty(n.value, np.uint8)
    rc = lib.mfcc_hip_get_table_banked(C.byref(p), flen, ref, which, buf.ctypes.data, buf.nbytes, C.byref(n))
    return rc, buf.tobytes()


def _framed(p, flen, which):
    lib = L.load()
    n = C.c_size_t(0)
    rc = lib.mfcc_hip_get_table_framed(C.byref(p), flen, which, None, 0, C.byref(n))
    if rc:
        return rc, b""
    buf = np.empty(n.value, np.uint8)
    rc = lib.mfcc_hip_get_table_framed(C.byref(p), flen, which, buf.ctypes.data, buf.nbytes, C.byref(n))
    return rc, buf.tobytes()


def test_new_exports_exist_and_the_abi_is_unchanged():
    lib = L.load()
    for name in NEW:
        assert name in L.SYMBOLS and getattr(lib, name) is not None, name
    assert lib.mfcc_hip_abi_version() == 2 == L.ABI_VERSION
    assert C.sizeof(L.Params) == 64 and C.sizeof(L.MelBank) == 32
    assert lib.mfcc_hip_mel_bank_of(None, C.byref(L.MelBank())) == L.ERROR_INVALID_PARAM


@pytest.mark.parametrize("kw,flen", [(dict(nfft=512, hop=160, nfilters=32, nceptrums=13), 400),
                                     (dict(nfft=512, nfilters=32, nceptrums=13), 0),
                                     (dict(nfft=1024, hop=320, nfilters=40, nceptrums=13, samplerate=48000), 800),
                                     (dict(nfft=512, hop=160, nfilters=20, nceptrums=13), 400)])
def test_null_and_notebook_banks_are_the_framed_tables_byte_for_byte(kw, flen):
    p = mfcc_amd.make_params(**kw)
    for which in TABLES:
        want = _framed(p, flen, which)
        assert _table(p, flen, None, which) == want, which
        assert _table(p, flen, _bank(L.MEL_NOTEBOOK), which) == want, which
    # ... and through Python: the defaults are the notebook bank
    py = dict(kw, win_length=flen or None)
    for which in (L.TABLE_WINDOW_F32, L.TABLE_MEL_POINTS_I32, L.TABLE_MEL_DENSE_F32, L.TABLE_DCT_F32):
        assert mfcc_amd.get_table(which, mel="notebook", **py).tobytes() == _framed(p, flen, which)[1]


@pytest.mark.parametrize("n_mel,low,high,rate", BANKS)
def test_htk_dense_table_is_the_reference_rounded_to_fp32(n_mel, low, high, rate):
    kw = dict(nfft=512, hop=160, nfilters=n_mel, nceptrums=13, samplerate=rate)
    got = mfcc_amd.get_table(L.TABLE_MEL_DENSE_F32, win_length=400, mel="htk", fmin=low, fmax=high or None, **kw)
    assert got.dtype == np.float32 and got.shape == (n_mel * 257,)
    got = got.reshape(n_mel, 257)
    ref = mr.htk_matrix(512, n_mel, rate, low, high).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the same matrix from C with high_hz spelled out, and for a plain (unframed) handle
    p = mfcc_amd.make_params(**kw)
    for flen, hi in ((400, float(high)), (0, float(high or rate / 2))):
        rc, raw = _table(p, flen, _bank(L.MEL_HTK, float(low), hi), L.TABLE_MEL_DENSE_F32)
        assert rc == L.SUCCESS and raw == ref.tobytes()
    # no empty filter, no weight on the DC bin, triangles: one peak per row, weights in [0, 1]
    assert (got != 0).any(axis=1).all()
    assert not got[:, 0].any()
    assert got.min() >= 0.0 and got.max() <= 1.0
    for row in got:
        nz = np.flatnonzero(row)
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))
        k = int(row.argmax())
        assert (np.diff(row[nz[0]:k + 1]) > 0).all() and (np.diff(row[k:nz[-1] + 1]) < 0).all()
    # the other float tables do not depend on the bank
    for which in (L.TABLE_WINDOW_F32, L.TABLE_DCT_F32):
        assert _table(p, 400, _bank(L.MEL_HTK, float(low), float(high)), which) == _framed(p, 400, which)


def test_the_reference_matrix_has_the_band_limits():
    """melbank_ref itself: the first filter starts at ``low``, the last ends at ``high``, the peaks are equally spaced
    on the mel axis."""
    w = mr.htk_matrix(512, 64, 16000, 125.0, 7500.0)
    hz = np.arange(257) * 16000.0 / 512
    support = hz[(w != 0).any(axis=0)]
    assert support.min() > 125.0 and support.min() - 31.25 <= 125.0
    assert support.max() < 7500.0 and support.max() + 31.25 >= 7500.0
    assert np.array_equal(mr.htk_matrix(512, 40, 16000, 20.0, None), mr.htk_matrix(512, 40, 16000, 20.0, 8000.0))


def test_banks_outside_the_contract_are_refused():
    lib = L.load()
    p = mfcc_amd.make_params(nfft=512, hop=160, nfilters=40, nceptrums=13)
    bad = [_bank(L.MEL_HTK, 4000.0, 4000.0), _bank(L.MEL_HTK, 5000.0, 4000.0),        # low >= high
           _bank(L.MEL_HTK, 8000.0, 0.0),                                              # low >= sample_rate / 2
           _bank(L.MEL_HTK, 0.0, 8000.5), _bank(L.MEL_HTK, 20.0, 16000.0),             # high > sample_rate / 2
           _bank(L.MEL_HTK, -1.0, 0.0), _bank(L.MEL_HTK, float("nan"), 0.0), _bank(L.MEL_HTK, 0.0, float("nan")),
           _bank(L.MEL_NOTEBOOK, 20.0, 0.0), _bank(L.MEL_NOTEBOOK, 0.0, 7600.0),       # the notebook bank has no edges
           _bank(2), _bank(-1),                                                        # unknown kinds
           _bank(L.MEL_HTK, size=28), _bank(L.MEL_HTK, size=0), _bank(L.MEL_NOTEBOOK, size=36)]
    bad += [_bank(kind, reserved=i) for kind in (L.MEL_HTK, L.MEL_NOTEBOOK) for i in range(4)]
    n = C.c_size_t(0)
    for i, b in enumerate(bad):
        h = C.c_void_p()
        assert lib.mfcc_hip_get_table_banked(C.byref(p), 400, C.byref(b), L.TABLE_MEL_DENSE_F32, None, 0, C.byref(n)) \
            == L.ERROR_INVALID_PARAM, i
        assert lib.mfcc_hip_create_banked(C.byref(p), 400, C.byref(b), C.byref(h)) == L.ERROR_INVALID_PARAM and not h.value, i
    # 65 filters: refused as for every bank; a bad frame length or parameter block is refused before the bank is read
    wide = mfcc_amd.make_params(nfft=512, hop=160, nfilters=65, nceptrums=13)
    assert _table(wide, 400, _bank(L.MEL_HTK), L.TABLE_MEL_DENSE_F32)[0] == L.ERROR_INVALID_PARAM
    assert _table(p, 159, _bank(L.MEL_HTK), L.TABLE_MEL_DENSE_F32)[0] == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_create_banked(C.byref(p), 400, C.byref(_bank(L.MEL_HTK)), None) == L.ERROR_INVALID_PARAM
    # the edges of the contract are accepted
    for b in (_bank(L.MEL_HTK, 0.0, 8000.0), _bank(L.MEL_HTK, 7999.0, 0.0), _bank(L.MEL_HTK, 0.0, 1.0)):
        assert _table(p, 400, b, L.TABLE_MEL_DENSE_F32)[0] == L.SUCCESS
    one = mfcc_amd.make_params(nfft=512, hop=160, nfilters=1, nceptrums=1)
    assert _table(one, 400, _bank(L.MEL_HTK), L.TABLE_MEL_DENSE_F32)[0] == L.SUCCESS


def test_an_htk_bank_has_no_filter_points_and_no_fixed_tables():
    # 512 / 170 / 32 is the fixed path's own shape: refused only because of the bank
    for kw, flen in ((dict(nfft=512, nfilters=32, nceptrums=13), 0), (dict(nfft=512, hop=160, nfilters=40, nceptrums=13), 400)):
        p = mfcc_amd.make_params(**kw)
        for which in (L.TABLE_MEL_POINTS_I32, L.TABLE_FX_MEL_DENSE_U32):
            assert _table(p, flen, _bank(L.MEL_HTK, 20.0, 0.0), which)[0] == L.ERROR_UNSUPPORTED
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                mfcc_amd.get_table(which, win_length=flen or None, mel="htk", fmin=20, **kw)
            assert e.value.code == L.ERROR_UNSUPPORTED
        assert _table(p, flen, _bank(L.MEL_HTK, 20.0, 0.0), 99)[0] == L.ERROR_INVALID_PARAM
    p = mfcc_amd.make_params(nfft=512, nfilters=32, nceptrums=13)
    assert _table(p, 0, None, L.TABLE_FX_MEL_DENSE_U32)[0] == L.SUCCESS


def test_python_checks_the_bank_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(mfcc_amd.api._lib, "load", no_library)
    kw = dict(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13)
    for bad in (dict(mel="slaney"), dict(mel=None), dict(mel=1), dict(mel="htk", fmin=-1), dict(mel="htk", fmin=4000, fmax=4000),
                dict(mel="htk", fmin=5000, fmax=4000), dict(mel="htk", fmax=8001), dict(mel="htk", fmax=0),
                dict(mel="htk", fmin="20"), dict(mel="htk", fmin=float("nan")), dict(mel="htk", fmax=float("inf")),
                dict(mel="htk", fmin=True), dict(mel="htk", nfilters=65), dict(mel="htk", nfilters=0),
                dict(mel="notebook", fmin=20), dict(mel="notebook", fmax=7600), dict(fmin=20), dict(fmax=8000)):
        with pytest.raises(ValueError):
            mfcc_amd.MFCC(**dict(kw, **bad))
        tab = {k: v for k, v in dict(kw, **bad).items() if k != "win_length"}
        with pytest.raises(ValueError):
            mfcc_amd.get_table(L.TABLE_MEL_DENSE_F32, win_length=400, **tab)
    with pytest.raises(ValueError):
        mfcc_amd.MFCC(**dict(kw, mel="htk", samplerate=8000, fmax=4001))
