"""CPU-side checks of PCEN (``MFCC(output="logmel", pcen=...)``, ``mfcc_hip_set_pcen``, ``mfcc_hip_pcen_dev``,
``mfcc_hip_bank_create_online_pcen``): the host-only constants against float64 pow, the closed forms of the definition,
the tile form's restatement against the definition under the bound of tests/pcen_ref.py, the Python argument checks and
the refusals that need no GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import mfcc_amd
import pcen_ref as pr
from mfcc_amd import _lib as L
from mfcc_amd import api


def _block(s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6):
    p = L.Pcen()
    p.struct_size = C.sizeof(L.Pcen)
    p.s, p.alpha, p.delta, p.r, p.eps = s, alpha, delta, r, eps
    return p


def _constants(p):
    lib = mfcc_amd.load_library()
    decay = np.empty(L.PCEN_TILE, dtype=np.float32)
    a, dr = C.c_float(), C.c_float()
    rc = lib.mfcc_hip_pcen_constants(C.byref(p), decay.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(dr))
    return rc, decay, np.float32(a.value), np.float32(dr.value)


def test_struct_and_defaults():
    lib = mfcc_amd.load_library()
    assert C.sizeof(L.Pcen) == 36 and L.PCEN_TILE == pr.TILE == 128
    p = L.Pcen()
    assert lib.mfcc_hip_pcen_defaults(C.byref(p)) == L.SUCCESS
    assert p.struct_size == 36 and list(p.reserved) == [0, 0, 0]
    got = (p.s, p.alpha, p.delta, p.r, p.eps)
    assert got == tuple(pr.f32(v) for v in pr.DEFAULTS)
    assert lib.mfcc_hip_pcen_defaults(None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_abi_version() == 2 and C.sizeof(L.Params) == 64
    src = open(os.path.join(os.path.dirname(L.__file__), "..", "include", "mfcc_hip.h")).read()
    assert "#define MFCC_HIP_PCEN_TILE 128" in src and "#define MFCC_HIP_ABI_VERSION 2" in src


@pytest.mark.parametrize("ps", pr.PARAM_SETS + [(0.5, 0.0, 0.0, 1.0, 1.0), (np.float32(1e-4), 0.5, 1e-3, 0.3, 1e-10)])
def test_constants_are_float64_pow_rounded_once(ps):
    s, alpha, delta, r, eps = ps
    rc, decay, a, dr = _constants(_block(s, alpha, delta, r, eps))
    assert rc == L.SUCCESS
    d = 1.0 - float(np.float32(s))
    want = np.array([math.pow(d, k + 1.0) for k in range(128)]).astype(np.float32)
    assert np.array_equal(decay.view(np.uint32), want.view(np.uint32))
    assert a.view(np.uint32) == np.float32(d).view(np.uint32)
    assert dr.view(np.uint32) == np.float32(math.pow(float(np.float32(delta)), float(np.float32(r)))).view(np.uint32)
    rdecay, ra, rdr = pr.constants(s, delta, r)
    assert np.array_equal(rdecay, decay) and ra == a and rdr == dr
    # the Python helper is the same call
    pd, pa, pdr = mfcc_amd.pcen_constants(dict(s=s, alpha=alpha, delta=delta, r=r, eps=eps))
    assert np.array_equal(pd, decay) and pa == a and pdr == dr


def test_bad_blocks_are_refused_without_a_gpu():
    lib = mfcc_amd.load_library()
    nan, inf = float("nan"), float("inf")
    bad = [dict(s=0.0), dict(s=-0.1), dict(s=1.5), dict(s=nan), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=nan),
           dict(delta=-1.0), dict(delta=inf), dict(r=0.0), dict(r=1.5), dict(r=nan), dict(eps=0.0), dict(eps=-1e-6),
           dict(eps=inf)]
    for kw in bad:
        assert _constants(_block(**kw))[0] == L.ERROR_INVALID_PARAM, kw
    p = _block()
    p.struct_size = 32
    assert _constants(p)[0] == L.ERROR_INVALID_PARAM
    p = _block()
    p.reserved[1] = 1
    assert _constants(p)[0] == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_pcen_constants(None, None, None, None) == L.ERROR_INVALID_PARAM
    # the edges of the ranges are inside
    for kw in [dict(s=1.0), dict(alpha=0.0), dict(alpha=1.0), dict(delta=0.0), dict(r=1.0), dict(eps=1e-30)]:
        assert _constants(_block(**kw))[0] == L.SUCCESS, kw
    assert lib.mfcc_hip_pcen_constants(C.byref(_block()), None, None, None) == L.SUCCESS


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = mfcc_amd.load_library()
    off = (C.c_size_t * 3)(0, 4, 8)
    ok = _block()
    assert lib.mfcc_hip_set_pcen(None, C.byref(ok)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_pcen(None, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_pcen_dev(None, None, 13, off, 2, C.byref(ok)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_pcen_dev(None, None, 13, None, 0, None) == L.ERROR_INVALID_PARAM
    b = C.c_void_p()
    assert lib.mfcc_hip_bank_create_online_pcen(None, 4, C.byref(ok), 0, 0, 0, 2, C.byref(b)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_bank_create_online_pcen(None, 4, None, 0, 0, 0, 2, C.byref(b)) == L.ERROR_INVALID_PARAM
    for name in ["mfcc_hip_pcen_defaults", "mfcc_hip_pcen_constants", "mfcc_hip_set_pcen", "mfcc_hip_pcen_dev",
                 "mfcc_hip_bank_create_online_pcen"]:
        assert name in L.SYMBOLS


# ---- the definition's closed forms

def test_constant_energy_gives_a_constant_output():
    x = np.full((700, 3), 11.25, dtype=np.float32)
    x[:, 1] = -3.5
    x[:, 2] = 20.0
    for ps in pr.PARAM_SETS:
        s, alpha, delta, r, eps = (pr.f32(v) for v in ps)
        E = np.exp2(x[0].astype(np.float64))
        want = (E / (eps + E) ** alpha + delta) ** r - delta ** r
        ref = pr.pcen_f64(x, None, *ps)
        np.testing.assert_allclose(ref, np.broadcast_to(want, ref.shape), rtol=1e-12)
        got = pr.pcen_tiled(x, None, *ps)
        pr.check(got, ref, delta, r, what="constant E %r" % (ps,))
        # the tile form holds M = E to rounding over five tiles: nothing accumulates
        assert np.abs(got[-1] - got[0]).max() <= 4 * pr.C * (np.abs(want).max() + delta ** r)


def test_s_one_gives_m_equal_e():
    rng = np.random.default_rng(3)
    x = rng.uniform(-5, 22, (300, 8)).astype(np.float32)
    s, alpha, delta, r, eps = pr.PARAM_SETS[2]
    assert s == 1.0
    E = np.exp2(x.astype(np.float64))
    a, d, rr, e = pr.f32(alpha), pr.f32(delta), pr.f32(r), pr.f32(eps)
    want = (E / (e + E) ** a + d) ** rr - d ** rr
    np.testing.assert_allclose(pr.pcen_f64(x, None, *pr.PARAM_SETS[2]), want, rtol=1e-12)
    decay, a32, _ = pr.constants(1.0, delta, r)
    assert a32 == 0 and np.all(decay == 0)                      # no carry, no memory
    pr.check(pr.pcen_tiled(x, None, *pr.PARAM_SETS[2]), want, delta, r, what="s = 1")


def test_an_all_silent_segment_gives_zero():
    x = np.full((260, 5), -np.inf, dtype=np.float32)
    x[:, 1] = np.nan
    x[:, 2] = np.inf                                            # every non-finite value counts as E = 0
    for ps in pr.PARAM_SETS:
        assert np.all(pr.pcen_f64(x, None, *ps) == 0.0)
        got = pr.pcen_tiled(x, None, *ps)
        assert np.all(got == 0.0) and got.dtype == np.float32


def test_segments_are_independent_and_rows_outside_them_stay():
    rng = np.random.default_rng(4)
    x = rng.uniform(0, 20, (400, 4)).astype(np.float32)
    off = [10, 10, 150, 390]
    got = pr.pcen_tiled(x, off)
    assert np.array_equal(got[:10], x[:10]) and np.array_equal(got[390:], x[390:])
    assert np.array_equal(got[10:150], pr.pcen_tiled(x[10:150]))
    assert np.array_equal(got[150:390], pr.pcen_tiled(x[150:390]))


# ---- the tile form against the definition

def test_restatement_meets_the_definition_on_the_golden_rows(golden_dir):
    x = pr.golden_rows(golden_dir)
    assert x.shape == (1046, 32) and np.isinf(x[0, 5]) and np.isinf(x).sum() > 500
    worst = 0.0
    for ps in pr.PARAM_SETS:
        ref = pr.pcen_f64(x, None, *ps)
        got = pr.pcen_tiled(x, None, *ps)
        e = pr.check(got, ref, ps[2], ps[3], what="%r" % (ps,))
        print("restatement vs definition %r: %.3g" % (ps, e))
        worst = max(worst, e)
    # the figure C was derived from (pcen_ref.MEASURED), measured again
    assert worst <= pr.MEASURED * 1.01
    assert pr.C == 8 * pr.MEASURED and pr.C <= 1e-4


def test_bound_rejects_a_wrong_value_and_handles_delta_zero(golden_dir):
    x = pr.golden_rows(golden_dir)[:200]
    ps = pr.PARAM_SETS[3]
    assert ps[2] == 0.0
    ref = pr.pcen_f64(x, None, *ps)
    got = pr.pcen_tiled(x, None, *ps)
    assert np.any(ref == 0.0)                                   # silent entries: the bound there is got == 0
    pr.check(got, ref, ps[2], ps[3])
    bad = got.copy()
    i = np.unravel_index(np.argmax(ref), ref.shape)
    bad[i] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError):
        pr.check(bad, ref, ps[2], ps[3])
    bad = got.copy()
    bad[np.argwhere(ref == 0.0)[0][0], np.argwhere(ref == 0.0)[0][1]] = 1e-30
    with pytest.raises(AssertionError):
        pr.check(bad, ref, ps[2], ps[3])


# ---- Python

def test_python_argument_validation():
    f = api._pcen_args
    assert f(None) is None and f(False) is None
    p = f(True)
    assert (p.s, p.alpha, p.delta, p.r, p.eps) == tuple(pr.f32(v) for v in pr.DEFAULTS) and p.struct_size == 36
    p = f(dict(s=0.04, alpha=0.8, delta=10, r=0.25))
    assert (p.s, p.alpha, p.delta, p.r, p.eps) == tuple(pr.f32(v) for v in (0.04, 0.8, 10, 0.25, 1e-6))
    p = f(True, r=np.float32(1.0), delta=0)
    assert p.r == 1.0 and p.delta == 0.0
    nan, inf = float("nan"), float("inf")
    bad = [dict(s=0), dict(s=1.0001), dict(s=nan), dict(s="0.1"), dict(s=True), dict(s=None), dict(alpha=-1e-3),
           dict(alpha=2), dict(alpha=inf), dict(delta=-1), dict(delta=1e39), dict(r=0), dict(r=1.1), dict(r=[0.5]),
           dict(eps=0), dict(eps=1e-60), dict(eps=-1), dict(eps=nan), dict(gain=0.98), dict(s=0.1, time_constant=0.4),
           dict(time_constant=0), dict(time_constant=-1), dict(time_constant=inf), dict(time_constant="1")]
    for kw in bad:
        with pytest.raises(ValueError):
            f(kw)
        with pytest.raises(ValueError):
            f(True, **kw)
    for notdict in [1, "on", 0.5, [0.025], (0.025, 0.98)]:
        with pytest.raises(ValueError):
            f(notdict)
    with pytest.raises(ValueError):
        f(None, s=0.1)                                          # parameters without pcen


def test_time_constant_is_librosas_formula():
    for tc, sr, hop in [(0.4, 22050, 512), (0.4, 16000, 170), (0.06, 16000, 160), (2.0, 8000, 80)]:
        t = tc * sr / hop
        want = (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)
        assert mfcc_amd.pcen_smoothing(tc, sr, hop) == pytest.approx(want, rel=1e-14)
        p = api._pcen_args(dict(time_constant=tc), sr, hop)
        assert p.s == pr.f32(want)
    # librosa's documented default: time_constant 0.4 s at sr 22050, hop 512 gives b = 0.0562...
    assert mfcc_amd.pcen_smoothing(0.4, 22050, 512) == pytest.approx(0.05638, abs=5e-5)


def test_constructor_validates_the_keyword_before_the_device():
    import torch
    for bad in [dict(s=0), dict(r=2), "yes", dict(foo=1)]:
        with pytest.raises(ValueError):
            mfcc_amd.MFCC(nfilters=32, nceptrums=13, output="logmel", pcen=bad)
    if not torch.cuda.is_available():                          # with a GPU tests/test_gpu_pcen.py covers the handle
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            mfcc_amd.MFCC(nfilters=32, nceptrums=13, output="logmel", pcen=True)
        assert e.value.code == L.ERROR_NOT_FOUND
