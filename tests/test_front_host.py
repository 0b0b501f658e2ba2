"""The front of a handle -- window function and pre-emphasis pair -- on the CPU: the window tables against the
contract's formulas and scipy, the refusals of ``mfcc_hip_get_table_fronted`` and ``make_params``, the four-wave table
builders through a small C++ driver (tests/front_tables_driver.cpp), the references of tests/front_ref.py against
framed_ref / spectrum_ref on the default front, and the two bounds measured again for every front.  No GPU.

Bound not blind.  ``spectrum_ref``'s constant C_SPEC = 8 is twice the worst ratio of the fp32 restatement at C_SPEC = 1,
rounded up to a power of two.  Measured here with the same procedure for every front of ``front_ref.FRONTS`` (worst ratio,
the input that gives it; the default row is spectrum_ref's own table):

    ======================  ===============  ===============  =================  ==============  =============
    front                   512 / 170 / 512  512 / 160 / 400  1024 / 341 / 1024  256 / 80 / 200  64 / 21 / 64
    ======================  ===============  ===============  =================  ==============  =============
    hamming periodic 31/32  2.73 sine8       2.16 sine8       2.01 sine8         1.04 square     0.69 uniform
    hann periodic 0         1.72 speech      1.71 speech      1.89 sine8         1.15 speech     0.85 const_min
    povey symmetric 32/33   2.06 const_min   1.86 speech      1.21 sine8         0.80 square     0.58 sine8
    hamming symmetric .97   2.70 sine8       1.87 sine8       1.62 const_min     0.95 square     0.69 uniform
    blackman symmetric 0    1.92 sine8       1.81 speech      2.17 sine8         1.30 speech     0.67 noise
    rectangular per. 63/64  2.62 sine8       1.85 sine8       1.61 sine8         1.08 sine8      0.56 square
    ======================  ===============  ===============  =================  ==============  =============

No front exceeds the default's 2.73, so every front is held to C_SPEC = 8 and the restatement to B / 2.

Cepstral bound cap.  On the speech, noise and uniform inputs no frame has an infinite bound at any front (share 0.00 at
512/160/400, 512/170/512, 1024/341/1024 and 256/80/200).  The DC-plus-dither input is kept, but it is a weak input
without pre-emphasis: with ``num = 0`` the DC term is not removed in front of the window, the window's side lobes carry
it into every band, and the bound of such a frame reaches 3e-2 to 8e-2 under Hann / Blackman (6e-5 to 1.4e-2 at the
fronts with pre-emphasis) -- finite, but it pins little.  The test requires finiteness there and nothing more.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.signal import get_window

import framed_ref
import front_ref as fr
import spectrum_ref as sr
from oracle import error_bound as eb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
LENGTHS = [2, 3, 200, 400, 512, 1024]
SCIPY = {"hamming": "hamming", "hann": "hann", "blackman": "blackman"}


@pytest.fixture(scope="module")
def mfcc_amd():
    import mfcc_amd
    return mfcc_amd


def _nfft_of(L):
    nfft = 64
    while nfft < L:
        nfft *= 2
    return nfft


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


# ---- tables
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "symmetric"])
@pytest.mark.parametrize("kind", fr.KINDS)
def test_window_tables_are_the_formulas(mfcc_amd, kind, periodic):
    from mfcc_amd import _lib as L_
    for L in LENGTHS:
        nfft = _nfft_of(L)
        t = mfcc_amd.get_table(L_.TABLE_WINDOW_F32, win_length=L, nfft=nfft, hop=1, window=kind, window_periodic=periodic)
        assert t.dtype == np.float32 and t.shape == (nfft,)
        assert not t[L:].any(), (kind, periodic, L)                      # zero-padded to nfft
        want = fr.window(kind, L, periodic)
        assert _ulps(t[:L], want.astype(np.float32)) <= 1, (kind, periodic, L)
        if kind in SCIPY:
            assert _ulps(t[:L], get_window(SCIPY[kind], L, fftbins=periodic).astype(np.float32)) <= 1, (kind, periodic, L)
        if kind == "rectangular":
            assert (t[:L] == 1.0).all()
        assert np.array_equal(mfcc_amd.window(kind, L, periodic), t[:L])
        # the pair does not enter the table: MFCC_HIP_TABLE_WINDOW_F32 is the window without 1 / den
        t2 = mfcc_amd.get_table(L_.TABLE_WINDOW_F32, win_length=L, nfft=nfft, hop=1, window=kind, window_periodic=periodic,
                                preemph=(97, 100))
        assert np.array_equal(t, t2)


def test_default_front_is_the_framed_table_bit_for_bit(mfcc_amd):
    lib = mfcc_amd.load_library()
    from mfcc_amd import _lib as L_
    for L in LENGTHS:
        nfft = _nfft_of(L)
        p = mfcc_amd.make_params(nfft=nfft, hop=1)
        framed = np.empty(nfft, np.float32)
        n = C.c_size_t(0)
        assert lib.mfcc_hip_get_table_framed(C.byref(p), L, L_.TABLE_WINDOW_F32, framed.ctypes.data, framed.nbytes,
                                             C.byref(n)) == 0 and n.value == framed.nbytes
        for kw in (dict(), dict(window="hamming", window_periodic=True, preemph=(31, 32)), dict(preemph=(62, 64)),
                   dict(preemph=0.96875)):
            t = mfcc_amd.get_table(L_.TABLE_WINDOW_F32, win_length=L, nfft=nfft, hop=1, **kw)
            assert np.array_equal(t.view(np.uint32), framed.view(np.uint32)), (L, kw)
        # front == NULL is mfcc_hip_get_table_banked
        nul = np.empty(nfft, np.float32)
        assert lib.mfcc_hip_get_table_fronted(C.byref(p), L, None, None, L_.TABLE_WINDOW_F32, nul.ctypes.data, nul.nbytes,
                                              C.byref(n)) == 0
        assert np.array_equal(nul.view(np.uint32), framed.view(np.uint32))
        # every other table is the framed handle's too
        for which in (L_.TABLE_MEL_DENSE_F32, L_.TABLE_DCT_F32):
            a = mfcc_amd.get_table(which, win_length=L, nfft=nfft, hop=1, nfilters=8, nceptrums=8)
            b = mfcc_amd.get_table(which, win_length=L, nfft=nfft, hop=1, nfilters=8, nceptrums=8, window="povey",
                                   window_periodic=False, preemph=(32, 33))
            assert np.array_equal(a, b)


# ---- refusals
def _raw_front(window=0, symmetric=0, num=31, den=32, size=None, reserved=(0, 0, 0)):
    from mfcc_amd import _lib as L_
    f = L_.Front()
    f.struct_size = C.sizeof(L_.Front) if size is None else size
    f.window, f.symmetric, f.preemph_num, f.preemph_den = window, symmetric, num, den
    for i, v in enumerate(reserved):
        f.reserved[i] = v
    return f


def _raw_rc(mfcc_amd, front):
    from mfcc_amd import _lib as L_
    lib = mfcc_amd.load_library()
    p = mfcc_amd.make_params()
    n = C.c_size_t(0)
    return lib.mfcc_hip_get_table_fronted(C.byref(p), 0, None, C.byref(front), L_.TABLE_WINDOW_F32, None, 0, C.byref(n))


def test_get_table_fronted_refusals(mfcc_amd):
    from mfcc_amd import _lib as L_
    assert C.sizeof(L_.Front) == 32
    assert _raw_rc(mfcc_amd, _raw_front()) == 0
    bad = [_raw_front(window=-1), _raw_front(window=5), _raw_front(symmetric=2), _raw_front(symmetric=-1),
           _raw_front(den=0), _raw_front(num=33, den=32), _raw_front(num=128, den=128), _raw_front(num=1, den=255),
           _raw_front(num=-1, den=32), _raw_front(size=28), _raw_front(size=36), _raw_front(size=0),
           _raw_front(reserved=(1, 0, 0)), _raw_front(reserved=(0, 0, 7))]
    for f in bad:
        assert _raw_rc(mfcc_amd, f) == L_.ERROR_INVALID_PARAM, (f.window, f.symmetric, f.preemph_num, f.preemph_den,
                                                                 f.struct_size, list(f.reserved))
    # the limits themselves are fine: num = den, num + den = 255, every kind, both forms
    for f in [_raw_front(num=1, den=1), _raw_front(num=127, den=128), _raw_front(num=0, den=255), _raw_front(num=0, den=1)] + \
             [_raw_front(window=k, symmetric=s) for k in range(5) for s in (0, 1)]:
        assert _raw_rc(mfcc_amd, f) == 0
    # a non-default front has no fixed-point table, like a framed handle
    lib = mfcc_amd.load_library()
    p = mfcc_amd.make_params()
    n = C.c_size_t(0)
    hann = _raw_front(window=1, num=0, den=1)
    assert lib.mfcc_hip_get_table_fronted(C.byref(p), 0, None, C.byref(hann), L_.TABLE_FX_MEL_DENSE_U32, None, 0,
                                          C.byref(n)) == L_.ERROR_UNSUPPORTED
    dflt = _raw_front(num=62, den=64)
    assert lib.mfcc_hip_get_table_fronted(C.byref(p), 0, None, C.byref(dflt), L_.TABLE_FX_MEL_DENSE_U32, None, 0,
                                          C.byref(n)) == 0


def test_make_params_refusals_and_the_float_rule(mfcc_amd):
    for bad in (dict(window=-1), dict(window=5), dict(window="hanning"), dict(window_periodic=2), dict(preemph=(31, 0)),
                dict(preemph=(33, 32)), dict(preemph=(128, 128)), dict(preemph=(-1, 32)), dict(preemph=(1, 2, 3)),
                dict(preemph=(0.5, 1)), dict(preemph=1 / 3 + 1e-6), dict(preemph=1.5), dict(preemph=-0.5),
                dict(preemph=float("nan")), dict(preemph="0.97")):
        with pytest.raises(ValueError):
            mfcc_amd.make_params(**bad)
    pair = lambda **kw: (lambda f: (f.preemph_num, f.preemph_den))(mfcc_amd.make_params(**kw).front)      # noqa: E731
    assert pair(preemph=0.97) == (97, 100)
    assert pair(preemph=0.0) == (0, 1) and pair(preemph=0) == (0, 1)
    assert pair(preemph=0.96875) == (31, 32) and pair() == (31, 32)
    assert pair(preemph=1 / 3) == (1, 3) and pair(preemph=1) == (1, 1)
    assert pair(preemph=(62, 64)) == (62, 64)            # the library reduces it (read back through MFCC.front on a GPU)
    f = mfcc_amd.make_params(window="povey", window_periodic=False, preemph=(32, 33)).front
    assert (f.window, f.symmetric, f.preemph_num, f.preemph_den, f.struct_size) == (2, 1, 32, 33, 32)
    assert mfcc_amd.make_params(window=3).front.window == 3


# ---- the four-wave table builders
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("front_tables") / "driver"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(ROOT, "tests", "front_tables_driver.cpp")], check=True)
    return str(exe)


def test_four_wave_tables_carry_the_front(driver):
    # window symmetric num den frame_len: (hann, periodic, 0/1) at 400, (povey, symmetric, 32/33) at 512, the default,
    # and the pair at the fused limit
    cases = ["1 0 0 1 400", "2 1 32 33 512", "0 0 31 32 400", "4 0 63 64 400", "3 1 0 1 160"]
    lines = subprocess.run([driver], input="\n".join(cases) + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for case, line in zip(cases, lines):
        assert line == "ok %d" % (2 * 512 + 512 + 512 + 3), (case, line)


# ---- the references
def test_default_front_is_framed_ref_and_spectrum_ref_bit_for_bit(wav_pcm):
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)      # noqa: E731
    for nfft, hop, L in sr.CONFIGS:
        x = sr.input_list(nfft, hop, L, wav_pcm, frames=9)
        n_mel = 32 if nfft >= 512 else 8
        for ch in x:
            cep, st = fr.fronted_notebook(ch, fr.DEFAULT, L, hop, nfft, n_mel, 16000, sr.power_scale_of(nfft))
            cep0, st0 = framed_ref.framed_notebook(ch, L, hop, nfft, n_mel, 16000, sr.power_scale_of(nfft))
            assert same(cep, cep0) and sorted(st) == sorted(st0) and all(same(st[k], st0[k]) for k in st)
        for pad_mode, halo in sr.FRAMINGS:
            assert same(fr.power_reference(x, fr.DEFAULT, nfft, hop, L, pad_mode=pad_mode, halo=halo),
                        sr.reference(x, nfft, hop, L, pad_mode=pad_mode, halo=halo))
            assert same(fr.restatement_f32(x, fr.DEFAULT, nfft, hop, L, pad_mode=pad_mode, halo=halo),
                        sr.restatement_f32(x, nfft, hop, L, pad_mode=pad_mode, halo=halo))
            assert same(fr.zero_frames(x, fr.DEFAULT, nfft, hop, L, pad_mode, halo),
                        sr.zero_frames(x, nfft, hop, L, pad_mode, halo))
    r0, b0 = framed_ref.reference_and_bound(x[:2], "fp32/fp32", L, hop, nfft, 8, power_scale=sr.power_scale_of(nfft), n_cep=8)
    r1, b1 = fr.reference_and_bound(x[:2], "fp32/fp32", fr.DEFAULT, L, hop, nfft, 8, power_scale=sr.power_scale_of(nfft),
                                    n_cep=8)
    assert same(r0, r1) and same(b0, b1)


def test_references_follow_the_contract():
    """The staging against a direct evaluation: Hann / no pre-emphasis is ``|rfft(x * hann)|^2``, and the pair is exact."""
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, 400 + 160 * 3).astype(np.int16)
    p = fr.power_reference(x, ("hann", True, (0, 1)), 512, 160, 400)
    for f in range(4):
        frame = np.zeros(512)
        frame[:400] = x[160 * f: 160 * f + 400] * get_window("hann", 400, fftbins=True)
        want = np.abs(np.fft.rfft(frame) / 512.0) ** 2
        assert np.allclose(p[f], want, rtol=1e-12, atol=1e-9 * want.max())
    y = fr.pre_emphasis(x, 97, 100)
    assert y[0] == x[0] and np.allclose(y[1:], x[1:] - 0.97 * x[:-1].astype(np.float64), rtol=0, atol=1e-9)
    assert np.array_equal(fr.pre_emphasis(x, 0, 1), x.astype(np.float64))
    # a symmetric window is symmetric, a periodic one is the symmetric one of L + 1 without its last sample
    for kind in fr.KINDS:
        s = fr.window(kind, 401, False)
        assert np.allclose(s, s[::-1], rtol=0, atol=1e-15)
        if kind != "hamming":
            assert np.allclose(fr.window(kind, 400, True), s[:400], rtol=0, atol=1e-15)


# ---- the bounds, measured again
@pytest.mark.parametrize("front", fr.FRONTS, ids=fr.front_id)
def test_spectrum_bound_is_not_blind_at_any_front(front, wav_pcm):
    table = fr.measure(front, wav_pcm)
    print(fr.front_id(front), {k: (round(v, 3), n) for k, (v, n) in table.items()})
    assert sorted(table) == sorted(sr.CONFIGS)
    worst = max(v for v, _ in table.values())
    assert 2.0 * worst <= sr.C_SPEC == 8.0, table                         # the rule that gave C_SPEC holds this front too
    assert sr.c_spec_from(table) <= sr.C_SPEC
    # ... and the restatement stays inside half the bound the kernels are held to
    for nfft, hop, L in sr.CONFIGS:
        x = sr.input_list(nfft, hop, L, wav_pcm)
        for pad_mode, halo in sr.FRAMINGS:
            ref = fr.power_reference(x, front, nfft, hop, L, pad_mode=pad_mode, halo=halo)
            b = sr.bound(ref)
            sr.assert_not_blind(b, fr.zero_frames(x, front, nfft, hop, L, pad_mode, halo), fr.front_id(front))
            got = fr.restatement_f32(x, front, nfft, hop, L, pad_mode=pad_mode, halo=halo)
            sr.check(got, ref, b, "%s %s %s" % (fr.front_id(front), (nfft, hop, L), pad_mode), limit=0.5)


def _dc_dither(n, seed):
    rng = np.random.default_rng(seed)
    return (12000 + rng.integers(-2, 3, n)).astype(np.int16)


CAP_CONFIGS = [(512, 160, 400, 32, "bf16x2/fp32"), (512, 170, 512, 32, "bf16x2/fp32"), (1024, 341, 1024, 32, "fp32/fp32"),
               (256, 80, 200, 20, "fp32/fp32")]


@pytest.mark.parametrize("front", fr.FRONTS, ids=fr.front_id)
def test_cepstral_bound_is_finite_on_live_inputs(front, wav_pcm):
    import kernel_families as kf
    for nfft, hop, L, n_mel, model in CAP_CONFIGS:
        n = sr.samples_for(sr.MAX_FRAMES, L, hop)
        x = np.stack([kf.signal(k, n, 11 + i, wav_pcm) for i, k in enumerate(["speech", "noise", "uniform"])]
                     + [_dc_dither(n, 3)])
        _, b = fr.reference_and_bound(x, model, front, L, hop, nfft, n_mel, 16000, sr.power_scale_of(nfft), n_cep=13)
        assert b.shape == (4, sr.MAX_FRAMES, 13)
        share = float(np.isposinf(b[:3]).any(axis=-1).mean())
        print(fr.front_id(front), (nfft, hop, L), "infinite share %.2f" % share, "dc+dither max bound %.3g" % np.nanmax(b[3]))
        assert share == 0.0 and np.isfinite(b[:3]).all(), (front, nfft, hop, L)
        assert np.isfinite(b[3]).all(), (front, nfft, hop, L)             # kept, weak without pre-emphasis (docstring)
