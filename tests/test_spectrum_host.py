"""CPU-side checks of the power-spectrum output: the reference and its bound (tests/spectrum_ref.py), the host-only entry
point, the Python argument checks, and everything mfcc_amd/csrc/spectrum_plan.hpp decides, through
tests/spectrum_plan_driver.cpp (plain and built with -fsanitize=address,undefined)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mfcc_amd
import spectrum_ref as sr
from mfcc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")


# ---- the reference
def test_reference_reproduces_the_golden_power(golden_dir, wav_pcm):
    st = np.load(os.path.join(golden_dir, "f2bjrop_float64_stages.npz"))
    ref = sr.reference(wav_pcm)
    assert ref.shape == (1046, 257) and ref.dtype == np.float64
    assert np.array_equal(ref[st["frames_sel"]], st["power"])


def test_framed_reference_at_full_length_is_the_notebooks(wav_pcm):
    x = wav_pcm[4000:4000 + sr.samples_for(9, 512, 160)]
    a = sr.reference(x, 512, 160, 512)
    # the framed staging with L = nfft, which reference() itself never takes
    from oracle import mfcc_float as mf
    framed = mf.frame_audio(mf.pre_emphasis(x), nfft=512, hop=160) * mf.hamming_window(512)
    assert np.array_equal(a, mf.power_spectrum(mf.fft_frames(framed, 512), 512.0))


@pytest.fixture(scope="module")
def table(wav_pcm):
    return sr.measure(wav_pcm)


def test_c_spec_is_what_the_measurement_gives(table):
    """C_SPEC = twice the restatement's worst ratio at C_SPEC = 1, rounded up to a power of two, at most 8."""
    for cfg, (worst, kind) in table.items():
        print("fp32 restatement %s: worst |delta| / B(1) %.2f (%s)" % (cfg, worst, kind))
    assert set(table) == set(sr.CONFIGS)
    assert sr.c_spec_from(table) == sr.C_SPEC <= sr.C_SPEC_CAP == 8.0
    assert max(v for v, _ in table.values()) > 1.0          # C_SPEC = 1 does not hold a plain fp32 FFT


@pytest.mark.parametrize("cfg", sr.CONFIGS, ids=lambda c: "%d_%d_%d" % c)
def test_fp32_restatement_within_half_the_bound(wav_pcm, cfg):
    nfft, hop, flen = cfg
    x = sr.input_list(nfft, hop, flen, wav_pcm)
    seen_zero = 0
    for pad_mode, halo in sr.FRAMINGS:
        ref = sr.reference(x, nfft, hop, flen, pad_mode=pad_mode, halo=halo)
        assert ref.shape == (len(sr.KINDS), sr.num_frames(x.shape[1] - halo, flen, hop, pad_mode), nfft // 2 + 1)
        b = sr.bound(ref)
        zero = sr.zero_frames(x, nfft, hop, flen, pad_mode, halo)
        sr.assert_not_blind(b, zero, "%s %s halo %d" % (cfg, pad_mode, halo))
        got = sr.restatement_f32(x, nfft, hop, flen, pad_mode=pad_mode, halo=halo)
        worst = sr.check(got, ref, b, "%s %s halo %d" % (cfg, pad_mode, halo), limit=0.5)
        print("restatement %s %s halo %d: worst |delta| / B %.3f, %d all-zero frames" % (cfg, pad_mode, halo, worst, zero.sum()))
        seen_zero += int(zero.sum())
    assert seen_zero > 0                                    # the `silences` kind pins exact zeros


def test_fused_steady_state_batch_within_half_the_bound(wav_pcm):
    _, frames, nch = sr.steady_shape(sr.MI355X_CUS)
    for nfft, hop, flen in sr.CONFIGS[:2]:
        x = sr.batch_inputs(nfft, hop, flen, wav_pcm, nch, frames)
        ref = sr.reference(x, nfft, hop, flen)
        sr.check(sr.restatement_f32(x, nfft, hop, flen), ref, sr.bound(ref), "steady batch %d/%d" % (flen, hop), limit=0.5)


def test_check_refuses_what_it_must():
    ref = np.full((2, 3), 4.0)
    ref[1] = 0.0
    b = sr.bound(ref)
    assert (b[0] > 0).all() and (b[1] == 0).all()
    good = ref.astype(np.float32)
    assert sr.check(good, ref, b) == 0.0
    for bad, msg in [(np.where(ref > 0, np.nan, 0.0), "NaN"), (-good, "negative"), (good[:1], "shape"),
                     (good + np.float32(1e-30), "not \\+0.0"), (good * np.float32(1.01), "over")]:
        with pytest.raises(AssertionError, match=msg):
            sr.check(np.asarray(bad, np.float32), ref, b)
    neg0 = good.copy()
    neg0[1, 0] = -0.0
    with pytest.raises(AssertionError, match="negative"):
        sr.check(neg0, ref, b)
    with pytest.raises(AssertionError):
        sr.assert_not_blind(b, np.array([True, True]))


# ---- the host-only entry point and the Python layer
def test_spectrum_bins_and_its_refusals():
    lib = L.load()
    out = C.c_size_t(0)
    for nfft in (64, 128, 256, 512, 1024):
        kw = dict(nfft=nfft, nfilters=8, nceptrums=8)
        assert mfcc_amd.spectrum_bins(**kw) == nfft // 2 + 1
        p = mfcc_amd.make_params(**kw)
        assert lib.mfcc_hip_spectrum_bins(C.byref(p), C.byref(out)) == L.SUCCESS and out.value == nfft // 2 + 1
        assert lib.mfcc_hip_spectrum_bins(C.byref(p), None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_spectrum_bins(None, C.byref(out)) == L.ERROR_INVALID_PARAM
    for kw in [dict(nfft=500), dict(nfft=2048), dict(nfft=32), dict(nfilters=65), dict(hop=600), dict(output=2)]:
        p = mfcc_amd.make_params(**kw)
        assert lib.mfcc_hip_spectrum_bins(C.byref(p), C.byref(out)) == L.ERROR_INVALID_PARAM, kw
    p = mfcc_amd.make_params()
    p.reserved[1] = 1
    assert lib.mfcc_hip_spectrum_bins(C.byref(p), C.byref(out)) == L.ERROR_INVALID_PARAM
    # the settings that do not apply to the spectrum do not change it
    assert mfcc_amd.spectrum_bins(output="logmel", nfilters=64, nceptrums=13) == 257


def test_abi_is_unchanged_and_the_symbols_are_typed():
    assert C.sizeof(L.Params) == 64 and L.load().mfcc_hip_abi_version() == 2
    names = ["mfcc_hip_spectrum_bins", "mfcc_hip_spectrum_i16_dev", "mfcc_hip_spectrum_ragged_i16_dev",
             "mfcc_hip_spectrum_i16", "mfcc_hip_spectrum_kernel_name"]
    for n in names:
        assert n in L.SYMBOLS
    assert sorted(s for s in L.SYMBOLS if "spectrum" in s) == sorted(names)
    assert L.SYMBOLS["mfcc_hip_spectrum_i16_dev"] == L.SYMBOLS["mfcc_hip_process_i16_dev"]
    assert L.SYMBOLS["mfcc_hip_spectrum_ragged_i16_dev"] == L.SYMBOLS["mfcc_hip_process_ragged_i16_dev"]
    assert L.SYMBOLS["mfcc_hip_spectrum_i16"] == L.SYMBOLS["mfcc_hip_process_i16"]
    assert L.load().mfcc_hip_spectrum_kernel_name(None) == b""


def test_python_argument_checks_without_a_handle():
    m = mfcc_amd.MFCC.__new__(mfcc_amd.MFCC)
    m.nfft, m.sample_format = 1024, "s16"
    assert m.num_bins == 513
    x = np.zeros(2048, np.int16)
    with pytest.raises(ValueError, match="halo"):
        m.power_spectrum(x, halo=1)
    with pytest.raises(ValueError, match="out"):
        m.power_spectrum(x, out=np.zeros((1, 513), np.float32))
    with pytest.raises(TypeError):
        m.power_spectrum(x.astype(np.float32))


def test_compute_entries_need_a_gpu():
    import torch
    lib = L.load()
    got = C.c_size_t(0)
    # without a handle every compute entry refuses
    assert lib.mfcc_hip_spectrum_i16(None, None, 0, 0, None, 0, C.byref(got)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_spectrum_i16_dev(None, None, 0, 0, 0, 0, None, C.byref(got)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_spectrum_ragged_i16_dev(None, None, None, 0, None, 0, None) == L.ERROR_INVALID_PARAM
    if torch.cuda.is_available():
        return                                              # tests/test_gpu_spectrum.py has the handle
    # no CPU path: the handle cannot be made, so nothing computes
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13).power_spectrum(np.zeros(1024, np.int16))
    assert e.value.code == L.ERROR_NOT_FOUND


# ---- spectrum_plan.hpp through its driver
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("spectrum_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "spectrum_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


def both(drivers, lines):
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    a, b = (subprocess.run([d], input=text, capture_output=True, text=True, check=True).stdout.splitlines() for d in drivers)
    assert a == b and len(a) == len(lines)
    return a


FUSED, GENERIC = "mfcc_spectrum512_kernel", "mfcc_spectrum_generic_kernel"


def test_plan_kernel_choice(drivers):
    cases = [((512, 170, 512, 0), FUSED), ((512, 160, 400, 0), FUSED), ((512, 160, 160, 0), FUSED), ((512, 160, 512, 0), FUSED),
             ((512, 171, 512, 0), GENERIC), ((256, 85, 256, 0), GENERIC), ((1024, 341, 1024, 0), GENERIC),
             ((512, 170, 400, 0), GENERIC), ((512, 160, 159, 0), GENERIC), ((1024, 160, 400, 0), GENERIC),
             ((512, 170, 512, 1), GENERIC), ((512, 160, 400, 1), GENERIC)]
    got = both(drivers, [("choose",) + c for c, _ in cases])
    for (c, name), line in zip(cases, got):
        k, n, sup = line.split()
        assert n == name and int(k) == int(name == FUSED), (c, line)
        assert int(sup) == int(name == FUSED or c[3] == 1), (c, line)
    assert both(drivers, [("bins", n) for n in (64, 512, 1024)]) == ["33", "257", "513"]


def test_plan_store_geometry(drivers):
    """Every output alignment mod 4 x rows 1, 15, 16 against the brute-force list of what the kernel's store loop
    writes: each element of the span exactly once from its own LDS word, every vector store 16-byte aligned on both
    sides, at most three floats in front and behind."""
    base = 0x7f12_3456_7800 // 4                            # a 16-byte-aligned address, in floats
    cases = [(base + off + 257 * first_row, rows) for off in range(4) for first_row in (0, 1, 2, 3, 16) for rows in (1, 15, 16)]
    got = both(drivers, [("store", w, rows, 257) for w, rows in cases])
    seen_pads = set()
    for (word, rows), line in zip(cases, got):
        head, stores = line.split(" |")
        pad, lead, nvec, tail, count = (int(v) for v in head.split())
        assert count == rows * 257 and pad == word % 4 and lead == (4 - pad) % 4 and lead + 4 * nvec + tail == count
        assert 0 <= lead <= 3 and 0 <= tail <= 3
        assert pad + count <= 257 * 16 + 4                  # inside the LDS image (kRWords)
        tok = stores.split()
        written = np.zeros(count, int)
        n_s = n_v = 0
        for kind, e, w in zip(tok[0::3], tok[1::3], tok[2::3]):
            e, w = int(e), int(w)
            assert w == pad + e                             # element e comes from its own LDS word
            if kind == "v":
                assert (word + e) % 4 == 0 and w % 4 == 0   # 16-byte aligned in HBM and in LDS
                written[e:e + 4] += 1
                n_v += 1
            else:
                written[e] += 1
                n_s += 1
        assert (written == 1).all() and n_v == nvec and n_s == lead + tail
        seen_pads.add(pad)
    assert seen_pads == {0, 1, 2, 3}


def test_plan_limits(drivers):
    max_elems, tile, tile_elems, r_words = (int(v) for v in both(drivers, [("limits",)])[0].split())
    assert (max_elems, tile, tile_elems, r_words) == (1 << 62, 16, 16 * 257, 16 * 257 + 4)
    q = max_elems // 257
    assert both(drivers, [("fits", q, 257), ("fits", q + 1, 257), ("fits", 1 << 63, 0), ("fits", 0, 513)]) == ["1", "0", "1", "1"]
    lines = [("callfits", 9_600_000, 64, 257), ("callfits", 1 << 62, 1, 257), ("callfits", 1 << 40, 1 << 20, 257),
             ("callfits", 1 << 40, 0, 257), ("callfits", 100, 1 << 61, 257), ("callfits", (1 << 62) - 1, 1, 33)]
    assert both(drivers, lines) == ["1", "0", "0", "1", "0", "0"]
    # a ragged call: at most span + 2 n_utt rows
    lines = [("raggedfits", 1_600_000_000, 10_000, 257), ("raggedfits", 0, 0, 257), ("raggedfits", q - 20, 10, 257),
             ("raggedfits", q - 19, 10, 257), ("raggedfits", 1 << 61, 1, 33), ("raggedfits", 10, 1 << 61, 33)]
    assert both(drivers, lines) == ["1", "1", "1", "0", "0", "0"]
