"""CPU-side checks of the filterbank output: the exports, ``mfcc_hip_htk_weights``, the refusals of ``mfcc_hip_set_fbank``'s
arguments and of the Python layer, everything mfcc_amd/csrc/fbank_plan.hpp decides (through tests/fbank_plan_driver.cpp,
plain and built with -fsanitize=address,undefined), and the reference and bound of tests/fbank_ref.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fbank_ref as fr
import mfcc_amd
import spectrum_ref as sr
from mfcc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
FUSED, GENERIC = "mfcc_fbank512_kernel", "mfcc_fbank_generic_kernel"
NAMES = ["mfcc_hip_set_fbank", "mfcc_hip_fbank_bands", "mfcc_hip_fbank_i16_dev", "mfcc_hip_fbank_ragged_i16_dev",
         "mfcc_hip_fbank_i16", "mfcc_hip_fbank_kernel_name", "mfcc_hip_htk_weights"]


# ---- exports and ABI
def test_abi_is_unchanged_and_the_symbols_are_typed():
    lib = L.load()
    assert C.sizeof(L.Params) == 64 and lib.mfcc_hip_abi_version() == 2
    assert C.sizeof(L.Fbank) == 32 and L.MAX_FBANK_BANDS == 128
    for n in NAMES:
        assert n in L.SYMBOLS and getattr(lib, n)
    assert sorted(s for s in L.SYMBOLS if "fbank" in s or "htk_weights" in s) == sorted(NAMES)
    assert L.SYMBOLS["mfcc_hip_fbank_i16_dev"] == L.SYMBOLS["mfcc_hip_spectrum_i16_dev"]
    assert L.SYMBOLS["mfcc_hip_fbank_ragged_i16_dev"] == L.SYMBOLS["mfcc_hip_spectrum_ragged_i16_dev"]
    assert L.SYMBOLS["mfcc_hip_fbank_i16"] == L.SYMBOLS["mfcc_hip_spectrum_i16"]
    assert lib.mfcc_hip_fbank_kernel_name(None) == b""
    with open(os.path.join(ROOT, "include", "mfcc_hip.h")) as f:
        header = f.read()
    for n in NAMES + ["MFCC_HIP_MAX_FBANK_BANDS 128", "MFCC_HIP_FBANK_LOG10 = 3"]:
        assert n in header
    # the limits of 64 stay where they were
    out = C.c_size_t(0)
    p = mfcc_amd.make_params(nfilters=65)
    assert lib.mfcc_hip_spectrum_bins(C.byref(p), C.byref(out)) == L.ERROR_INVALID_PARAM


# ---- mfcc_hip_htk_weights
@pytest.mark.parametrize("n_bands", [23, 40, 64])
def test_htk_weights_are_the_handles_table(n_bands):
    for nfft, rate, fmin, fmax in ((512, 16000, 0.0, None), (512, 16000, 20.0, 7600.0), (256, 8000, 64.0, None)):
        w = mfcc_amd.htk_filterbank(n_bands, nfft=nfft, samplerate=rate, fmin=fmin, fmax=fmax)
        t = mfcc_amd.get_table(L.TABLE_MEL_DENSE_F32, mel="htk", fmin=fmin, fmax=fmax, nfft=nfft, samplerate=rate,
                               nfilters=n_bands, nceptrums=8)
        assert w.dtype == np.float32 and w.shape == (n_bands, nfft // 2 + 1)
        assert np.array_equal(w.view(np.uint32).ravel(), t.view(np.uint32))


@pytest.mark.parametrize("n_bands", [80, 128])
def test_htk_weights_are_the_float64_formula_rounded_once(n_bands):
    for nfft, rate, fmin, fmax in ((512, 16000, 0.0, None), (512, 16000, 20.0, 7600.0), (1024, 16000, 0.0, 8000.0)):
        w = mfcc_amd.htk_filterbank(n_bands, nfft=nfft, samplerate=rate, fmin=fmin, fmax=fmax)
        assert np.array_equal(w.view(np.uint32), fr.htk_weights(n_bands, nfft, rate, fmin, fmax).view(np.uint32))
    assert (w >= 0).all()


def test_htk_128_bands_at_512_has_exactly_one_empty_band():
    w = mfcc_amd.htk_filterbank(128)
    assert int((fr.nnz(w) == 0).sum()) == 1
    assert int((fr.nnz(mfcc_amd.htk_filterbank(80)) == 0).sum()) == 0


def test_htk_weights_refusals():
    lib = L.load()
    n = C.c_size_t(0)
    buf = np.empty(80 * 257, np.float32)
    call = lib.mfcc_hip_htk_weights
    assert call(512, 16000, 80, 0.0, 0.0, None, 0, C.byref(n)) == L.SUCCESS and n.value == 80 * 257
    assert call(512, 16000, 80, 0.0, 0.0, L.ptr(buf), buf.size, None) == L.SUCCESS
    assert call(512, 16000, 80, 0.0, 0.0, L.ptr(buf), buf.size - 1, C.byref(n)) == L.ERROR_BUFFER_SMALL and n.value == 80 * 257
    for bad in [(500, 16000, 80, 0.0, 0.0), (2048, 16000, 80, 0.0, 0.0), (32, 16000, 8, 0.0, 0.0), (512, 0, 80, 0.0, 0.0),
                (512, 16000, 0, 0.0, 0.0), (512, 16000, 129, 0.0, 0.0), (512, 16000, 80, -1.0, 0.0),
                (512, 16000, 80, 4000.0, 4000.0), (512, 16000, 80, 0.0, 8001.0), (512, 16000, 80, float("nan"), 0.0)]:
        assert call(*bad, L.ptr(buf), buf.size, C.byref(n)) == L.ERROR_INVALID_PARAM, bad
    with pytest.raises(ValueError):
        mfcc_amd.htk_filterbank(80, samplerate=16000.5)


# ---- refusals of the arguments: the library's own (no handle is needed to refuse) and the Python layer's
def test_python_argument_checks_without_a_handle():
    from mfcc_amd.api import _fbank_args
    good = fr.htk_weights(80)
    p, w = _fbank_args(good, "ln", 1.1920929e-07, 257)
    assert (p.struct_size, p.n_bands, p.scale) == (32, 80, L.FBANK_LN) and p.floor == np.float32(1.1920929e-07)
    assert w.dtype == np.float32 and w.flags.c_contiguous and np.array_equal(w, good)
    assert _fbank_args(good.astype(np.float64), "energy", 0.0, 257)[1].dtype == np.float32
    import torch
    assert np.array_equal(_fbank_args(torch.from_numpy(good), "log2", 0.0, 257)[1], good)
    for bad in (np.zeros((0, 257), np.float32), np.zeros((129, 257), np.float32), np.zeros((80, 256), np.float32),
                np.zeros((80, 513), np.float32), np.zeros(257, np.float32), np.zeros((2, 40, 257), np.float32)):
        with pytest.raises(ValueError):
            _fbank_args(bad, "log2", 0.0, 257)
    for v in (np.nan, np.inf, -np.inf, -1e-30):
        w = good.copy()
        w[17, 60] = v
        with pytest.raises(ValueError, match="finite and not negative"):
            _fbank_args(w, "log2", 0.0, 257)
    w = good.copy()
    w[3, 200] = -0.0                                         # -0.0 counts as 0
    _fbank_args(w, "log2", 0.0, 257)
    with pytest.raises(TypeError):
        _fbank_args(good.astype(np.complex64), "log2", 0.0, 257)
    for scale in ("log", "LOG2", 1, None):
        with pytest.raises(ValueError, match="scale"):
            _fbank_args(good, scale, 0.0, 257)
    for floor in (-1.0, np.nan, np.inf, -1e-40, 1e39):
        with pytest.raises(ValueError, match="floor"):
            _fbank_args(good, "log2", floor, 257)
    m = mfcc_amd.MFCC.__new__(mfcc_amd.MFCC)
    m.nfft, m.sample_format = 512, "s16"
    x = np.zeros(2048, np.int16)
    with pytest.raises(ValueError, match="halo"):
        m.filterbank(x, halo=1)
    with pytest.raises(ValueError, match="out"):
        m.filterbank(x, out=np.zeros((1, 80), np.float32))


def test_entries_without_a_handle_and_without_a_gpu():
    import torch
    lib = L.load()
    got = C.c_size_t(0)
    p = L.Fbank(struct_size=32, n_bands=80, scale=1, floor=0.0)
    w = fr.htk_weights(80)
    assert lib.mfcc_hip_set_fbank(None, C.byref(p), L.ptr(w)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_fbank(None, None, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_fbank_bands(None, C.byref(got)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_fbank_i16(None, None, 0, 0, None, 0, C.byref(got)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_fbank_i16_dev(None, None, 0, 0, 0, 0, None, C.byref(got)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_fbank_ragged_i16_dev(None, None, None, 0, None, 0, None) == L.ERROR_INVALID_PARAM
    if torch.cuda.is_available():
        return                                              # tests/test_gpu_fbank.py has the handle
    # no CPU path: the handle cannot be made, so nothing computes -- as for the spectrum
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13).set_filterbank(w)
    assert e.value.code == L.ERROR_NOT_FOUND


# ---- fbank_plan.hpp through its driver
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("fbank_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "fbank_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


def both(drivers, lines):
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    a, b = (subprocess.run([d], input=text, capture_output=True, text=True, check=True).stdout.splitlines() for d in drivers)
    assert a == b and len(a) == len(lines)
    return a


def test_plan_kernel_choice(drivers):
    cases = [((512, 170, 512, 0), FUSED), ((512, 160, 400, 0), FUSED), ((512, 160, 160, 0), FUSED), ((512, 160, 512, 0), FUSED),
             ((512, 171, 512, 0), GENERIC), ((256, 85, 256, 0), GENERIC), ((1024, 341, 1024, 0), GENERIC),
             ((512, 170, 400, 0), GENERIC), ((512, 160, 159, 0), GENERIC), ((1024, 160, 400, 0), GENERIC),
             ((64, 21, 64, 0), GENERIC), ((512, 170, 512, 1), GENERIC), ((512, 160, 400, 1), GENERIC)]
    got = both(drivers, [("choose",) + c for c, _ in cases])
    for (c, name), line in zip(cases, got):
        k, n = line.split()
        assert n == name and int(k) == int(name == FUSED), (c, line)


def test_plan_parameters(drivers):
    got = both(drivers, [("scale", s) for s in (-1, 0, 1, 2, 3, 4)])
    assert [g.split()[0] for g in got] == ["0", "1", "1", "1", "1", "0"]
    for g, name in zip(got[1:5], ("energy", "log2", "ln", "log10")):
        assert np.float32(float(g.split()[1])) == np.float32(fr.SCALES[name])
    floors = ["0", "-0", "1e-10", "1.1920929e-07", "3e38", "-1e-30", "nan", "inf", "-inf", "1e39"]
    assert both(drivers, [("floor", v) for v in floors]) == ["1", "1", "1", "1", "1", "0", "0", "0", "0", "0"]
    assert both(drivers, [("bands", n) for n in (-1, 0, 1, 64, 65, 128, 129, 1 << 40)]) == ["0", "0", "1", "1", "1", "1", "0", "0"]


def _fmt(w):
    return [("%.9g" % v) for v in np.asarray(w, np.float32).ravel()]


def _matrices():
    sel = fr.selections()
    gap = np.zeros((3, 257), np.float32)                    # zeros inside a range, a band of one bin, -0.0 weights
    gap[0, [5, 9, 200]] = [0.5, 0.25, 2.0]
    gap[1, 256] = 1.0
    gap[2, :] = -0.0
    return [("htk80", fr.htk_weights(80)), ("htk23", fr.htk_weights(23, fmin=20.0)), ("htk128", fr.htk_weights(128)),
            ("edge", fr.edge_band()), ("dense", fr.dense_random()), ("gap", gap)] + [("sel%d" % i, w) for i, (_, w) in enumerate(sel)]


def test_plan_table_covers_every_weight_exactly_once(drivers):
    """Per matrix: the per-band bin ranges against NumPy's, and the packed weights put back into a matrix -- every
    non-zero weight lands on its own (band, bin) exactly once and nothing else is non-zero."""
    mats = _matrices()
    got = both(drivers, [["table", len(w), w.shape[1]] + _fmt(w) for _, w in mats])
    for (name, w), line in zip(mats, got):
        bad, bands, sizes, packed = line.split("|")
        assert int(bad) == -1, name
        bands = np.array(bands.split(), int).reshape(len(w), 4)
        first, count = fr.band_ranges(w)
        assert np.array_equal(bands[:, 0], first) and np.array_equal(bands[:, 1], count), name
        assert np.array_equal(bands[:, 3], fr.nnz(w)), name
        assert np.array_equal(bands[:, 2], np.concatenate([[0], np.cumsum(count)[:-1]])), name
        n_packed, wlds, blob = (int(v) for v in sizes.split())
        assert n_packed == count.sum() and wlds == int(n_packed <= 3072) and blob == -(-n_packed * 4 // 16) * 16 + 16 * len(w)
        packed = np.array(packed.split(), np.float32)
        assert len(packed) == n_packed and not np.signbit(packed).any()
        back = np.zeros_like(w)
        hits = np.zeros(w.shape, int)
        for j in range(len(w)):
            back[j, first[j]:first[j] + count[j]] = packed[bands[j, 2]:bands[j, 2] + count[j]]
            hits[j, first[j]:first[j] + count[j]] += 1
        assert np.array_equal(back, np.where(w != 0, w, np.float32(0.0))) and (hits[w != 0] == 1).all(), name
        assert first.min() >= 0 and (first + count).max() <= w.shape[1], name
    by_name = dict(zip((n for n, _ in mats), got))
    assert by_name["htk80"].split("|")[2].split()[1] == "1" and by_name["dense"].split("|")[2].split()[:2] == ["32896", "0"]


def test_plan_sets_cover_every_weight_exactly_once(drivers):
    """The MFMA form's set list per matrix: the block masks against a brute-force walk of the matrix, the sets counted in
    front of each block, and the operands read back -- every non-zero weight is held by exactly one slot of a listed set,
    no weight by two, no slot holds anything else, and hi + lo leaves at most 2^-17 of a weight."""
    mats = _matrices() + [("wide%d" % i, w) for i, (_, _, w) in enumerate(fr.wide_selections())]
    got = both(drivers, [["sets", len(w), w.shape[1]] + _fmt(w) for _, w in mats])
    for (name, w), line in zip(mats, got):
        ok, masks, first, sizes, cover, worst = line.split("|")
        assert int(ok) == 1, name
        masks = [int(v) for v in masks.split()]
        assert masks == fr.set_masks(w), name
        counts = [bin(v).count("1") for v in masks]
        assert [int(v) for v in first.split()] == [sum(counts[:b]) for b in range(8)], name
        assert [int(v) for v in sizes.split()] == [sum(counts), sum(counts) * 2 * 64 * 4], name
        assert [int(v) for v in cover.split()] == [int(fr.nnz(w).sum()), 0, 0], name
        assert float(worst) <= 2.0 ** -17, name
    by_name = dict(zip((n for n, _ in mats), got))
    assert by_name["dense"].split("|")[1].split() == ["511"] * 8                    # every pair listed
    assert by_name["edge"].split("|")[1].split() == ["257"] + ["0"] * 7            # bins 0 and 256: steps 0 and 8
    assert by_name["gap"].split("|")[3].split()[0] == "3"


def test_plan_refuses_bad_weights(drivers):
    w = fr.htk_weights(23, fmin=20.0)
    lines, want = [], []
    for at, v in ((0, "nan"), (100, "inf"), (257 * 22 + 256, "-1e-30"), (300, "-inf")):
        t = _fmt(w)
        t[at] = v
        lines.append(["table", 23, 257] + t)
        want.append(at)
    got = both(drivers, lines)
    assert [int(g.split("|")[0]) for g in got] == want


def test_plan_tile_elements(drivers):
    """The fused kernel's contraction loop at widths 1, 23, 80, 127, 128 x rows 1, 15, 16: every element of the tile's span
    exactly once, the frame of a thread is its lane & 15, and the 16 lanes of a quarter of a wave hold one band."""
    cases = [(rows, nb) for nb in (1, 23, 80, 127, 128) for rows in (1, 15, 16)]
    got = both(drivers, [("tile", r, nb) for r, nb in cases])
    for (rows, nb), line in zip(cases, got):
        count, stores = line.split(" |")
        assert int(count) == rows * nb <= 16 * 128
        tok = np.array(stores.split(), int).reshape(-1, 4)
        assert sorted(tok[:, 0].tolist()) == list(range(rows * nb))
        assert np.array_equal(tok[:, 2] * nb + tok[:, 3], tok[:, 0]) and (tok[:, 3] < nb).all() and (tok[:, 2] < rows).all()
        assert np.array_equal(tok[:, 2], tok[:, 1] % 16)
        for quarter in np.unique(tok[:, 1] // 16):
            steps = tok[tok[:, 1] // 16 == quarter]
            assert len({tuple(sorted(steps[steps[:, 1] == t, 3])) for t in np.unique(steps[:, 1])}) == 1


def test_plan_range_words(drivers):
    cases = [(0, 0), (0, 257), (256, 1), (17, 23), (0, 513), (512, 1)]
    got = both(drivers, [("range", f, c) for f, c in cases])
    assert [tuple(int(v) for v in g.split()[1:]) for g in got] == cases


def test_plan_limits(drivers):
    assert both(drivers, [("limits",)])[0].split() == ["128", "16", str(16 * 257), str(fr.K_WLDS), "8", "9"]
    assert 8 * fr.BLOCK == fr.MAX_BANDS and fr.STEPS * fr.STEP >= 257 > (fr.STEPS - 1) * fr.STEP
    q = (1 << 62) // 80
    lines = [("callfits", 9_600_000, 64, 80), ("callfits", 1 << 62, 1, 80), ("callfits", 1 << 40, 1 << 20, 128),
             ("callfits", 1 << 40, 0, 80), ("callfits", 100, 1 << 61, 80), ("callfits", (1 << 62) - 1, 1, 2)]
    assert both(drivers, lines) == ["1", "0", "0", "1", "0", "0"]
    lines = [("raggedfits", 1_600_000_000, 10_000, 80), ("raggedfits", 0, 0, 128), ("raggedfits", q - 20, 10, 80),
             ("raggedfits", q - 19, 10, 80), ("raggedfits", 1 << 61, 1, 1), ("raggedfits", 10, 1 << 61, 1)]
    assert both(drivers, lines) == ["1", "1", "1", "0", "0", "0"]


# ---- the reference, the bound and the restated arithmetic
def _banks(nfft):
    """The matrices of the bound's table at this nfft: HTK banks as the GPU tests use them, and a dense random one."""
    htk = {512: (80, 128, 23), 1024: (40,), 256: (23,), 64: (7,)}[nfft]
    out = [("htk%d" % n, fr.htk_weights(n, nfft, fmin=20.0 if n == 23 and nfft == 512 else 0.0)) for n in htk]
    return out + [("dense", fr.dense_random(128 if nfft == 512 else 16, nfft))]


@pytest.mark.parametrize("cfg", sr.CONFIGS, ids=lambda c: "%d_%d_%d" % c)
def test_nothing_is_set_aside_and_the_restatement_stays_within_half(wav_pcm, cfg):
    """On the GPU tests' inputs: no live element of a non-empty band is set aside by the log condition (``const_min`` and
    ``sine8`` go through the log at the framed shapes only, and through ENERGY everywhere), and the fp32 restatement of
    the kernels' arithmetic stays within B_E / 2 in ENERGY scale and within half the log bound."""
    nfft, hop, flen = cfg
    x = sr.input_list(nfft, hop, flen, wav_pcm)
    framed = flen != nfft
    log_kinds = [i for i, k in enumerate(sr.KINDS) if framed or k not in ("const_min", "sine8")]
    for pad_mode, halo in sr.FRAMINGS:
        p_ref = sr.reference(x, nfft, hop, flen, pad_mode=pad_mode, halo=halo)
        p32 = sr.restatement_f32(x, nfft, hop, flen, pad_mode=pad_mode, halo=halo)
        zero = sr.zero_frames(x, nfft, hop, flen, pad_mode, halo)
        for name, W in _banks(nfft):
            what = "%s %s halo %d %s" % (cfg, pad_mode, halo, name)
            e_ref, b_e = fr.energy_ref_and_bound(p_ref, W)
            fr.assert_not_blind(b_e, fr.pinned_mask(zero, W), what)
            e32 = fr.contract_f32(p32, W)
            worst = fr.check_energy(e32, e_ref, b_e, what, limit=0.5)
            live = b_e[log_kinds] > 0
            share = float((b_e[log_kinds][live] / e_ref[log_kinds][live]).max())
            assert share <= 0.25, (what, share)
            y = fr.scale_f32(e32[log_kinds], "log2", 0.0)
            worst_log, aside = fr.check_log(y, e_ref[log_kinds], b_e[log_kinds], "log2", 0.0, what, limit=0.5)
            assert aside == 0, (what, aside)
            print("%s: restatement worst |delta| / B_E %.3f, log %.3f; worst kept B_E / E_ref %.3g" % (what, worst, worst_log, share))
            if fr.form_of(W, FUSED) != "bf16" or nfft != 512:
                continue
            # the fused kernel's MFMA form: the bf16 hi / lo split restated, against that form's bound
            e_ref, b_e = fr.energy_ref_and_bound(p_ref, W, "bf16")
            fr.assert_not_blind(b_e, fr.pinned_mask(zero, W), what)
            e16 = fr.contract_bf16(p32, W)
            worst = fr.check_energy(e16, e_ref, b_e, what + " bf16", limit=0.5)
            y = fr.scale_f32(e16[log_kinds], "log2", 0.0)
            worst_log, aside = fr.check_log(y, e_ref[log_kinds], b_e[log_kinds], "log2", 0.0, what + " bf16", limit=0.5)
            assert aside == 0, (what, aside)
            print("%s: bf16 restatement worst |delta| / B_E %.3f, log %.3f" % (what, worst, worst_log))


def test_bf16_restatement_on_sparse_bands_stays_within_half(wav_pcm):
    """The bf16 form where a band holds one or two weights, so nothing averages the split's error out: the wide
    selection matrices and a single band, at the fused shapes."""
    for cfg in ((512, 170, 512), (512, 160, 400)):
        x = sr.input_list(*cfg, wav_pcm)
        p_ref = sr.reference(x, *cfg)
        p32 = sr.restatement_f32(x, *cfg)
        zero = sr.zero_frames(x, *cfg, "notebook", 0)
        for i, (_, _, W) in enumerate(fr.wide_selections()):
            e_ref, b_e = fr.energy_ref_and_bound(p_ref, W, "bf16")
            fr.assert_not_blind(b_e, fr.pinned_mask(zero, W))
            worst = fr.check_energy(fr.contract_bf16(p32, W), e_ref, b_e, "%s wide %d" % (cfg, i), limit=0.5)
            print("%s wide selection %d: bf16 restatement worst |delta| / B_E %.3f" % (cfg, i, worst))
    assert np.array_equal(fr.bf16_round(np.array([1.0, 1.00390625, 1.01171875, 3.0e38], np.float32)),
                          np.array([1.0, 1.0, 1.015625, 3.0040553e38], np.float32))


def test_floors_and_scales_on_the_restatement(wav_pcm):
    cfg = (512, 160, 400)
    x = sr.input_list(*cfg, wav_pcm)
    W = fr.htk_weights(128)
    e_ref, b_e = fr.reference_and_bound(x, W, *cfg)
    e32 = fr.restatement_f32(x, W, *cfg)
    assert (b_e == 0).any() and (b_e > 0).any()
    for scale, floor in (("log2", 0.0), ("ln", 1.1920929e-07), ("log10", 1e-10), ("log2", 1e6)):
        worst, aside = fr.check(fr.scale_f32(e32, scale, floor), e_ref, b_e, scale, floor, "%s floor %g" % (scale, floor), limit=0.5)
        assert aside == 0
    assert fr.check(e32, e_ref, b_e, "energy", 0.0, limit=0.5)[1] == 0


def test_checks_refuse_what_they_must():
    W = np.array([[0, 1.0, 1.0], [0, 0, 0]], np.float32)
    p_ref = np.array([[4.0, 4.0, 4.0], [0.0, 0.0, 0.0]])
    e_ref, b_e = fr.energy_ref_and_bound(p_ref, W)
    pinned = fr.pinned_mask(np.array([False, True]), W)
    fr.assert_not_blind(b_e, pinned)
    with pytest.raises(AssertionError):
        fr.assert_not_blind(b_e, fr.pinned_mask(np.array([False, False]), W[:1].repeat(2, 0)))
    good = e_ref.astype(np.float32)
    assert fr.check_energy(good, e_ref, b_e) == 0.0
    for bad, msg in [(np.where(e_ref > 0, np.nan, 0.0), "NaN"), (-good, "negative"), (good[:1], "shape"),
                     (good + np.float32(1e-30), "not \\+0.0"), (good * np.float32(1.01), "over")]:
        with pytest.raises(AssertionError, match=msg):
            fr.check_energy(np.asarray(bad, np.float32), e_ref, b_e)
    for scale, floor in (("log2", 0.0), ("ln", 1e-3)):
        y = fr.scale_f32(good, scale, floor)
        assert fr.check_log(y, e_ref, b_e, scale, floor)[0] < 1e-3
        with pytest.raises(AssertionError, match="over"):
            fr.check_log(y + np.float32(1e-3) * (b_e > 0), e_ref, b_e, scale, floor)
        with pytest.raises(AssertionError, match="NaN"):
            fr.check_log(np.where(b_e > 0, np.float32(np.nan), y), e_ref, b_e, scale, floor)
        with pytest.raises(AssertionError, match="shape"):
            fr.check_log(y[:1], e_ref, b_e, scale, floor)
        odd = y.copy()
        odd[1, 1] = 0.0
        with pytest.raises(AssertionError, match="different values"):
            fr.check_log(odd, e_ref, b_e, scale, floor)
    with pytest.raises(AssertionError, match="-inf"):
        fr.check_log(np.where(b_e > 0, fr.scale_f32(good, "log2", 0.0), np.float32(-100.0)), e_ref, b_e, "log2", 0.0)
    # an element whose bound passes a quarter of its energy is set aside, and counted
    assert fr.check_log(fr.scale_f32(good, "log2", 0.0), e_ref, np.where(b_e > 0, e_ref / 3.0, 0.0), "log2", 0.0)[1] == 1
