"""The sample rate -> kernel instantiation map, on the CPU.

``sample_rate`` is a free integer, and the mel matrix built from it decides which instantiation of each fused kernel
runs and whether a fused kernel runs at all.  The two host table drivers (tests/fused512_tables_driver.cpp,
tests/fused1024_tables_driver.cpp) are compiled as tests/test_fused512_tables_host.py and
tests/test_fused1024_tables_host.py compile them and asked for every rate of ``RATES``; only their ``ok``,
``needs_dc_exact``, variant / schedule and ``set_mask`` answers are read, no hashes, and the golden files are not
touched.  The tables below are what this module pins; tests/test_gpu_sample_rates.py imports them, so a change that
moves a rate to another instantiation fails here first and the GPU tests never run silently on the wrong code.

Empty filters (rows of the mel matrix whose weights are all zero) are counted on the float64 oracle's own banks,
``oracle.mfcc_float.get_filters`` and ``melbank_ref.htk_matrix``.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import melbank_ref as mr
from oracle import mfcc_float as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")

# 1000, 4000 and 24000: ordinary rates below 48 kHz that no other test uses; they pin the map at its low end
RATES = [1000, 4000, 7999, 12000, 16001, 24000, 37800, 64000, 88200, 96000, 176400, 192000, 384000]

# ---- 512 points: mfcc_fused::build_tables<false> (sparse) / <true> (dense) and needs_dc_exact
SPARSE_512 = {12000, 16001}                                  # rates the sparse 512 / 32 tables accept; dense elsewhere
DC_EXACT = {32: {r for r in RATES if r >= 64000},            # n_mel -> rates whose bank has weight on the DC bin
            16: {r for r in RATES if r >= 176400}}
# ---- 1024 / 40: mfcc_fused1024::build_tables (bf16-split set lists) and mfcc_fused1024_f32::build_tables (schedules)
BF16_1024 = {1000: 0, 4000: 0, 7999: 0, 12000: 0, 16001: 0, 24000: 0, 64000: 1}     # rate -> set list; others refused
F32_1024 = {7999: 1, 12000: 2, 16001: 0}                                             # rate -> schedule; others refused
GENERIC_1024 = [r for r in RATES if r not in BF16_1024]      # 37800 (no DC weight: no set list fits) and from 88200 up
DC_1024 = {r for r in RATES if r >= 88200}                   # the generic kernel's double-precision DC sum at 1024
# ---- empty filters of the notebook bank: (nfft, n_mel) -> rate -> bands; rates not named have none
EMPTY = {
    (512, 32): {88200: [1], 96000: [1], 176400: [0, 2, 4], 192000: [0, 2, 4], 384000: [0, 1, 2, 4, 6]},
    (512, 16): {384000: [0]},
    (1024, 40): {176400: [1], 192000: [1, 4], 384000: [0, 1, 3, 6]},
}
# ---- HTK banks at 400 / 160 / 512: id -> (n_mel, fmin, fmax (0: Nyquist), rate, set mask, empty bands)
HTK_BANKS = {
    "vggish_48k": (64, 125.0, 7500.0, 48000, 85, [0, 5, 10]),
    "htk40_96k": (40, 20.0, 0.0, 96000, 53, [0]),
    "htk40_192k": (40, 0.0, 0.0, 192000, 53, [0, 1, 4]),
}


def empty_bands(nfft, n_mel, rate):
    return list(EMPTY.get((nfft, n_mel), {}).get(rate, []))


def _compile(tmp_path_factory, name):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp(name) / "driver"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(ROOT, "tests", name + "_driver.cpp")], check=True)
    return str(exe)


def _ask(driver, cases):
    lines = subprocess.run([driver], input="\n".join(cases) + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    return [line.split() for line in lines]


@pytest.fixture(scope="module")
def driver512(tmp_path_factory):
    return _compile(tmp_path_factory, "fused512_tables")


@pytest.fixture(scope="module")
def driver1024(tmp_path_factory):
    return _compile(tmp_path_factory, "fused1024_tables")


@pytest.mark.parametrize("frame_len", [0, 400])
def test_512_sparse_dense_and_dc_exact_by_rate(driver512, frame_len):
    """nb dense rate n_mel n_cep frame_len lifter -> ok needs_dc_exact ...; the handle takes the sparse tables where they
    are accepted and the bank has no DC weight, the dense ones (with the exact-DC path where needed) elsewhere."""
    sparse = _ask(driver512, ["nb 0 %d 32 13 %d 0" % (r, frame_len) for r in RATES])
    dense = _ask(driver512, ["nb 1 %d 32 32 %d 0" % (r, frame_len) for r in RATES])
    dense16 = _ask(driver512, ["nb 1 %d 16 16 %d 0" % (r, frame_len) for r in RATES])
    sparse16 = _ask(driver512, ["nb 0 %d 16 16 %d 0" % (r, frame_len) for r in RATES])
    assert {r for r, a in zip(RATES, sparse) if a[0] == "1"} == SPARSE_512
    assert not any(a[0] == "1" for a in sparse16)              # 16 filters always run on the dense schedule
    assert all(a[0] == "1" for a in dense) and all(a[0] == "1" for a in dense16)      # ... which takes every rate
    assert {r for r, a in zip(RATES, dense) if a[1] == "1"} == DC_EXACT[32]
    assert {r for r, a in zip(RATES, sparse) if a[1] == "1"} == DC_EXACT[32]
    assert {r for r, a in zip(RATES, dense16) if a[1] == "1"} == DC_EXACT[16]
    assert not SPARSE_512 & DC_EXACT[32]


def test_dc_exact_is_weight_on_the_dc_bin():
    """needs_dc_exact restated on the oracle's bank: some filter has weight on bin 0."""
    for n_mel in (32, 16):
        assert {r for r in RATES if (mf.mel_filterbank(512, n_mel, r)[:, 0] != 0).any()} == DC_EXACT[n_mel]
    assert {r for r in RATES if (mf.mel_filterbank(1024, 40, r)[:, 0] != 0).any()} == DC_1024


def test_1024_builders_by_rate(driver1024):
    """bf / f32 rate n_cep lifter power_scale -> ok variant-or-schedule ...; the same answer for 13 and 40 cepstra."""
    for n_cep in (13, 40):
        bf = _ask(driver1024, ["bf %d %d 0 1024" % (r, n_cep) for r in RATES])
        f32 = _ask(driver1024, ["f32 %d %d 0 1024" % (r, n_cep) for r in RATES])
        assert {r: int(a[1]) for r, a in zip(RATES, bf) if a[0] == "1"} == BF16_1024
        assert {r: int(a[1]) for r, a in zip(RATES, f32) if a[0] == "1"} == F32_1024
        assert all(a[:3] == ["0", "-1", "0"] for r, a in zip(RATES, bf) if r not in BF16_1024)
        assert all(a[:3] == ["0", "-1", "0"] for r, a in zip(RATES, f32) if r not in F32_1024)
    assert GENERIC_1024 == [37800, 88200, 96000, 176400, 192000, 384000]
    assert 37800 not in DC_1024 and set(GENERIC_1024) - {37800} == DC_1024      # every fused builder refuses DC weight
    assert set(BF16_1024.values()) == {0, 1} and sorted(F32_1024.values()) == [0, 1, 2]


def test_bank_builder_accepts_the_banks_with_empty_filters(driver512):
    """mb rate n_mel n_cep frame_len low high lifter -> ok bytes hash set_mask, for 13 cepstra and for log-mel rows."""
    for name, (n_mel, lo, hi, rate, mask, _) in HTK_BANKS.items():
        for n_cep in (13, 1):
            ok, _, _, got = _ask(driver512, ["mb %d %d %d 400 %g %g 0" % (rate, n_mel, n_cep, lo, hi)])[0]
            assert ok == "1" and int(got) == mask, (name, n_cep, ok, got)
        assert mask < 1 << (2 * ((n_mel + 15) // 16)), name


def test_empty_filter_counts():
    for (nfft, n_mel), by_rate in EMPTY.items():
        for r in RATES:
            points, _ = mf.get_filter_points(0, r / 2, n_mel, nfft, sample_rate=r)
            W = mf.get_filters(points, nfft)
            assert np.flatnonzero(~(W != 0).any(axis=1)).tolist() == by_rate.get(r, []), (nfft, n_mel, r)
            assert np.array_equal(W, mf.mel_filterbank(nfft, n_mel, r))
    # the counts of the survey this map came from
    assert [len(empty_bands(512, 32, r)) for r in (64000, 88200, 96000, 176400, 192000, 384000)] == [0, 1, 1, 3, 3, 5]
    assert [len(empty_bands(512, 16, r)) for r in (192000, 384000)] == [0, 1]
    assert [len(empty_bands(1024, 40, r)) for r in (96000, 176400, 192000)] == [0, 1, 2]
    for name, (n_mel, lo, hi, rate, _, empty) in HTK_BANKS.items():
        W = mr.htk_matrix(512, n_mel, rate, lo, hi or None)
        assert np.flatnonzero(~(W != 0).any(axis=1)).tolist() == empty, name
        assert not (W[:, 0] != 0).any(), name                  # an HTK bank has no weight on bin 0, low = 0 included
    assert [len(b[5]) for b in HTK_BANKS.values()] == [3, 1, 3]
