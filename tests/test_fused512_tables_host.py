"""The table blobs of the four-wave fused 512 kernels, on the CPU: a few lines of C++ (tests/fused512_tables_driver.cpp)
call mfcc_fused::build_tables<false/true> + mfcc_fused160::set_window and mfcc_fused160mb::build_tables and print the
size and an FNV-1a hash of every blob (and the bank form's set mask).  tests/golden/fused512_tables.json holds what the
builders gave before they shared their window, twiddle, column-16 and bf16 helpers and their blob offsets: the blobs are
kernel arguments, so they must stay byte for byte what they were.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

import kernel_families as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused512_tables.json")

# nb dense sample_rate n_mel n_cep frame_len lifter (frame_len 0: the hop-170 kernel's own window, no set_window)
NOTEBOOK = [
    "nb 0 16000 32 13 0 0", "nb 0 16000 32 13 400 0", "nb 0 16000 32 13 160 0", "nb 0 16000 32 13 511 0",   # banded
    "nb 0 16000 32 32 400 0", "nb 0 16000 32 16 400 22", "nb 1 16000 32 13 400 0",
    "nb 0 8000 32 13 400 0",                                 # refused: 8 kHz does not fit the banded schedule
    "nb 1 8000 32 13 0 0", "nb 1 8000 32 13 400 0", "nb 1 8000 32 32 511 0",        # dense, no filter on bin 0
    "nb 1 48000 32 13 0 0", "nb 1 48000 32 13 400 0", "nb 1 48000 32 16 160 0", "nb 1 44100 32 32 511 22",  # ... with
    "nb 0 16000 16 13 400 0",                                # refused: 16 filters run on the dense schedule
    "nb 1 16000 16 13 400 0", "nb 1 16000 16 16 0 0", "nb 1 48000 16 13 511 0",
]
# mb sample_rate n_mel n_cep frame_len low high lifter (high 0: sample_rate / 2)
BANK = [
    "mb 16000 23 13 400 20 0 0", "mb 16000 40 13 400 20 0 0", "mb 16000 40 16 160 20 0 22", "mb 16000 40 32 400 20 0 0",
    "mb 16000 64 13 400 125 7500 0", "mb 16000 64 16 511 125 7500 0", "mb 16000 64 32 400 20 0 0",
    "mb 16000 64 13 400 0 0 0",                              # low 0: the first filter still has no weight on bin 0
    "mb 16000 16 13 400 20 0 0", "mb 16000 1 1 400 20 0 0", "mb 8000 40 13 400 0 0 0", "mb 48000 23 13 400 20 0 0",
]
CASES = NOTEBOOK + BANK


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("fused512_tables") / "driver"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(ROOT, "tests", "fused512_tables_driver.cpp")], check=True)
    return str(exe)


def test_blobs_are_byte_for_byte_what_they_were(driver):
    golden = json.load(open(GOLDEN))
    assert list(golden) == CASES                       # the fixture lists exactly these cases, in this order
    lines = subprocess.run([driver], input="\n".join(CASES) + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    assert len(lines) == len(CASES)
    for case, line in zip(CASES, lines):
        assert line == golden[case], case


def test_set_masks_of_the_banks_the_gpu_tests_run(driver):
    """kernel_families.MASK_BANKS, the bank list of tests/test_gpu_melbank.py: every bank is accepted and gives the set
    mask the list claims, and together they reach the masks the golden cases do not.  Not part of the golden file."""
    cases = ["mb %d %d %d 400 %g %g 0" % (rate, n_mel, min(13, n_mel), lo, hi)
             for n_mel, lo, hi, rate, _ in kf.MASK_BANKS.values()]
    lines = subprocess.run([driver], input="\n".join(cases) + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for (name, bank), line in zip(kf.MASK_BANKS.items(), lines):
        ok, _, _, mask = line.split()
        assert ok == "1" and int(mask) == bank[4], (name, line)
        n_mel = bank[0]
        assert bank[4] < 1 << (2 * ((n_mel + 15) // 16)), name                          # pairs of the blocks present only
    golden = json.load(open(GOLDEN))
    seen = {int(golden[c].split()[3]) for c in BANK}
    assert {b[4] for b in kf.MASK_BANKS.values()} - seen == {0, 1, 2, 10, 11, 21, 42, 53, 170, 181}


def test_the_cases_cover_what_they_claim():
    """The fixture itself: refusals where the handle falls to the dense schedule, the DC path at 44.1 / 48 kHz only,
    blob sizes by schedule, set masks that grow with the bank."""
    golden = json.load(open(GOLDEN))
    nb = {c: golden[c].split() for c in NOTEBOOK}
    assert [c for c, g in nb.items() if g[0] == "0"] == ["nb 0 8000 32 13 400 0", "nb 0 16000 16 13 400 0"]
    for c, g in nb.items():
        dense, rate, n_mel = c.split()[1:4]
        assert g[1] == ("1" if rate in ("44100", "48000") and n_mel == "32" else "0"), c     # 16 wider filters: none on bin 0
        if g[0] == "1":
            assert g[2] == ("146648" if dense == "1" else "114904"), c
    assert len({g[3] for g in nb.values() if g[0] == "1"}) == len(NOTEBOOK) - 2        # no two cases share a blob
    mb = {c: golden[c].split() for c in BANK}
    assert all(g[0] == "1" for g in mb.values())
    assert len({g[2] for g in mb.values()}) == len(BANK)
    for c, g in mb.items():
        n_mel, mask = int(c.split()[2]), int(g[3])
        assert 0 < mask < 1 << (2 * ((n_mel + 15) // 16)), c                           # pairs of the blocks present only
        assert int(g[1]) == 4 * (512 + 512 + 4 * 16 * 64) + 4 * bin(mask).count("1") * 2 * 64 * 16, c
