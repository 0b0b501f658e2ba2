"""The table blobs of the four fused 1024 kernels, on the CPU: a few lines of C++ (tests/fused1024_tables_driver.cpp) call
mfcc_fused1024::build_tables (the bf16-split set lists) and mfcc_fused1024_f32::build_tables (one fp32 list per rate) and
print accepted / refused, the chosen variant or schedule, the size and an FNV-1a hash of every blob.
tests/golden/fused1024_tables.json was generated at the parent commit of the change that gave the two builders one
function each for the window rows, the twiddles, the DCT rows and the column-16 DFT rows, before either builder was
touched: the blobs are kernel arguments, so they must stay byte for byte what they were.  The GPU tests
(tests/test_gpu_fused1024_forms.py) rely on the rate -> instantiation map that the third test here proves.  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused1024_tables.json")

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000]
# sample_rate n_cep lifter power_scale, for both builders.  n_cep 1 appears with one lifter per rate only: the lifter's
# weight on coefficient 0 is 1, so the two blobs would be the same bytes
SHAPES = ["%d 13 0 1024" % r for r in RATES] + [
    "16000 1 0 1024", "16000 16 0 1024", "16000 17 0 1024", "16000 32 0 1024", "16000 40 0 1024",       # M tiles of the DCT
    "16000 13 22 1024", "16000 40 22 1024", "32000 32 22 1024", "48000 40 22 1024", "11025 1 22 1024",  # lifter
    "16000 13 0 1", "8000 17 22 1", "44100 16 0 1", "22050 32 0 1",                                     # power scale
    "32000 40 0 1024", "44100 17 0 1024",
]
CASES = ["%s %s" % (kind, s) for kind in ("bf", "f32") for s in SHAPES]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("fused1024_tables") / "driver"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(ROOT, "tests", "fused1024_tables_driver.cpp")], check=True)
    return str(exe)


def test_blobs_are_byte_for_byte_what_they_were(driver):
    golden = json.load(open(GOLDEN))
    assert list(golden) == CASES                       # the fixture lists exactly these cases, in this order
    lines = subprocess.run([driver], input="\n".join(CASES) + "\n", capture_output=True, text=True,
                           check=True).stdout.splitlines()
    assert len(lines) == len(CASES)
    for case, line in zip(CASES, lines):
        assert line == golden[case], case


def test_the_cases_hold_the_values_they_are_to_cover():
    for kind in ("bf", "f32"):
        mine = [c.split() for c in CASES if c.split()[0] == kind]
        assert {int(c[1]) for c in mine} == set(RATES)
        assert {int(c[2]) for c in mine} == {1, 13, 16, 17, 32, 40}
        assert {c[3] for c in mine} == {"0", "22"} and {c[4] for c in mine} == {"1024", "1"}


def test_the_cases_cover_what_they_claim():
    """The fixture itself: the bf16 builder takes every rate and reaches its three set lists, the fp32 builder takes the
    five lower rates on five different lists and refuses 44.1 and 48 kHz (weight on the DC bin), blob sizes follow the
    list, and no two accepted cases share a blob."""
    golden = {c: golden_line.split() for c, golden_line in json.load(open(GOLDEN)).items()}
    rate_of = lambda c: int(c.split()[1])
    bf = {c: g for c, g in golden.items() if c.startswith("bf ")}
    f32 = {c: g for c, g in golden.items() if c.startswith("f32 ")}
    assert all(g[0] == "1" for g in bf.values())
    variant = {}
    for c, g in bf.items():
        assert variant.setdefault(rate_of(c), g[1]) == g[1], c                  # a rate's list does not depend on the rest
        n_sets = 5 if g[1] == "2" else 4
        assert int(g[2]) == 4 * (32 * 32 + 32 * 16 * 2 + 3 * 14 * 64 + 2 * 12 * 64) + 2 * 4 * 8 * n_sets * 2 * 256, c
    assert variant == {8000: "0", 11025: "0", 16000: "0", 22050: "0", 32000: "2", 44100: "1", 48000: "1"}
    assert set(variant.values()) == {"0", "1", "2"}
    sched = {}
    for c, g in f32.items():
        if rate_of(c) in (44100, 48000):
            assert g[:3] == ["0", "-1", "0"], c
            continue
        assert g[0] == "1", c
        assert sched.setdefault(rate_of(c), g[1]) == g[1], c
        assert int(g[2]) == 4 * (32 * 32 + 32 * 16 * 2 + 8 * 19 * 64 + 5 * 12 * 64), c
    assert sorted(sched) == RATES[:5] and len(set(sched.values())) == 5
    accepted = [g[3] for g in golden.values() if g[0] == "1"]
    assert len(set(accepted)) == len(accepted)
