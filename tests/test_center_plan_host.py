"""mfcc_amd/csrc/center_plan.hpp (no HIP in it) through tests/center_plan_driver.cpp, plain and built with
-fsanitize=address,undefined: the geometry, the ragged table of a centred call -- the padded utterances abut from 0, an
utterance without a frame takes no room -- the host rule, and every source index the kernel may read.  The sanitized
program is a stand-alone binary with its own main: no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import center_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
MODE = {"reflect": 1, "zeros": 2}
IDS = ["%d_%d_%d" % f for f in cr.FRAMINGS]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("center_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "center_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


def run(driver, lines):
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[int(v) for v in ln.split()] for ln in out]


def both(drivers, lines):
    plain, san = (run(d, lines) for d in drivers)
    assert plain == san
    return plain


def corpora(nfft, hop, flen):
    base = cr.corpus_lengths(nfft, hop, flen)
    return [base, base[::-1], [5 * hop] * 3, []]


@pytest.mark.parametrize("nfft,hop,flen", cr.FRAMINGS, ids=IDS)
def test_geometry(drivers, nfft, hop, flen):
    ns = sorted(set(cr.lengths(nfft, hop, flen) + cr.corpus_lengths(nfft, hop, flen)))
    for mode in cr.MODES:
        got = both(drivers, [("geom", nfft, flen, hop, MODE[mode], n) for n in ns])
        for n, (pl, f, np_) in zip(ns, got):
            assert (pl, f, np_) == (cr.left_pad(nfft, flen), cr.frames(n, nfft, hop, flen, mode),
                                    cr.padded_len(n, nfft, hop, flen, mode)), (n, mode)


@pytest.mark.parametrize("first", [0, 7, (1 << 32) - 100])
@pytest.mark.parametrize("mode", cr.MODES)
@pytest.mark.parametrize("nfft,hop,flen", cr.FRAMINGS, ids=IDS)
def test_ragged_table(drivers, nfft, hop, flen, mode, first):
    lists = corpora(nfft, hop, flen)
    got = both(drivers, [("plan", nfft, flen, hop, MODE[mode], first, len(ls)) + tuple(ls) for ls in lists])
    for ls, row in zip(lists, got):
        n = len(ls)
        total, n_live, max_padded, stride8 = row[:4]
        own2, recs = row[4:4 + n + 1], np.asarray(row[4 + n + 1:], dtype=np.int64).reshape(n, 4)
        want = [cr.padded_len(v, nfft, hop, flen, mode) for v in ls]
        assert own2[0] == 0 and list(np.diff(own2)) == want                      # they abut, from 0
        assert total == own2[-1] == sum(want)
        assert n_live == sum(1 for v in want if v) and max_padded == max(want, default=0)
        assert stride8 % 8 == 0 and 0 <= stride8 - max_padded < 8
        src = first + np.concatenate([[0], np.cumsum(ls)])[:-1] if n else np.zeros(0)
        assert list(recs[:, 0]) == [int(v) for v in src] and list(recs[:, 1]) == ls
        assert list(recs[:, 2]) == own2[:-1] and list(recs[:, 3]) == want
        for v, w, a, b in zip(ls, want, own2[:-1], own2[1:]):                    # no frame, no room
            frames = cr.frames(v, nfft, hop, flen, mode)
            assert (b - a == 0) == (frames == 0) and (w == 0 or w == (frames - 1) * hop + flen)


@pytest.mark.parametrize("mode", cr.MODES)
@pytest.mark.parametrize("nfft,hop,flen", cr.FRAMINGS, ids=IDS)
def test_host_rule_and_source_indices(drivers, nfft, hop, flen, mode):
    ns = [n for n in cr.corpus_lengths(nfft, hop, flen) + cr.lengths(nfft, hop, flen)]
    rng = np.random.default_rng(3)
    xs = [rng.integers(-32768, 32768, n).astype(np.int16) for n in ns]
    got = both(drivers, [("run", nfft, flen, hop, MODE[mode], len(x)) + tuple(int(v) for v in x) for x in xs])
    src = both(drivers, [("src", nfft, flen, hop, MODE[mode], n) for n in ns])
    for n, x, p, s in zip(ns, xs, got, src):
        want = cr.pad(x, nfft, hop, flen, mode)
        assert p == [int(v) for v in want], (n, mode)
        # nothing outside the row is ever read: every source is an index of it, or the zero of the zeros mode
        assert len(s) == len(want) and all(-1 <= j < n for j in s)
        assert mode == "zeros" or all(j >= 0 for j in s)
        assert [0 if j < 0 else int(x[j]) for j in s] == p
