"""The filterbank stream bank (``mfcc_hip_bank_create_filterbank`` / ``MFCC.stream_bank(n, filterbank=True)``) as far as it
goes without a GPU: the export, its NULL arguments, the Python refusals that need no device, and the host plan at the row
widths only such a bank has, 65 .. 128 -- the delta kernels' tiles (mfcc_amd/csrc/bank_plan.hpp: tile_rows,
wide_tile_rows) and the layouts and records of pushes, flushes and resets, held to the restatement and the invariants of
tests/test_bank_plan_host.py.  tests/fbank_bank_plan_driver.cpp prints them, built plain and, as a program of its own,
with -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import test_bank_plan_host as bp

ROOT = bp.ROOT
NARROW_LDS, WIDE_LDS, NARROW_WIDTH = 4096, 8192, 64   # floats of LDS of the two delta kernels; the widest narrow row


def tile(lds, W, order, window):
    """The delta kernels' tile, restated: a tile of g emitted rows holds (g + 2L) W static floats, L = order * window,
    and at order 2 (g + 2 window) W delta floats too."""
    per, L = lds // W, order * window
    return per - 2 * L if order == 1 else (per - 2 * L - 2 * window) // 2


# kind -> the settings of bp.KINDS at the widths and tiles of a filterbank bank: g is what the tile function gives for
# the bank's order x window (deltas 1 x 8 at 65, 2 x 2 at 80, 2 x 8 at 128: g = 8, the LDS edge), S a CMVN run
WIDE_KINDS = {
    "plain_80":           dict(W=80, elem=4, S=0, L=0, order=0, g=0, pcen=0),
    "plain_128":          dict(W=128, elem=4, S=0, L=0, order=0, g=0, pcen=0),
    "cmvn_128":           dict(W=128, elem=4, S=32, L=0, order=0, g=0, pcen=0),
    "delta1x8_65":        dict(W=65, elem=4, S=0, L=8, order=1, g=tile(WIDE_LDS, 65, 1, 8), pcen=0),
    "delta2x2_80":        dict(W=80, elem=4, S=0, L=4, order=2, g=tile(WIDE_LDS, 80, 2, 2), pcen=0),
    "pcen_80":            dict(W=80, elem=4, S=0, L=0, order=0, g=0, pcen=1),
    "pcen_cmvn_delta2x8_128": dict(W=128, elem=4, S=32, L=16, order=2, g=tile(WIDE_LDS, 128, 2, 8), pcen=1),
    "cmvn_delta2x8_65":   dict(W=65, elem=4, S=8, L=16, order=2, g=tile(WIDE_LDS, 65, 2, 8), pcen=0),
}
GEOMETRIES = [(512, 170), (400, 160), (128, 1)]       # the last: a frame per sample, pushes of many tiles and runs


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("fbank_bank_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", bp.CSRC, "-I", os.path.join(ROOT, "tests"),
            os.path.join(ROOT, "tests", "fbank_bank_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


@pytest.fixture(scope="module")
def scheduled():
    runs = []
    for gi, geo in enumerate(GEOMETRIES):
        for ki, (name, k) in enumerate(WIDE_KINDS.items()):
            bank = bp.Bank(geo, k)
            rng = np.random.default_rng(geo[0] * 1000 + geo[1] * 10 + ki + 77)
            runs.append((name, bank, bp.schedule(bank, rng, emit=(gi + ki) % 2)))
    text = "".join(" ".join(str(v) for v in [c[0]] + c[1]) + "\n" for _, _, cases in runs for c in cases)
    return runs, text


# ------------------------------------------------------------------------------------------------ the export

def test_export_is_declared_present_and_typed():
    from mfcc_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "mfcc_hip.h")).read()
    decl = re.search(r"int\s+mfcc_hip_bank_create_filterbank\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert decl, "include/mfcc_hip.h does not declare mfcc_hip_bank_create_filterbank"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["mfcc_hip_handle *h", "size_t n_streams", "const mfcc_hip_pcen *p", "int normalize", "int normalize_window",
                    "int delta_order", "int delta_window", "mfcc_hip_bank **out"]
    assert hasattr(C.CDLL(L.LIB_PATH), "mfcc_hip_bank_create_filterbank")
    assert "mfcc_hip_bank_create_filterbank" in L.SYMBOLS
    assert L.load().mfcc_hip_abi_version() == 2                   # an added export: the version stays


def test_null_arguments_are_invalid():
    from mfcc_amd import _lib as L
    lib = L.load()
    out = C.c_void_p(1234)
    ok = L.Pcen()
    assert lib.mfcc_hip_pcen_defaults(C.byref(ok)) == 0
    for p in (None, C.byref(ok)):
        assert lib.mfcc_hip_bank_create_filterbank(None, 2, p, 0, 0, 0, 2, C.byref(out)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_bank_create_filterbank(None, 2, p, 2, 40, 2, 8, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_bank_row_width(None) == 0 and lib.mfcc_hip_bank_lag(None) == 0


def test_python_refusals_that_need_no_device():
    import mfcc_amd
    from mfcc_amd import _lib as L
    handle = types.SimpleNamespace(_lib=L.load(), _h=None, samplerate=16000, hop=160)     # nothing of it is reached
    bank = lambda **kw: mfcc_amd.MfccStreamBank(handle, 2, **kw)                          # noqa: E731
    with pytest.raises(ValueError, match="float only"):
        bank(fixed=True, filterbank=True)
    with pytest.raises(ValueError, match="float only"):
        bank(fixed=True, filterbank=True, normalize="mean", normalize_window=5)
    for bad in (dict(deltas=3), dict(deltas=-1), dict(deltas=1.0), dict(deltas=1, delta_window=0), dict(deltas=2, delta_window=9),
                dict(normalize="meanvar"), dict(normalize="meanvar", normalize_window=0),
                dict(normalize="mean", normalize_window=L.MAX_NORMALIZE_WINDOW + 1), dict(normalize="mean", normalize_window=2.5),
                dict(normalize="median", normalize_window=5), dict(pcen=dict(s=0))):
        with pytest.raises(ValueError):
            bank(filterbank=True, **bad)
    with pytest.raises(ValueError):
        mfcc_amd.MfccStreamBank(handle, 0, filterbank=True)
    sig = __import__("inspect").signature(mfcc_amd.MFCC.stream_bank).parameters["filterbank"]
    assert sig.kind is sig.KEYWORD_ONLY and sig.default is False


# ------------------------------------------------------------------------------------------------ the tiles

def test_tiles_of_the_delta_kernels(drivers):
    lines = subprocess.run([drivers[0], "tiles"], capture_output=True, text=True, check=True).stdout.splitlines()
    san = subprocess.run([drivers[1], "tiles"], capture_output=True, text=True)
    assert san.returncode == 0 and san.stdout.splitlines() == lines, san.stderr[-2000:]
    assert [int(v) for v in lines[0].split()] == [NARROW_LDS, WIDE_LDS, NARROW_WIDTH]
    rows = {tuple(v[:3]): v[3:] for v in ([int(x) for x in ln.split()] for ln in lines[1:])}
    assert len(rows) == 128 * 2 * 8
    for (W, order, window), (narrow, wide, chosen) in rows.items():
        L = order * window
        if W <= NARROW_WIDTH:
            # today's formula, written out: per = 4096 / W, per - 2L or (per - 2L - 2 Nd) / 2
            per = 4096 // W
            assert narrow == (per - 2 * L if order == 1 else (per - 2 * L - 2 * window) // 2), (W, order, window)
            assert chosen == narrow and narrow >= 8
        else:
            g = wide
            assert chosen == wide == tile(WIDE_LDS, W, order, window) and g >= 8, (W, order, window, g)
            floats = (g + 2 * L) * W + ((g + 2 * window) * W if order == 2 else 0)
            assert floats <= WIDE_LDS, (W, order, window, g, floats)
            assert narrow < g                                    # ... which the narrow tile does not offer
    assert rows[(128, 2, 8)][1] == 8 and rows[(128, 2, 8)][0] < 0            # the edge the wide tile exists for


# ------------------------------------------------------------------------------------------------ the plan

def test_wide_layouts_and_records_hold_the_invariants(drivers, scheduled):
    runs, text = scheduled
    lines = subprocess.run([drivers[0]], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == sum(len(cases) for _, _, cases in runs)
    cover = dict.fromkeys(["lockstep", "mixed", "run_before_seen", "runs3", "tiles2", "flush_held_lag", "reset", "nothing"], 0)
    n = bp.N_STREAMS
    it = iter(lines)
    for name, bank, cases in runs:
        k = bank.k
        for kind, head, state, arg, want in cases:
            st = (state[:n], state[n:2 * n], state[2 * n:])
            push = kind == "push"
            rc, fo, got = bp.parse(next(it), n + 1 if push else len(arg[2]) + 1, push)
            assert rc == bp.OK, (name, head)
            w_fo, w_t, w_lay = (want[0], want[4], want[5]) if push else want
            assert fo == w_fo, (name, head)
            lay = got["layout"]
            if w_lay is None:
                assert lay["n_rec"] == 0 and not got["block"]
                cover["nothing"] += 1
                continue
            assert lay == w_lay, (name, head, lay, w_lay)
            assert bp.BLANK not in got["block"]                              # tables without gaps
            t = bp.tables_of(lay, got["block"])
            assert t == w_t, (name, head)
            bp.check_invariants(bank, lay, t, fo, st, push, cover)           # every returned row written exactly once
            # raw_off / stat_off / out_bytes follow from W
            rows_bytes = lay["n_active"] * lay["nfmax"] * k["W"] * 4
            assert lay["raw_off"] == bp.up256(lay["desc_ll"] * 8)
            if bank.online:
                assert lay["stat_off"] == lay["raw_off"] + bp.up256(rows_bytes)
                assert lay["out_bytes"] == lay["stat_off"] + bp.up256(rows_bytes) + 64
            else:
                assert lay["stat_off"] == lay["raw_off"]
                assert lay["out_bytes"] == lay["raw_off"] + (0 if lay["direct"] else rows_bytes) + 64
            if push:
                cover["lockstep"] += lay["lockstep"] and lay["n_active"] > 1
                cover["mixed"] += lay["n_active"] > 1 and not lay["lockstep"]
            else:
                cover["reset"] += not arg[1]
                cover["flush_held_lag"] += bool(arg[1] and k["L"] and any(st[2][u] == k["L"] for u in arg[2]))
    assert all(cover.values()), cover


def test_driver_runs_clean_under_the_sanitizers(drivers, scheduled):
    text = scheduled[1]
    plain = subprocess.run([drivers[0]], input=text, capture_output=True, text=True, check=True)
    san = subprocess.run([drivers[1]], input=text, capture_output=True, text=True)
    assert san.returncode == 0, san.stderr[-2000:]
    assert san.stdout == plain.stdout
