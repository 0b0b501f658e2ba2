"""The filterbank post-passes (``mfcc_hip_set_filterbank_post`` / ``MFCC.set_filterbank(..., normalize=, deltas=, pcen=)``) as
far as they go without a GPU: the exports and the struct, the NULL handle, the Python refusals that need no device, and the
host plan of the wide kernels -- mfcc_amd/csrc/post_plan.hpp's tiles and grid and seg_plan.hpp's scratch layouts at the
widths 65 .. 128, through tests/post_wide_plan_driver.cpp, built plain and, as a program of its own, with
-fsanitize=address,undefined.  (A field of the struct can only be refused on a handle, and a handle needs a device:
tests/test_gpu_fbank_post.py has those refusals.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mfcc_amd
from mfcc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
NAMES = ["mfcc_hip_set_filterbank_post", "mfcc_hip_filterbank_row_width"]
NARROW_LDS, NORM_TILE = 4096, 8192


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("post_wide_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "post_wide_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


def run_both(drivers, args, text=""):
    outs = [subprocess.run([d] + args, input=text, capture_output=True, text=True, check=True).stdout for d in drivers]
    assert outs[0] == outs[1]
    return outs[0]


@pytest.fixture(scope="module")
def tiles(drivers):
    lines = run_both(drivers, ["tiles"]).splitlines()
    head = [int(v) for v in lines[0].split()]
    rows = np.array([[int(v) for v in ln.split()] for ln in lines[1:]])
    assert rows.shape == (128 * 2 * 8, 9)
    return head, rows


# ------------------------------------------------------------------------------------------------ exports and struct

def test_exports_are_declared_present_and_typed():
    lib = L.load()
    assert lib.mfcc_hip_abi_version() == 2                          # added exports: the version stays
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfcc_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+mfcc_hip_set_filterbank_post\(mfcc_hip_handle \*h, const mfcc_hip_filterbank_post \*p\s*\);", src)
    assert re.search(r"size_t\s+mfcc_hip_filterbank_row_width\(const mfcc_hip_handle \*h\);", src)
    for n in NAMES:
        assert n in L.SYMBOLS and hasattr(C.CDLL(L.LIB_PATH), n) and "fbank" not in n
    # struct mfcc_hip_filterbank_post: eight words, a mfcc_hip_pcen, four reserved words
    assert C.sizeof(L.Pcen) == 36 and C.sizeof(L.FilterbankPost) == 32 + 36 + 16
    names = [f[0] for f in L.FilterbankPost._fields_]
    assert names == ["struct_size", "normalize", "normalize_window", "normalize_min_window", "normalize_center", "delta_order",
                     "delta_window", "pcen_on", "pcen", "reserved"]
    body = re.search(r"typedef struct mfcc_hip_filterbank_post \{(.*?)\} mfcc_hip_filterbank_post;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == names
    assert L.FilterbankPost.pcen.offset == 32 and L.FilterbankPost.reserved.offset == 68


def test_entries_without_a_handle():
    lib = L.load()
    q = L.FilterbankPost(struct_size=C.sizeof(L.FilterbankPost), delta_window=2, normalize_min_window=1, normalize_center=1)
    assert lib.mfcc_hip_set_filterbank_post(None, C.byref(q)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_set_filterbank_post(None, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_filterbank_row_width(None) == 0


def test_python_keyword_refusals_need_no_device():
    m = mfcc_amd.MFCC.__new__(mfcc_amd.MFCC)                        # no handle: every refusal comes before the library is asked
    m.nfft, m.samplerate, m.hop = 512, 16000.0, 160
    w = np.ones((80, 257), np.float32)
    bad = [dict(normalize="cmvn"), dict(normalize=1), dict(normalize="mean", normalize_window=0),
           dict(normalize="mean", normalize_window=16385), dict(normalize="mean", normalize_window=40, normalize_min_window=41),
           dict(normalize="mean", normalize_window=40, normalize_min_window=0), dict(normalize="mean", normalize_window=2.5),
           dict(normalize_center=2), dict(deltas=3), dict(deltas=-1), dict(deltas=True), dict(deltas=1, delta_window=0),
           dict(deltas=1, delta_window=9), dict(delta_window=9), dict(pcen="yes"), dict(pcen=dict(s=0.0)), dict(pcen=dict(s=1.5)),
           dict(pcen=dict(alpha=2.0)), dict(pcen=dict(r=0.0)), dict(pcen=dict(eps=0.0)), dict(pcen=dict(gain=1.0)),
           dict(pcen=dict(s=0.1, time_constant=0.4)), dict(pcen=dict(time_constant=-1.0))]
    for kw in bad:
        with pytest.raises(ValueError):
            m.set_filterbank(w, **kw)
    for scale in ("ln", "log10", "energy"):                          # PCEN reads log2 energies
        with pytest.raises(ValueError, match="log2"):
            m.set_filterbank(w, scale, pcen=True)
    for kw in (dict(normalize="mean"), dict(deltas=1), dict(pcen=True), dict(normalize_window=40)):
        with pytest.raises(ValueError, match="need a matrix"):
            m.set_filterbank(None, **kw)
    with pytest.raises(TypeError):
        m.set_filterbank(w, "log2", 0.0, "mean")                    # keyword-only


# ------------------------------------------------------------------------------------------------ tiles and grid

def old_delta_tile(lds, W, order, window):
    """kernel_deltas.hpp's formula as it was before the wide form existed."""
    per = (lds - 8) // W
    return (per - 2 * window) // 3 if order == 1 else (per - 6 * window) // 5


def trunc_div(a, b):
    return int(a / b)                                               # C++ integer division truncates towards zero


def test_narrow_tiles_are_the_old_formulas(tiles):
    head, rows = tiles
    assert head[0] == NARROW_LDS and head[2] == 64 and head[3] == 128 and head[4] == NORM_TILE
    for w, order, window, narrow, _, _, norm, stripes, wide in rows:
        if w <= 64:
            per = (NARROW_LDS - 8) // w
            want = trunc_div(per - 2 * window, 3) if order == 1 else trunc_div(per - 6 * window, 5)
            assert narrow == want and want >= 3
            assert norm == NORM_TILE // w and stripes == 256 // w and not wide
        else:
            assert wide


def test_wide_delta_tile_has_at_least_eight_rows_and_fits(tiles):
    head, rows = tiles
    lds = head[1]
    assert 8192 <= lds <= 16384                                     # between 32 and 64 KB
    for w, order, window, _, g, floats, _, _, wide in rows:
        if not wide:
            continue
        assert g == old_delta_tile(lds, w, order, window)           # the same scheme over the larger image
        assert g >= 8, (w, order, window, g)
        # static rows, D rows, the output copy behind up to 3 floats of rounding and up to 3 of pad
        H = order * window
        need = (g + 2 * H) * w + ((g + 2 * window) * w if order == 2 else 0) + 3 + 3 + g * w * (1 + order)
        assert floats <= need + 3 and need <= lds and floats <= lds, (w, order, window)
        # the largest such tile: one more row would go past the image less its 8 floats of slack
        assert (g + 1 + 2 * H) * w + ((g + 1 + 2 * window) * w if order == 2 else 0) + (g + 1) * w * (1 + order) > lds - 8 - w
        # int products of a tile stay small at rows of 384 floats
        assert (g + 2 * H) * w * 4 < 2 ** 31 and g * w * (1 + order) <= lds


def test_wide_normalization_stripes_and_tile_rows(tiles):
    _, rows = tiles
    by_w = {int(r[0]): (int(r[6]), int(r[7])) for r in rows}
    assert by_w[65] == (126, 3) and by_w[85] == (96, 3) and by_w[86] == (95, 2) and by_w[128] == (64, 2)
    for w in range(65, 129):
        t, g = by_w[w]
        assert t == NORM_TILE // w and t * w <= NORM_TILE and g == 256 // w and g >= 2 and g * w <= 256


def test_wide_grid(drivers):
    for n, cu, want in [(1, 256, 1), (2047, 256, 2047), (2048, 256, 2048), (2049, 256, 2048), (10 ** 12, 256, 2048),
                        (5, 1, 5), (9, 1, 8), (100, 0, 8), (3 * 2048 + 1, 304, 2432)]:
        assert int(run_both(drivers, ["grid", str(n), str(cu)])) == want


# ------------------------------------------------------------------------------------------------ scratch layouts

def up256(b):
    return (b + 255) & ~255


@pytest.mark.parametrize("W", [65, 80, 128])
def test_scratch_layouts_against_a_brute_force_sum(drivers, W):
    T = NORM_TILE // W
    rng = np.random.default_rng(W)
    for lens in ([T], [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3], [3 * T] * 4, list(rng.integers(0, 4 * T, 37))):
        off = np.concatenate([[7], 7 + np.cumsum(lens)]).astype(np.int64)
        text = "%d %d %d %s\n" % (W, T, len(lens), " ".join(str(v) for v in off))
        norm, pcen = [[int(v) for v in ln.split()] for ln in run_both(drivers, ["scratch"], text).splitlines()]
        n_blocks = sum(-(-int(n) // T) for n in lens)               # brute force: the tiles of every segment
        uniform = len(set(int(n) for n in lens)) == 1
        table_ll = 0 if uniform else len(lens) + 1 + 2 * n_blocks
        for got, (a0, a1) in ((norm, (n_blocks * W * 24, len(lens) * W * 8)), (pcen, (n_blocks * W * 4, n_blocks * W * 4))):
            assert got[:3] == [n_blocks, len(lens), table_ll]
            assert got[3] == 0 and got[4] == up256(a0) and got[5] == up256(a0) + up256(a1)
            assert got[6] == got[5] + table_ll * 8 + 64
            assert got[4] >= a0 and got[5] - got[4] >= a1           # no area reaches into the next
