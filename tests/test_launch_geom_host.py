"""The tile geometry of the eight fused float kernels, on the CPU: mfcc_amd/csrc/launch_geom.hpp has no HIP in it, so a
few lines of C++ (tests/launch_geom_driver.cpp) print what it computes and this test holds that against the formulas
restated below -- one copy per grid rule, as the kernels' launch() functions carried them before they shared one.
t_lo / t_hi decide which tiles are read with aligned 16-byte loads: a slip there is an out-of-bounds read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")

TWO_PER_CU, ONE_PER_CU, PAIRS = 0, 1, 2          # mfcc_fc::GridRule, in the header's order

# kernel -> (headers that define its constants, name of its tile hop, tile, tile_hop, s_used, grid rule, guard bits)
KERNELS = {
    "fused512":         (["kernel_fused512.hpp"], "kTileHop", 16, 2720, 3072, TWO_PER_CU, 31),
    "fused512_w12":     (["kernel_fused512.hpp", "kernel_fused512_w12.hpp"], "kTileHop", 16, 2720, 3072, PAIRS, 30),
    "fused512_h160":    (["kernel_fused512.hpp", "kernel_fused512_h160.hpp"], "kTileHop160", 16, 2560, 3072, TWO_PER_CU, 31),
    "fused512_h160_mb": (["kernel_fused512.hpp", "kernel_fused512_h160.hpp", "kernel_fused512_h160_mb.hpp"],
                         "kTileHop160", 16, 2560, 3072, TWO_PER_CU, 31),
    # the four 1024 forms take their geometry from one header
    "fused1024":        (["fused1024_common.hpp", "kernel_fused1024.hpp"], "kTileHop", 16, 5456, 6152, ONE_PER_CU, 31),
    "fused1024_f32":    (["fused1024_common.hpp", "kernel_fused1024_f32.hpp"], "kTileHop", 16, 5456, 6152, ONE_PER_CU, 31),
    "fused1024_w12":    (["fused1024_common.hpp", "kernel_fused1024_w12.hpp"], "kTileHop", 16, 5456, 6152, PAIRS, 30),
    "fused1024_w12bf":  (["fused1024_common.hpp", "kernel_fused1024_w12.hpp"], "kTileHop", 16, 5456, 6152, PAIRS, 30),
}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _constants(headers):
    """The `constexpr int` definitions of the headers, evaluated in order (later headers see the earlier ones' names,
    as their `using namespace` does)."""
    env = {}
    for name in headers:
        src = re.sub(r"//[^\n]*", "", _read(name))
        for stmt in re.findall(r"^constexpr int ([^;]*);", src, flags=re.M):
            for part in stmt.split(","):
                if "=" not in part:
                    continue
                key, expr = (x.strip() for x in part.split("=", 1))
                try:
                    env[key] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(env)))
                except Exception:
                    pass                      # not integer arithmetic on names seen so far: none of the geometry's
    return env


def test_listed_constants_match_the_headers():
    for kernel, (headers, hop_name, tile, tile_hop, s_used, rule, bits) in KERNELS.items():
        c = _constants(headers)
        assert (c["kTile"], c[hop_name], c["kSUsed"]) == (tile, tile_hop, s_used), kernel
    order = re.search(r"enum class GridRule \{(.*?)\};", _read("launch_geom.hpp"), flags=re.S).group(1)
    assert re.findall(r"^\s*(k\w+),", order, flags=re.M) == ["kTwoPerCu", "kOnePerCu", "kPairs"]


def _cdiv(a, b):
    """C's integer division: toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _int32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def expected(frames_per_ch, total_frames, ch_stride, n_samples, halo, n_cu, tile, tile_hop, s_used, rule, bits):
    """What a kernel's launch() computed before the copies were joined: (ok, workgroups, LaunchGeom fields)."""
    tiles_per_ch = _cdiv(frames_per_ch + tile - 1, tile)
    n_ch = _cdiv(total_frames, frames_per_ch)
    n_tiles = tiles_per_ch * n_ch
    if n_tiles >= 1 << bits or tiles_per_ch >= 1 << 26 or n_ch >= 1 << bits:
        return (0,)
    if rule == PAIRS:                        # the twelve-wave forms: two virtual workgroups in one
        wgs = _cdiv(n_tiles + 1, 2)
        if wgs > n_cu:
            wgs = n_cu
        if wgs < 1:
            wgs = 1
        grid = 2 * wgs
    else:
        cap = n_cu * 2 if rule == TWO_PER_CU else n_cu
        grid = n_tiles if n_tiles < cap else cap
        if grid < 1:
            grid = 1
        wgs = grid
    grid_div, grid_mod = _cdiv(grid, tiles_per_ch), grid % tiles_per_ch
    step_ptr = grid_div * ch_stride + grid_mod * tile_hop
    wrap_ptr = ch_stride - tiles_per_ch * tile_hop
    t_lo = max(0, _cdiv(9 - halo + tile_hop - 1, tile_hop))
    hi = _cdiv(n_samples - s_used, tile_hop)
    t_hi = -1 if n_samples < s_used else _int32(min(hi, tiles_per_ch))
    return (1, wgs, tiles_per_ch, n_ch, grid_div, grid_mod, step_ptr, wrap_ptr, t_lo, t_hi)


def cases():
    out = []
    for kernel, (_, _, tile, tile_hop, s_used, rule, bits) in KERNELS.items():
        k = (tile, tile_hop, s_used, rule, bits)
        for n_cu in (256, 1):
            cap = n_cu if rule == ONE_PER_CU else 2 * n_cu          # tiles at which the cursor stride stops growing
            shapes = [(f, n) for f in (1, tile - 1, tile, tile + 1) for n in (1, 5)]
            for tpc in (1, 3, 7):                                   # n_tiles below, at (where it divides) and above the cap
                f = tile * tpc - (tile - 5 if tpc > 1 else 0)
                shapes += [(f, n) for n in sorted({1, max(1, cap // tpc - 1), max(1, cap // tpc), cap // tpc + 1,
                                                   3 * (cap // tpc) + 2})]
            for f, n_ch in shapes:
                tpc = (f + tile - 1) // tile
                for halo in (0, 1):
                    for n_samples in (s_used - 1, s_used, s_used + tile_hop - 1, tpc * tile_hop + s_used + 123):
                        for pad in (0, 37):                          # ch_stride equal to the channel's extent, and not
                            out.append((kernel, (f, f * n_ch, n_samples + halo + pad, n_samples, halo, n_cu) + k))
        # the three guards, one below and at their limit (the return value is what counts)
        lim = 1 << bits
        for f, n_ch in ((1, lim - 1), (1, lim), (tile * ((1 << 26) - 1), 1), (tile * (1 << 26), 1),
                        (2 * tile, lim // 2 - 1), (2 * tile, lim // 2)):
            out.append((kernel, (f, f * n_ch, 10 * s_used, 10 * s_used, 0, 256) + k))
    # every kernel's tile hop is far above 9, so t_lo is 1 for all of them: small made-up hops pin its formula
    for tile_hop in (1, 4, 8, 9, 10):
        for halo in (0, 1):
            out.append(("t_lo", (40, 200, 1000, 900, halo, 4, 16, tile_hop, 64, TWO_PER_CU, 31)))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    exe = tmp_path_factory.mktemp("launch_geom") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "launch_geom_driver.cpp")], check=True)
    return str(exe)


def test_launch_geom_matches_the_restated_formulas(driver):
    cs = cases()
    text = "".join(" ".join(str(v) for v in c) + "\n" for _, c in cs)
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    # the struct is a kernel argument: 4 ints, 2 long longs, 2 ints
    assert lines[0].split() == ["layout", "40", "0", "4", "8", "12", "16", "24", "32", "36"]
    assert len(lines) == len(cs) + 1
    seen_mod = {0: 0, 1: 0}
    refused = 0
    for (kernel, c), line in zip(cs, lines[1:]):
        got = tuple(int(v) for v in line.split())
        want = expected(*c)
        if want[0] == 0:
            assert got[0] == 0, (kernel, c)
            refused += 1
            continue
        assert got == want, (kernel, c, got, want)
        seen_mod[int(want[5] != 0)] += 1
        assert want[2] * want[4] + want[5] == (2 * want[1] if c[9] == PAIRS else want[1])     # grid = div * tpc + mod
    assert refused == 3 * len(KERNELS) and seen_mod[0] and seen_mod[1]
    assert any(expected(*c)[-1] == -1 for _, c in cs) and any(expected(*c)[-1] > 0 for _, c in cs)
