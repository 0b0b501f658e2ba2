"""What a segment pass decides on the host, on the CPU: mfcc_amd/csrc/seg_plan.hpp has no HIP in it, so a few lines of
C++ (tests/seg_plan_driver.cpp) print its plan, its table, its scratch layout, every tile as the kernels' own tile_of
gives it, and the answer of the direct entries' argument check.  This test holds them against the rules restated below
and against invariants that do not depend on the restatement.  The records name rows of device buffers: a slip here is
an out-of-bounds read or write on the GPU."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")

OK, INVALID, SMALL = 0, -101, -106                    # include/mfcc_hip.h
PROCEED, NOTHING = 1, 2                               # mfcc_seg::kProceed, kNothing
BLANK = -7777                                         # the driver's fill of the table
READ, WRITE, PACKED, UNSIZED = range(4)               # mfcc_seg::Role
TILE_ROWS = [1, 3, 128, 630]
SELECT = -1                                           # the driver's word for mfcc_seg::kSelectAreas ...
SELECT_AREAS = [(4, 0, 0), (8, 0, 8), (0, 8, 8)]      # ... tile counts, tile prefixes (n_blocks + 1), segment offsets (n_segs + 1)


def up256(b):
    return (b + 255) // 256 * 256


# ---- the scratch of every pass, from the text of the commit before seg_plan.hpp: (areas handed to the layout as
# (per tile, per segment, fixed), the offsets and the total as that commit computed them from nb tiles, ns segments and
# a table of tll long longs).  W = 13; sizeof Part = 24, float2 = 8, MeanPart = 16
W = 13


def _normalize(nb, ns, tll):
    part, coef = up256(nb * W * 24), up256(ns * W * 8)
    return [0, part], part + coef, part + coef + tll * 8 + 64


def _pcen(nb, ns, tll):
    tile = up256(nb * W * 4)
    return [0, tile], 2 * tile, 2 * tile + tll * 8 + 64


def _table_only(nb, ns, tll):                         # deltas, sliding normalization, mfcc_hip_gate_dev
    return [], 0, tll * 8 + 64


def _select(nb, ns, tll):                             # select_plan and mfcc_hip_gate_windows_dev
    cnt, toff, soff = up256(nb * 4), up256((nb + 1) * 8), up256((ns + 1) * 8)
    return [0, cnt, cnt + toff], cnt + toff + soff, cnt + toff + soff + tll * 8 + 64


def _vad_mean(nb, ns, tll):
    part, theta = up256(nb * 16), up256(ns * 8)
    return [0, part], part + theta, part + theta + tll * 8 + 64


PASSES = {
    "normalize": ([(W * 24, 0, 0), (0, W * 8, 0)], _normalize),
    "pcen": ([(W * 4, 0, 0), (W * 4, 0, 0)], _pcen),
    "table_only": ([], _table_only),
    "select": (SELECT, _select),
    "vad_mean": ([(16, 0, 0), (0, 8, 0)], _vad_mean),
}


# ---- the cases
def length_lists(T):
    """segment lengths drawn from {0, 1, T - 1, T, T + 1, 2T + 3}: (name, lengths)"""
    L = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    out = [("all", L), ("reversed", L[::-1]), ("leading_empty", [0, 0, T + 1, 1]), ("trailing_empty", [T, 2 * T + 3, 0, 0]),
           ("consecutive_empty", [T + 1, 0, 0, 0, T - 1, T]), ("equal", [T + 1] * 3), ("equal_1", [1] * 4),
           ("equal_long", [2 * T + 3] * 2), ("equal_but_one", [T + 1] * 3 + [1]), ("equal_but_first", [T] + [2 * T + 3] * 3)]
    out += [("one_%d" % n, [n]) for n in L if n]
    rng = np.random.default_rng(T)
    out += [("drawn_%d" % i, [int(x) for x in rng.choice(L, int(rng.integers(2, 9)))]) for i in range(6)]
    return [(name, lens) for name, lens in out if sum(lens)]


def offsets_of(lens, off0):
    return [off0 + int(x) for x in np.concatenate([[0], np.cumsum(lens)])]


def windows(n, n_frames, stride):
    return (n - n_frames) // stride + 1 if n >= n_frames else 0


def plan_line(width, T, off, extra, areas, n_segs=None):
    """extra: (base offsets, step) of the plan's extra column base[k] - off[k] * step, or None"""
    n_segs = len(off) - 1 if n_segs is None else n_segs
    flat = [] if areas == SELECT else [v for a in areas for v in a]
    return ["plan", width, T, n_segs, len(off), int(extra is not None), SELECT if areas == SELECT else len(areas)] + off + \
        (extra[0] + [extra[1]] if extra else []) + flat


def parse(line, n_areas):
    v = [int(x) for x in line.split()]
    if v[0] != OK:
        assert len(v) == 1
        return v[0], None
    names = ["base_row", "seg_rows", "blocks_per_seg", "n_blocks", "n_segs", "width", "tile_rows", "table_ll"]
    got = dict(zip(names, v[1:9]))
    v = v[9:]
    got["table"], v = v[:got["table_ll"]], v[got["table_ll"]:]
    got["has_extra"], got["area_off"], got["table_off"], got["total"] = v[0], v[1:1 + n_areas], v[1 + n_areas], v[2 + n_areas]
    t = v[3 + n_areas:]
    assert len(t) == 3 * got["n_blocks"]
    got["tiles"] = [tuple(t[i:i + 3]) for i in range(0, len(t), 3)]
    return OK, got


def restated(off, T, uniform, extra):
    """Segs and the table as the planner must give them for unit offsets `off`"""
    n = len(off) - 1
    lens = [b - a for a, b in zip(off, off[1:])]
    if uniform:
        bps = -(-lens[0] // T)
        return dict(base_row=off[0], seg_rows=lens[0], blocks_per_seg=bps, n_blocks=bps * n, table_ll=0, table=[])
    blk0, rec = [], []
    for k in range(n):
        blk0.append(len(rec) // 2)
        for r in range(off[k], off[k + 1], T):
            rec += [r, min(T, off[k + 1] - r) | k << 32]           # BlockRec{long long row0; int rows; int seg;}
    blk0.append(len(rec) // 2)
    table = blk0 + (extra[:n] if extra else []) + rec
    return dict(base_row=0, seg_rows=0, blocks_per_seg=0, n_blocks=len(rec) // 2, table_ll=len(table), table=table)


def check_partition(off, T, got):
    """what must hold whatever the restatement says: the tiles partition every segment's units exactly, in order"""
    n = len(off) - 1
    tiles, b = got["tiles"], 0
    for k in range(n):
        if got["table_ll"]:
            assert got["table"][k] == b                             # seg_blk0 is the running count
        else:
            assert got["blocks_per_seg"] * k == b
        at = off[k]
        while at < off[k + 1]:
            row0, rows, seg = tiles[b]
            assert (row0, seg) == (at, k) and 0 < rows <= T and row0 + rows <= off[k + 1], (k, tiles[b])
            assert rows == T or row0 + rows == off[k + 1]           # only a segment's last tile is short
            at += rows
            b += 1
        assert at == off[k + 1]
    assert b == len(tiles) == got["n_blocks"]
    if got["table_ll"]:
        assert got["table"][n] == b
    assert BLANK not in got["table"]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("seg_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "seg_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


def run(driver, lines):
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


def row_cases():
    """(line, T, off, uniform, extra, pass name): every length list at two first rows, the passes' areas in turn"""
    out = []
    names = itertools.cycle(PASSES)
    for T in TILE_ROWS:
        for name, lens in length_lists(T):
            for off0 in (0, 5):
                off = offsets_of(lens, off0)
                p = next(names)
                out.append((plan_line(W, T, off, None, PASSES[p][0]), T, off, len(set(lens)) == 1, None, p))
    return out


def gate_cases():
    """the same length lists as rows of gate segments: (line, T, off, wo, uniform, extra, n_frames, stride, pass name)"""
    out = []
    names = itertools.cycle(["table_only", "select"])
    for T in TILE_ROWS:
        for n_frames, stride in itertools.product([1, 5, 93], [1, 2, 7]):
            for name, lens in length_lists(T):
                off = offsets_of(lens, 5 if stride == 2 else 0)
                wo = offsets_of([windows(n, n_frames, stride) for n in lens], 0)
                if not wo[-1]:
                    continue
                extra = [o - w * stride for o, w in zip(off, wo)]
                p = next(names)
                line = plan_line(1, T, wo, (off, stride), PASSES[p][0])
                out.append((line, T, off, wo, len(set(lens)) == 1, extra, n_frames, stride, p))
    return out


def test_header_has_no_hip():
    src = open(os.path.join(CSRC, "seg_plan.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert '#include "seg_plan.hpp"' in open(os.path.join(CSRC, "kernel_normalize.hpp")).read()


def check_layout(p, got, n_segs):
    areas, formula = PASSES[p]
    offs, table_off, total = formula(got["n_blocks"], n_segs, got["table_ll"])
    assert (got["area_off"], got["table_off"], got["total"]) == (offs, table_off, total), (p, got)
    ends = got["area_off"][1:] + [got["table_off"]]
    sizes = [a[0] * got["n_blocks"] + a[1] * n_segs + a[2] for a in (SELECT_AREAS if areas == SELECT else areas)]
    for lo, hi, size in zip(got["area_off"], ends, sizes):         # disjoint, aligned, the table behind them
        assert lo % 256 == 0 and lo + size <= hi
    assert got["table_off"] % 256 == 0 and got["table_off"] + got["table_ll"] * 8 <= got["total"]


def test_tiles_partition_the_segments(drivers):
    cases = row_cases()
    cover = dict.fromkeys(["uniform", "table", "empty_segments", "one_segment", "shifted"] + list(PASSES), 0)
    for (line, T, off, uniform, _, p), text in zip(cases, run(drivers[0], [c[0] for c in cases])):
        rc, got = parse(text, len(PASSES[p][1](0, 0, 0)[0]))
        assert rc == OK, line
        want = restated(off, T, uniform, None)
        assert {k: got[k] for k in want} == want, (line, got)
        assert (got["n_segs"], got["width"], got["tile_rows"], got["has_extra"]) == (len(off) - 1, W, T, 0)
        assert (got["table_ll"] == 0) == uniform                   # equal lengths: no table; one odd segment: a table
        check_partition(off, T, got)
        check_layout(p, got, len(off) - 1)
        cover["uniform" if uniform else "table"] += 1
        cover["empty_segments"] += any(a == b for a, b in zip(off, off[1:]))
        cover["one_segment"] += len(off) == 2
        cover["shifted"] += off[0] > 0
        cover[p] += not uniform
    assert all(cover.values()), cover


def test_gate_windows_start_inside_their_segments(drivers):
    cases = gate_cases()
    cover = dict.fromkeys(["uniform", "table", "no_window_segment", "tile_edge_inside"], 0)
    for (line, T, off, wo, uniform, extra, n_frames, stride, p), text in zip(cases, run(drivers[0], [c[0] for c in cases])):
        rc, got = parse(text, len(PASSES[p][1](0, 0, 0)[0]))
        assert rc == OK, line
        want = restated(wo, T, uniform, extra)
        assert {k: got[k] for k in want} == want, (line, got)
        assert got["has_extra"] == (not uniform)
        check_partition(wo, T, got)
        check_layout(p, got, len(off) - 1)
        n = len(off) - 1
        for win0, nw, seg in got["tiles"]:
            for w in (win0, win0 + nw - 1):                         # kernel_gate.hpp first_row(): delta or the uniform rule
                d = got["table"][n + 1 + seg] if not uniform else off[0] + seg * ((off[1] - off[0]) - got["seg_rows"] * stride)
                first = d + w * stride
                assert first == off[seg] + (w - wo[seg]) * stride
                assert off[seg] <= first and first + n_frames <= off[seg + 1]          # the last row touched
        cover["uniform" if uniform else "table"] += 1
        cover["no_window_segment"] += any(a == b for a, b in zip(wo, wo[1:]))
        cover["tile_edge_inside"] += any(b - a > T for a, b in zip(wo, wo[1:]))
    assert all(cover.values()), cover


def test_dense_span_is_filled_in_as_it_is(drivers):
    lines = [["dense", W, T, n, base, rows, 2, W * 24, 0, 0, 0, W * 8, 0] for T in TILE_ROWS for n, base, rows in
             [(1, 0, 1), (3, 7, T + 1), (40000, 0, 1), (5, 2, 2 * T + 3)]]
    for line, text in zip(lines, run(drivers[0], lines)):
        rc, got = parse(text, 2)
        T, n, base, rows = line[2:6]
        assert rc == OK and got["table_ll"] == 0 and (got["base_row"], got["seg_rows"], got["n_segs"]) == (base, rows, n)
        check_partition([base + k * rows for k in range(n + 1)], T, got)
        check_layout("normalize", got, n)


def test_count_refuses_2_31_segments(drivers):
    """BlockRec::seg is an int.  The count is faked, not the array: the refusal comes before any walk over it"""
    lines = [plan_line(W, 4, [0, 1, 3], None, [], n_segs=1 << 31), plan_line(1, 4, [0, 1, 3], ([0, 9, 12], 2), [], n_segs=1 << 31),
             plan_line(W, 4, [0, 1, 3], None, [], n_segs=2)]
    assert [parse(t, 0)[0] for t in run(drivers[0], lines)] == [INVALID, INVALID, OK]


# ---- the argument check.  Each entry below restates the description its C entry hands to check_rows and what the entry
# does with the answer; RUN: the pass is enqueued.  The codes in CALLS were worked out from the entries of the commit
# before seg_plan.hpp, which spelled the checks out one by one.
RUN = "run"
A, B = 0x10000, 0x40000
RB = W * 4                                            # bytes of a float row
OFF = [2, 5, 9]                                       # rows 2 .. 9: bytes A + 104 .. A + 468 of a float row buffer


def check_line(width, max_width, off, ptrs, units=None, n_segs=None):
    n_segs = (len(off) - 1 if off is not None else 0) if n_segs is None else n_segs
    return ["check", width, max_width, n_segs, int(off is not None), int(units is not None), len(ptrs)] + (off or []) + \
        (units or []) + [v for p in ptrs for v in p]


def answer(rc):
    return rc if rc < 0 else (RUN if rc == PROCEED else OK)


def normalize(ask, rows, width=W, off=OFF, mode=2, n_segs=None):
    rc = ask(check_line(width, 64, off, [(rows, 4, width * 4, WRITE, 0)], n_segs=n_segs))
    return OK if rc == PROCEED and mode == 0 else answer(rc)


def pcen(ask, rows, width=W, off=OFF, n_segs=None):
    return answer(ask(check_line(width, 64, off, [(rows, 4, width * 4, WRITE, 0)], n_segs=n_segs)))


def sliding(ask, src, dst, width=W, off=OFF, mode=2):
    ptrs = [(src, 4, width * 4, READ, 0), (dst, 4, width * 4, WRITE, 0)]
    rc = ask(check_line(width, 64, off, [] if mode == 0 else ptrs))
    return OK if rc == PROCEED and mode == 0 else answer(rc)


def deltas(ask, src, dst, width=W, off=OFF, order=2):
    return answer(ask(check_line(width, 64, off, [(src, 4, width * 4, READ, 0), (dst, 4, width * 4 * (1 + order), WRITE, 0)])))


def vad(ask, rows, voiced, width=W, off=OFF):
    return answer(ask(check_line(width, 64, off, [(rows, 4, width * 4, READ, 0), (voiced, 1, 1, WRITE, 0)])))


def select(ask, src, voiced, dst, cap, width=W, off=OFF):
    rc = ask(check_line(width, 192, off, [(src, 4, width * 4, READ, 0), (voiced, 1, 1, READ, 0), (dst, 4, width * 4, PACKED, 0)]))
    return SMALL if rc == PROCEED and cap < off[-1] - off[0] else answer(rc)


GATE_OFF = [2, 13, 17, 30]                            # 11, 4 and 13 rows of 26 bytes: 4, 0 and 5 windows of 5 rows, stride 2
GRB = W * 2                                           # the gate's rows are int16: bytes A + 52 .. A + 780


def gate_units(off):
    if off is None:
        return [0]
    if any(b < a for a, b in zip(off, off[1:])):
        return None                                   # gate_count refuses
    return offsets_of([windows(b - a, 5, 2) for a, b in zip(off, off[1:])], 0)


def gate(ask, rows, power, gate_, ref, off=GATE_OFF):
    wo = gate_units(off)
    if wo is None:
        return INVALID
    rc = ask(check_line(W, 64, off, [(rows, 2, GRB, READ, 0), (power, 8, 8, PACKED, 1), (gate_, 1, 1, PACKED, 1),
                                     (ref, 1, 1, PACKED, 1)], units=wo))
    return INVALID if rc == PROCEED and not (power or gate_ or ref) else answer(rc)


def gate_windows(ask, rows, mask, dst, starts, off=GATE_OFF):
    wo = gate_units(off)
    if wo is None:
        return INVALID
    return answer(ask(check_line(W, 64, off, [(rows, 2, GRB, READ, 0), (mask, 1, 1, READ, 0), (dst, 2, 0, UNSIZED, 1),
                                              (starts, 8, 0, UNSIZED, 1)], units=wo)))


NO_ROWS, DECREASING, BACK_TO_START = [3, 3, 3], [2, 5, 4], [3, 5, 3]
CALLS = [
    # normalize_dev: the pointer is looked at only when there are rows, and mode NONE answers success after that
    (normalize, dict(rows=A), RUN), (normalize, dict(rows=0), INVALID), (normalize, dict(rows=A + 2), INVALID),
    (normalize, dict(rows=0, off=NO_ROWS), OK), (normalize, dict(rows=A + 2, off=NO_ROWS), OK),
    (normalize, dict(rows=A, off=DECREASING), INVALID), (normalize, dict(rows=A, off=BACK_TO_START), INVALID),
    (normalize, dict(rows=A, width=0), INVALID), (normalize, dict(rows=A, width=65), INVALID),
    (normalize, dict(rows=A, width=64), RUN), (normalize, dict(rows=0, off=None), OK),
    (normalize, dict(rows=A, off=None, n_segs=2), INVALID), (normalize, dict(rows=A, mode=0), OK),
    (normalize, dict(rows=0, mode=0), INVALID), (normalize, dict(rows=A + 2, mode=0), INVALID),
    (normalize, dict(rows=0, off=NO_ROWS, mode=0), OK), (normalize, dict(rows=A + 4), RUN),
    # pcen_dev
    (pcen, dict(rows=A), RUN), (pcen, dict(rows=0), INVALID), (pcen, dict(rows=A + 1), INVALID),
    (pcen, dict(rows=0, off=NO_ROWS), OK), (pcen, dict(rows=0, off=None), OK), (pcen, dict(rows=A, off=DECREASING), INVALID),
    (pcen, dict(rows=A, width=65), INVALID), (pcen, dict(rows=A, off=None, n_segs=1), INVALID),
    # normalize_sliding_dev: success for an empty span or mode NONE before the pointers; in and out must not overlap
    (sliding, dict(src=A, dst=B), RUN), (sliding, dict(src=0, dst=B), INVALID), (sliding, dict(src=A, dst=B + 2), INVALID),
    (sliding, dict(src=0, dst=0, off=NO_ROWS), OK), (sliding, dict(src=0, dst=0, off=None), OK),
    (sliding, dict(src=0, dst=0, mode=0), OK), (sliding, dict(src=A, dst=A, mode=0), OK),
    (sliding, dict(src=A, dst=B, mode=0, off=DECREASING), INVALID), (sliding, dict(src=A, dst=B, mode=0, width=65), INVALID),
    (sliding, dict(src=A, dst=A), INVALID), (sliding, dict(src=A, dst=A + 364), RUN), (sliding, dict(src=A, dst=A + 360), INVALID),
    (sliding, dict(src=A, dst=A - 364), RUN), (sliding, dict(src=A, dst=A - 360), INVALID),
    (sliding, dict(src=A, dst=B, off=DECREASING), INVALID), (sliding, dict(src=A, dst=B, width=0), INVALID),
    # deltas_dev (order 2: rows of 156 bytes out, bytes dst + 312 .. dst + 1404)
    (deltas, dict(src=A, dst=B), RUN), (deltas, dict(src=0, dst=B), INVALID), (deltas, dict(src=A, dst=0), INVALID),
    (deltas, dict(src=A + 2, dst=B), INVALID), (deltas, dict(src=0, dst=0, off=NO_ROWS), OK), (deltas, dict(src=0, dst=0, off=None), OK),
    (deltas, dict(src=A, dst=A + 156), RUN), (deltas, dict(src=A, dst=A + 152), INVALID),
    (deltas, dict(src=A, dst=A - 1300), RUN), (deltas, dict(src=A, dst=A - 1296), INVALID),
    (deltas, dict(src=A, dst=B, off=DECREASING), INVALID), (deltas, dict(src=A, dst=B, width=65), INVALID),
    (deltas, dict(src=A, dst=A + 260, order=1), RUN), (deltas, dict(src=A, dst=A + 256, order=1), INVALID),
    # vad_dev: bytes voiced + 2 .. voiced + 9 are written
    (vad, dict(rows=A, voiced=B), RUN), (vad, dict(rows=A, voiced=B + 1), RUN), (vad, dict(rows=A, voiced=0), INVALID),
    (vad, dict(rows=0, voiced=B), INVALID), (vad, dict(rows=A + 2, voiced=B), INVALID),
    (vad, dict(rows=0, voiced=0, off=NO_ROWS), OK), (vad, dict(rows=0, voiced=0, off=None), OK),
    (vad, dict(rows=A, voiced=A + 466), RUN), (vad, dict(rows=A, voiced=A + 465), INVALID),
    (vad, dict(rows=A, voiced=A + 95), RUN), (vad, dict(rows=A, voiced=A + 96), INVALID),
    (vad, dict(rows=A, voiced=B, off=DECREASING), INVALID), (vad, dict(rows=A, voiced=B, width=65), INVALID),
    # select_dev: up to 7 rows of 52 bytes are written from dst on; BUFFER_SMALL after the overlap checks
    (select, dict(src=A, voiced=B, dst=2 * B, cap=7), RUN), (select, dict(src=A, voiced=B, dst=2 * B, cap=6), SMALL),
    (select, dict(src=A, voiced=B, dst=2 * B, cap=7, width=192), RUN), (select, dict(src=A, voiced=B, dst=2 * B, cap=7, width=193), INVALID),
    (select, dict(src=0, voiced=0, dst=0, cap=0, off=NO_ROWS), OK), (select, dict(src=0, voiced=0, dst=0, cap=0, off=None), OK),
    (select, dict(src=0, voiced=B, dst=2 * B, cap=7), INVALID), (select, dict(src=A, voiced=0, dst=2 * B, cap=7), INVALID),
    (select, dict(src=A, voiced=B, dst=0, cap=7), INVALID), (select, dict(src=A, voiced=B, dst=2 * B + 2, cap=7), INVALID),
    (select, dict(src=A, voiced=B, dst=A + 468, cap=7), RUN), (select, dict(src=A, voiced=B, dst=A + 464, cap=7), INVALID),
    (select, dict(src=A, voiced=B, dst=A + 464, cap=6), INVALID), (select, dict(src=A, voiced=B, dst=A - 260, cap=7), RUN),
    (select, dict(src=A, voiced=B, dst=A - 256, cap=7), INVALID), (select, dict(src=A, voiced=B + 362, dst=B, cap=7), RUN),
    (select, dict(src=A, voiced=B + 361, dst=B, cap=7), INVALID), (select, dict(src=A, voiced=B - 9, dst=B, cap=7), RUN),
    (select, dict(src=A, voiced=B - 8, dst=B, cap=7), INVALID), (select, dict(src=A, voiced=A + 104, dst=B, cap=7), RUN),
    (select, dict(src=A, voiced=B, dst=2 * B, cap=0, off=DECREASING), INVALID),
    # gate_dev: 9 windows; at least one output, checked against the rows and against each other
    (gate, dict(rows=A, power=B, gate_=B + 72, ref=B + 81), RUN), (gate, dict(rows=A, power=0, gate_=B, ref=0), RUN),
    (gate, dict(rows=A, power=0, gate_=0, ref=0), INVALID), (gate, dict(rows=0, power=0, gate_=0, ref=0, off=[2, 5, 9]), OK),
    (gate, dict(rows=0, power=0, gate_=0, ref=0, off=None), OK), (gate, dict(rows=0, power=B, gate_=0, ref=0), INVALID),
    (gate, dict(rows=A + 1, power=B, gate_=0, ref=0), INVALID), (gate, dict(rows=A, power=B + 4, gate_=0, ref=0), INVALID),
    (gate, dict(rows=A, power=A + 784, gate_=0, ref=0), RUN), (gate, dict(rows=A, power=A + 776, gate_=0, ref=0), INVALID),
    (gate, dict(rows=A, power=0, gate_=A + 780, ref=0), RUN), (gate, dict(rows=A, power=0, gate_=A + 779, ref=0), INVALID),
    (gate, dict(rows=A, power=0, gate_=A + 43, ref=0), RUN), (gate, dict(rows=A, power=0, gate_=A + 44, ref=0), INVALID),
    (gate, dict(rows=A, power=0, gate_=B, ref=B + 9), RUN), (gate, dict(rows=A, power=0, gate_=B, ref=B + 8), INVALID),
    (gate, dict(rows=A, power=B, gate_=B + 71, ref=0), INVALID), (gate, dict(rows=A, power=B, gate_=0, ref=B - 8), INVALID),
    (gate, dict(rows=A, power=B, gate_=0, ref=B - 9), RUN), (gate, dict(rows=A, power=B, gate_=0, ref=0, off=[2, 13, 12, 30]), INVALID),
    # gate_windows_dev: pointers and alignment now, the ranges once the selected count is known
    (gate_windows, dict(rows=A, mask=B, dst=2 * B, starts=3 * B), RUN), (gate_windows, dict(rows=A, mask=B, dst=0, starts=0), RUN),
    (gate_windows, dict(rows=A, mask=0, dst=2 * B, starts=0), INVALID), (gate_windows, dict(rows=0, mask=B, dst=2 * B, starts=0), INVALID),
    (gate_windows, dict(rows=A + 1, mask=B, dst=2 * B, starts=0), INVALID), (gate_windows, dict(rows=A, mask=B, dst=2 * B + 1, starts=0), INVALID),
    (gate_windows, dict(rows=A, mask=B, dst=2 * B, starts=3 * B + 4), INVALID), (gate_windows, dict(rows=A, mask=B, dst=A, starts=A), RUN),
    (gate_windows, dict(rows=0, mask=0, dst=0, starts=0, off=[2, 5, 9]), OK), (gate_windows, dict(rows=0, mask=0, dst=0, starts=0, off=None), OK),
]


def check_lines():
    """every line the entries of CALLS hand to the driver, in order"""
    lines = []
    for entry, kw, _ in CALLS:
        entry(lambda ln: lines.append(ln) or NOTHING, **kw)
    return lines


def test_entries_keep_their_answers(drivers):
    answers = iter(run(drivers[0], check_lines()))
    for entry, kw, want in CALLS:
        got = entry(lambda ln: int(next(answers)), **kw)
        assert got == want, (entry.__name__, kw, got)


def test_driver_runs_clean_under_the_sanitizers(drivers):
    """the same input through the driver built with -fsanitize=address,undefined, as a program of its own: a record
    written past the table's end, or a tile read past it, ends it"""
    lines = [c[0] for c in row_cases()] + [c[0] for c in gate_cases()] + check_lines() + \
        [plan_line(W, 4, [0, 1, 3], None, [], n_segs=1 << 31)]
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    plain = subprocess.run([drivers[0]], input=text, capture_output=True, text=True, check=True)
    san = subprocess.run([drivers[1]], input=text, capture_output=True, text=True)
    assert san.returncode == 0, san.stderr[-2000:]
    assert san.stdout == plain.stdout
