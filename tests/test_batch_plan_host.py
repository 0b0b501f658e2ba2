"""What a ragged call and a host-buffer call decide on the host, on the CPU: mfcc_amd/csrc/batch_plan.hpp has no HIP in
it, so a few lines of C++ (tests/batch_plan_driver.cpp) print its scan, its route, its tables with the layout of their
device buffers, and its chunk lists.  This test holds them against the arithmetic of the commit before batch_plan.hpp,
restated below, and against invariants that do not depend on the restatement.  Every number here is an address or a
length that a kernel reads or writes: a slip is an out-of-bounds access on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")

OK, INVALID = 0, -101                                   # include/mfcc_hip.h
BLANK = -7777                                           # the driver's fill of every table
UNIFORM, TILE_RECS, FRAME_RECS, PACK = range(4)         # mfcc_batch::Route
NONE, TILES, FRAMES = range(3)                          # mfcc_batch::Records
LIM_LEN, LIM_TILES = 1 << 31, 1 << 30                   # mfcc_batch::Limits
TILE = 16                                               # frames per tile of the fused kernels
FRAMINGS = [(512, 170, 512), (512, 160, 400), (64, 21, 64), (128, 1, 128)]         # (nfft, hop, frame length)
ROW_BYTES = 13 * 4
CHUNK = 1 << 20


def geom(nfft, hop):
    """(tile, samples from a tile to the next, samples of a tile's window): 16, 2720, 3072 for the 512 / 170 kernel"""
    return TILE, TILE * hop, (7 + (TILE - 1) * hop + nfft + 15) // 16 * 16


def frames_of(n, hop, flen, stream):
    if n < flen:
        return int(stream)
    return (n - flen) // hop + 1 + int(stream)


def length_lists(hop, flen):
    """utterance lengths drawn from {0, 1, flen - 1, flen, flen + 1, flen + hop, one tile of frames, one tile + 1 frame,
    two tiles + 3}, in the lists of tests/test_seg_plan_host.py: (name, lengths)"""
    of = lambda k: flen + (k - 1) * hop
    L = [0, 1, flen - 1, flen, flen + 1, flen + hop, of(TILE), of(TILE + 1), of(2 * TILE + 3)]
    T = of(TILE)
    out = [("all", L), ("reversed", L[::-1]), ("leading_empty", [0, 0, T + hop, 1]), ("trailing_empty", [T, of(2 * TILE + 3), 0, 0]),
           ("consecutive_empty", [T + hop, 0, 0, 0, flen - 1, T]), ("equal", [T + hop] * 3), ("equal_1", [1] * 4),
           ("equal_flen", [flen] * 5), ("equal_long", [of(2 * TILE + 3)] * 2), ("equal_but_one", [T + hop] * 3 + [1]),
           ("equal_but_one_sample", [flen + hop, flen + hop, flen + hop + 1]), ("equal_but_first", [T] + [of(2 * TILE + 3)] * 3),
           ("none", [])]
    out += [("one_%d" % n, [n]) for n in L]
    rng = np.random.default_rng(hop)
    out += [("drawn_%d" % i, [int(x) for x in rng.choice(L, int(rng.integers(2, 9)))]) for i in range(6)]
    return out


def offsets_of(lens, off0):
    return [off0 + int(x) for x in np.concatenate([[0], np.cumsum(lens)])] if lens else [off0]


def ragged_line(flen, hop, stream, g, off, kernel=NONE, fixed=0, lim_len=0, lim_tiles=0, chunk=CHUNK):
    return ["ragged", flen, hop, int(stream), g[0], g[1], g[2], ROW_BYTES, kernel, fixed, lim_len, lim_tiles, chunk,
            len(off) - 1] + off


def take(v, n):
    return v[:n], v[n:]


def parse_ragged(text, n):
    v = [int(x) for x in text.split()]
    if v[0] != OK:
        return dict(rc=v[0], fo=v[1:])
    got = dict(zip(["rc", "total", "n_tiles", "max_len", "len0", "frames0", "uniform"], v[:7]))
    got["fo"], v = take(v[7:], n + 1)
    (got["route"], got["table_ll"]), v = take(v, 2)
    pack, v = take(v, 7)
    got["pack"] = dict(zip(["len", "F", "desc_ll", "gather_ll", "in_bytes", "desc_off", "out_bytes"], pack))
    got["desc"], v = take(v, 7 * n)
    tp, v = take(v, 4)
    got["tiles"] = dict(zip(["n_tiles", "chan_ll", "map_off", "bytes"], tp))
    ch, v = take(v, 6 * n)
    got["chans"] = [tuple(ch[i:i + 6]) for i in range(0, len(ch), 6)]
    rp, v = take(v, 3)
    got["recs_plan"] = dict(zip(["n_recs", "rec_ll", "bytes"], rp))
    rr, v = take(v, 6 * rp[0])
    got["recs"] = [tuple(rr[i:i + 6]) for i in range(0, len(rr), 6)]
    (nr,), v = take(v, 1)
    assert len(v) == 4 * nr
    got["ranges"] = [tuple(v[i:i + 4]) for i in range(0, len(v), 4)]
    return got


# ---- the commit before batch_plan.hpp, restated: process_ragged_dev_raw's loops, process_ragged's and process_host's cutters
def restated_ragged(off, hop, flen, stream, g, kernel, fixed, lim_len, lim_tiles, chunk):
    n_utt = len(off) - 1
    lens = [b - a for a, b in zip(off, off[1:])]
    nfs = [frames_of(n, hop, flen, stream) for n in lens]
    fo = [0] + [int(x) for x in np.cumsum(nfs)]
    want = dict(total=fo[-1], fo=fo, uniform=int(n_utt >= 1 and nfs[0] > 0 and len(set(lens)) == 1))
    desc, gather, pos, last = [], [], 0, None
    for u in range(n_utt):
        d = [off[u], pos, lens[u] if nfs[u] else 0]
        gather += [pos // hop, fo[u], nfs[u]]
        if nfs[u]:
            pos = (pos + max(lens[u], hop * (nfs[u] - 1) + flen) + 1 + hop - 1) // hop * hop
            last = u
        desc += d + [pos]
    F, ln = pos // hop, pos + flen + hop
    if last is not None:
        desc[4 * last + 3] = ln
    want["desc"] = desc + gather
    want["pack"] = dict(len=ln, F=F, desc_ll=7 * n_utt, gather_ll=4 * n_utt, in_bytes=ln * 2 + 64,
                        desc_off=(F * ROW_BYTES + 7) & ~7, out_bytes=F * ROW_BYTES + 7 * n_utt * 8 + 64)
    chans, n_tiles = [], 0
    for u in range(n_utt):
        tiles = -(-nfs[u] // g[0])
        t_hi = -1 if lens[u] < g[2] else min((lens[u] - g[2]) // g[1], tiles)
        chans.append((off[u], fo[u], lens[u], nfs[u], t_hi, n_tiles))
        n_tiles += tiles
    want["chans"] = chans
    map_off = (n_utt * 32 + 255) & ~255
    want["tiles"] = dict(n_tiles=n_tiles, chan_ll=4 * n_utt, map_off=map_off, bytes=map_off + n_tiles * 32 + 64)
    want["n_tiles"] = n_tiles
    want["recs"] = [(off[u], fo[u], lens[u], nfs[u], 0, 0) for u in range(n_utt) if nfs[u]]
    want["recs_plan"] = dict(n_recs=len(want["recs"]), rec_ll=4 * len(want["recs"]), bytes=32 * len(want["recs"]) + 64)
    rec_fits = n_utt < lim_len and all(n < lim_len for n in lens)
    if want["uniform"]:
        want["route"] = UNIFORM
    elif not fixed and kernel == TILES and rec_fits and n_tiles < lim_tiles:
        want["route"] = TILE_RECS
    elif fixed and kernel == FRAMES and rec_fits:
        want["route"] = FRAME_RECS
    else:
        want["route"] = PACK
    ranges, u0 = [], 0
    for u in range(n_utt):
        if u + 1 == n_utt or (off[u + 1] - off[u0]) * 2 >= chunk:
            ranges.append((u0, u + 1, fo[u0], fo[u + 1]))
            u0 = u + 1
    want["ranges"] = ranges
    return want


def restated_dense(n, nch, nf, row, hop, flen, chunk):
    """(in_off, in_samples, n, stride, nch, halo, frames, out_elems, out_off) per chunk, and the staging rows"""
    chunks, ch_bytes = [], n * 2
    if ch_bytes <= chunk:
        per = max(chunk // (ch_bytes or 1), 1)
        for c0 in range(0, nch, per):
            k = min(per, nch - c0)
            chunks.append((c0 * n, k * n, n, n, k, 0, nf, k * nf * row, c0 * nf * row))
        return chunks, min(nch, chunk // (ch_bytes or 1) + 1) * nf
    per = max((chunk // 2) // hop, 1)
    for c in range(nch):
        for f0 in range(0, nf, per):
            f1, halo = min(nf, f0 + per), int(f0 > 0)
            s0, s1 = f0 * hop - halo, min((f1 - 1) * hop + flen, n)
            chunks.append((c * n + s0, s1 - s0, s1 - s0 - halo, s1 - s0, 1, halo, f1 - f0, (f1 - f0) * row, (c * nf + f0) * row))
    return chunks, None


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("batch_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "batch_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


def run(driver, lines):
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


def ragged_cases():
    """(line, arguments of restated_ragged, name): every list at offsets[0] 0 and 7, both padding modes; the kernel kinds
    and contracts in turn; a chunk size that cuts the longer lists"""
    out, k = [], 0
    for nfft, hop, flen in FRAMINGS:
        g = geom(nfft, hop)
        for stream in (False, True):
            for name, lens in length_lists(hop, flen):
                for off0 in (0, 7):
                    off = offsets_of(lens, off0)
                    kernel, fixed = [(TILES, 0), (FRAMES, 1), (NONE, 0), (NONE, 1), (TILES, 1), (FRAMES, 0)][k % 6]
                    chunk = [CHUNK, 2 * (flen + hop), 2][k % 3]
                    k += 1
                    out.append((ragged_line(flen, hop, stream, g, off, kernel, fixed, chunk=chunk),
                                (off, hop, flen, stream, g, kernel, fixed, LIM_LEN, LIM_TILES, chunk), name))
    return out


def test_header_has_no_hip():
    src = open(os.path.join(CSRC, "batch_plan.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src and '#include "kernel' not in src
    for kernel in ("kernel_fused512_w12.hpp", "kernel_fixed512.hpp"):
        text = open(os.path.join(CSRC, kernel)).read()
        assert '#include "batch_plan.hpp"' in text and "struct Ragged" not in text.replace("struct RaggedTables", "")


def check_invariants(got, off, hop, flen, stream, g):
    """what must hold whatever the restatement says"""
    n_utt = len(off) - 1
    lens = [b - a for a, b in zip(off, off[1:])]
    nfs = [frames_of(n, hop, flen, stream) for n in lens]
    fo = got["fo"]
    assert fo[0] == 0 and [b - a for a, b in zip(fo, fo[1:])] == nfs and got["total"] == sum(nfs)
    assert got["max_len"] == max(lens, default=0)
    # the uniform route exactly when all lengths are equal and have a frame
    assert (got["route"] == UNIFORM) == bool(n_utt and len(set(lens)) == 1 and nfs[0] > 0)
    for tbl in (got["desc"], [x for c in got["chans"] for x in c], [x for c in got["recs"] for x in c]):
        assert BLANK not in tbl
    # ---- pack and gather
    desc, gather, p = got["desc"][:4 * n_utt], got["desc"][4 * n_utt:], got["pack"]
    assert p["gather_ll"] == 4 * n_utt and p["desc_ll"] == 7 * n_utt
    at, last = 0, max([u for u in range(n_utt) if nfs[u]], default=None)
    for u in range(n_utt):
        src, dst, n, end = desc[4 * u:4 * u + 4]
        row0, out0, rows = gather[3 * u:3 * u + 3]
        assert (src, out0, rows) == (off[u], fo[u], nfs[u])
        if not nfs[u]:
            assert n == 0 and end == dst                            # nothing copied: an empty span, which the kernel skips
            continue
        assert dst == at and end > dst                              # the spans tile the stream in order ...
        at = end
        assert n == lens[u] and dst % hop == 0 and row0 == dst // hop
        assert dst + max(n, hop * (nfs[u] - 1) + flen) + 1 <= end   # a zero behind it == in front of the next one
        assert row0 + rows <= p["F"]
    if last is not None:
        assert at == p["len"]                                       # ... exactly once, up to its end
        # every frame of the packed stream lies inside it (launch: p.F frames forced, frame F - 1 ends inside len)
        assert (p["F"] - 1) * hop + flen <= p["len"] and p["in_bytes"] >= 2 * p["len"]
    assert p["desc_off"] % 8 == 0 and p["desc_off"] >= p["F"] * ROW_BYTES
    assert p["desc_off"] + 8 * p["desc_ll"] <= p["out_bytes"]
    # ---- tile records
    t, tile0 = got["tiles"], 0
    for u, (pcm, row, n, nf, t_hi, t0) in enumerate(got["chans"]):
        tiles = -(-nfs[u] // g[0])
        assert (pcm, row, n, nf, t0) == (off[u], fo[u], lens[u], nfs[u], tile0)
        tile0 += tiles
        assert t_hi <= tiles
        for k in range(1, t_hi + 1):                                # no tile named whose window leaves the utterance
            assert k * g[1] + g[2] <= n
    assert tile0 == t["n_tiles"] == got["n_tiles"]
    assert t["map_off"] % 256 == 0 and t["map_off"] >= 32 * n_utt and t["map_off"] + 32 * t["n_tiles"] <= t["bytes"]
    assert t["chan_ll"] * 8 == 32 * n_utt
    # ---- frame records: exactly the utterances with frames
    assert [(r[0], r[1], r[2], r[3]) for r in got["recs"]] == [(off[u], fo[u], lens[u], nfs[u]) for u in range(n_utt) if nfs[u]]
    rp = got["recs_plan"]
    assert rp["n_recs"] == len(got["recs"]) and rp["rec_ll"] * 8 == 32 * rp["n_recs"] <= rp["bytes"]
    # the host table of the route holds what is filled into it
    need = {UNIFORM: 0, TILE_RECS: t["chan_ll"], FRAME_RECS: rp["rec_ll"], PACK: p["desc_ll"]}[got["route"]]
    assert got["table_ll"] >= need


def check_ranges(got, off, chunk):
    n_utt, at = len(off) - 1, 0
    for u0, u1, rows0, rows1 in got["ranges"]:
        assert u0 == at and u1 > u0 and (rows0, rows1) == (got["fo"][u0], got["fo"][u1])
        at = u1
        size = lambda u: (off[u] - off[u0]) * 2
        assert u1 == n_utt or size(u1) >= chunk                     # closed because it is full, or the last
        assert all(size(u) < chunk for u in range(u0 + 1, u1))      # ... and as soon as it was
    assert at == n_utt


def test_ragged_plans(drivers):
    cases = ragged_cases()
    cover = dict.fromkeys(["uniform", "tile_recs", "frame_recs", "pack", "no_frames", "no_utterance", "empties", "shifted",
                           "stream", "many_ranges", "just_not_uniform"], 0)
    for (line, args, name), text in zip(cases, run(drivers[0], [c[0] for c in cases])):
        off, hop, flen, stream, g, kernel, fixed, _, _, chunk = args
        got = parse_ragged(text, len(off) - 1)
        assert got["rc"] == OK, line
        want = restated_ragged(*args)
        assert {k: got[k] for k in want} == want, (name, line, got, want)
        check_invariants(got, off, hop, flen, stream, g)
        check_ranges(got, off, chunk)
        cover[["uniform", "tile_recs", "frame_recs", "pack"][got["route"]]] += 1
        cover["no_frames"] += got["total"] == 0 and len(off) > 1
        cover["no_utterance"] += len(off) == 1
        cover["empties"] += any(a == b for a, b in zip(off, off[1:]))
        cover["shifted"] += off[0] > 0
        cover["stream"] += bool(stream)
        cover["many_ranges"] += len(got["ranges"]) > 2
        cover["just_not_uniform"] += name == "equal_but_one_sample" and got["route"] != UNIFORM
    assert all(cover.values()), cover


def test_lowered_limits_fall_through_to_pack_and_gather(drivers):
    """the record routes' limits (2^31 samples or utterances, 2^30 tiles) cannot be reached at a size a test can hold:
    lowered to just the case's own values, the route is pack-and-gather and the pack table is what it was"""
    lines, wants = [], []
    for nfft, hop, flen in FRAMINGS:
        g = geom(nfft, hop)
        for name, lens in length_lists(hop, flen):
            off = offsets_of(lens, 7)
            base = restated_ragged(off, hop, flen, False, g, TILES, 0, LIM_LEN, LIM_TILES, CHUNK)
            if base["route"] != TILE_RECS or not base["total"]:
                continue
            n_utt, longest = len(lens), max(lens)
            for kernel, fixed, lim_len, lim_tiles, route in (
                    (TILES, 0, 0, 0, TILE_RECS), (FRAMES, 1, 0, 0, FRAME_RECS),
                    (TILES, 0, longest, 0, PACK), (FRAMES, 1, longest, 0, PACK),                # a sample count does not fit
                    (TILES, 0, longest + 1, 0, TILE_RECS if n_utt <= longest else PACK),
                    (FRAMES, 1, longest + 1, 0, FRAME_RECS if n_utt <= longest else PACK),
                    (TILES, 0, 0, base["n_tiles"], PACK), (TILES, 0, 0, base["n_tiles"] + 1, TILE_RECS),   # the tile count
                    (FRAMES, 1, 0, 1, FRAME_RECS)):                                             # ... is not the frame records'
                lines.append(ragged_line(flen, hop, False, g, off, kernel, fixed, lim_len, lim_tiles))
                wants.append((route, base, len(off) - 1))
    assert len(lines) > 50
    for line, (route, base, n), text in zip(lines, wants, run(drivers[0], lines)):
        got = parse_ragged(text, n)
        assert got["route"] == route, line
        assert got["desc"] == base["desc"] and got["pack"] == base["pack"], line
        assert got["table_ll"] == (7 * n if route == PACK else 4 * n)
    # the utterance count against the same limit
    off = offsets_of([1, 600, 0, 700, 3], 0)
    for lim_len, route in ((5, PACK), (6, PACK), (701, TILE_RECS)):
        text = run(drivers[0], [ragged_line(512, 170, False, geom(512, 170), off, TILES, 0, lim_len, 0)])[0]
        assert parse_ragged(text, 5)["route"] == route


def test_decreasing_offsets_are_refused(drivers):
    g = geom(512, 170)
    for off, written in (([0, 600, 599, 2000], 2), ([5, 4], 1), ([0, 0, 700, 700, 699], 4)):
        got = parse_ragged(run(drivers[0], [ragged_line(512, 170, False, g, off)])[0], len(off) - 1)
        assert got["rc"] == INVALID
        lens = [b - a for a, b in zip(off, off[1:])][:written - 1]
        assert got["fo"][:written] == [0] + [int(x) for x in np.cumsum([frames_of(n, 170, 512, False) for n in lens])]


def dense_cases():
    out = []
    for nfft, hop, flen in FRAMINGS:
        for stream in (False, True):
            for n in (0, flen - 1, flen, flen + hop + 1, flen + 36 * hop, flen + 37 * hop + hop // 2):
                for nch in (1, 3, 8):
                    for chunk in (1, 2 * hop, 2 * flen + 2, 2 * n, 2 * n - 2, 5 * n + 1, 16 * n, 1 << 20):
                        if chunk > 0:
                            out.append((flen, hop, stream, n, nch, 13, chunk))
    return out


def test_dense_chunks(drivers):
    cases = dense_cases()
    lines = [["dense", flen, hop, int(stream), n, nch, row, chunk] for flen, hop, stream, n, nch, row, chunk in cases]
    cover = dict.fromkeys(["channels", "ranges", "halo", "clipped", "one_chunk", "smaller_staging"], 0)
    for (flen, hop, stream, n, nch, row, chunk), text in zip(cases, run(drivers[0], lines)):
        v = [int(x) for x in text.split()]
        nf, cuts, max_rows, n_chunks = v[:4]
        chunks = [tuple(v[i:i + 9]) for i in range(4, len(v), 9)]
        assert nf == frames_of(n, hop, flen, stream) and len(chunks) == n_chunks
        if not nf:
            assert not chunks
            continue
        want, staging = restated_dense(n, nch, nf, row, hop, flen, chunk)
        assert chunks == want and cuts == int(2 * n > chunk)
        # the staging rows: those of the largest chunk, never more than the parent's estimate
        assert max_rows == max(c[4] * c[6] for c in chunks)
        if staging is not None:
            assert max_rows <= staging
            cover["smaller_staging"] += max_rows < staging
        # every (channel, frame) in exactly one chunk; ascending in both buffers; nothing read past n
        seen = np.zeros((nch, nf), int)
        in_end = out_end = 0
        for in_off, in_samples, cn, stride, cch, halo, frames, out_elems, out_off in chunks:
            assert in_off >= in_end - (flen + 1) and out_off == out_end and out_elems == cch * frames * row
            in_end, out_end = in_off + in_samples, out_off + out_elems
            c0, f0 = divmod(out_off // row, nf)
            assert out_off % row == 0 and in_samples == (cch - 1) * stride + cn + halo
            if cuts:
                assert cch == 1 and halo == int(f0 > 0) and in_off == c0 * n + f0 * hop - halo
                assert in_off + in_samples <= (c0 + 1) * n
                assert (frames - 1) * hop + (flen if not stream else 0) <= cn      # its last frame: whole, or STREAM's padded one
                cover["clipped"] += (frames - 1) * hop + flen > cn
            else:
                assert halo == 0 and f0 == 0 and frames == nf and in_off == c0 * n and stride == cn == n
            assert in_off + in_samples <= nch * n
            seen[c0:c0 + cch, f0:f0 + frames] += 1
            cover["halo"] += halo
        assert (seen == 1).all() and out_end == nch * nf * row
        assert [c[0] for c in chunks] == sorted(c[0] for c in chunks)
        cover["ranges" if cuts else "channels"] += 1
        cover["one_chunk"] += n_chunks == 1
    assert all(cover.values()), cover


def test_sanitized_driver_agrees(drivers):
    """the same cases through the driver built with -fsanitize=address,undefined: every table is allocated at exactly the
    length its plan names"""
    lines = [c[0] for c in ragged_cases()]
    lines += [["dense", flen, hop, int(stream), n, nch, row, chunk] for flen, hop, stream, n, nch, row, chunk in dense_cases()]
    assert run(drivers[1], lines) == run(drivers[0], lines)
