"""Sample-rate conversion on the CPU (include/mfcc_hip.h "sample rates"): the shipped tap table
against the float64 design of tests/resample_ref.py, the refusals, the counts, mfcc_hip_resample_host against the index
rule bit for bit, one quality check whose bound comes from the design, and mfcc_amd/csrc/resample_plan.hpp (no HIP in
it) through tests/resample_plan_driver.cpp, plain and built with -fsanitize=address,undefined: every number it prints
is an address or a length the kernel reads or writes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mfcc_amd
from mfcc_amd import _lib
import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")
OK, INVALID, UNSUPPORTED, SMALL = 0, -101, -105, -106
TILE, MAX_SPAN = 2048, 16384                              # mfcc_rs::kTile, kMaxSpan
IDS = ["%d_%d" % r for r in rr.RATIOS]


def geometry_of(i, o):
    lib = _lib.load()
    L, M, K = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = lib.mfcc_hip_resample_geometry(i, o, C.byref(L), C.byref(M), C.byref(K))
    return rc, L.value, M.value, K.value


# ---- the table
@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_table(ratio):
    L, M, H, K = rr.geometry(*ratio)
    assert geometry_of(*ratio) == (OK, L, M, K)
    t = mfcc_amd.resample_taps(*ratio)
    assert t.shape == (L, K) and t.dtype == np.int16
    want = 16384 * rr.design(*ratio)
    err = np.abs(t - want)
    residual = 16384 - np.rint(want).sum(axis=1)
    off = err > 0.5 + 1e-6
    assert (off.sum(axis=1) <= 1).all()                                       # the one adjusted tap per phase
    assert (err.max(axis=1) <= 0.5 + 1e-6 + np.abs(residual)).all()
    assert (t.astype(np.int64).sum(axis=1) == 16384).all()
    mag = np.abs(t.astype(np.int64)).sum(axis=1).max()
    print("%s: L %d K %d, max sum|T| %d, largest residual %d" % (ratio, L, K, mag, np.abs(residual).max()))
    assert mag <= 65535


def test_refusals():
    lib = _lib.load()
    n = C.c_size_t(7)
    for i, o in [(0, 16000), (16000, 0), (-8000, 16000), (8000, -1)]:
        assert geometry_of(i, o)[0] == INVALID
        assert lib.mfcc_hip_resample_count(i, o, 10, C.byref(n)) == INVALID
        assert lib.mfcc_hip_resample_taps(i, o, None, 0, C.byref(n)) == INVALID
        assert lib.mfcc_hip_resample_host(i, o, None, 0, None, 0) == INVALID
    # L or M over 1024, a table over 64 KiB (1000 phases of 34 taps)
    for i, o in [(16000, 16001), (16001, 16000), (1025, 1), (1, 1025), (1001, 1000)]:
        assert geometry_of(i, o) == (UNSUPPORTED, -1, -1, -1)
        assert lib.mfcc_hip_resample_count(i, o, 10, C.byref(n)) == UNSUPPORTED
        assert lib.mfcc_hip_resample_taps(i, o, None, 0, C.byref(n)) == UNSUPPORTED
        assert lib.mfcc_hip_resample_host(i, o, None, 0, None, 0) == UNSUPPORTED
    assert n.value == 7
    assert geometry_of(1024, 1)[:3] == (OK, 1, 1024) and geometry_of(1, 1024)[:3] == (OK, 1024, 1)     # the limits themselves
    # short buffers: nothing is written
    buf = np.full(64, 77, np.int16)
    assert lib.mfcc_hip_resample_taps(8000, 16000, _lib.ptr(buf), 63, C.byref(n)) == SMALL and n.value == 64
    assert (buf == 77).all()
    assert lib.mfcc_hip_resample_taps(8000, 16000, None, 64, None) == INVALID
    x = np.arange(10, dtype=np.int16)
    assert lib.mfcc_hip_resample_host(8000, 16000, _lib.ptr(x), 10, _lib.ptr(buf), 19) == SMALL
    assert (buf == 77).all()
    assert lib.mfcc_hip_resample_host(8000, 16000, None, 10, _lib.ptr(buf), 64) == INVALID
    assert lib.mfcc_hip_resample_host(8000, 16000, _lib.ptr(x), 10, None, 64) == INVALID
    assert lib.mfcc_hip_resample_count(8000, 16000, 10, None) == INVALID
    assert lib.mfcc_hip_resample_count(8000, 16000, 1 << 40, C.byref(n)) == INVALID
    assert lib.mfcc_hip_resample_host(8000, 16000, None, 0, None, 0) == OK                             # n = 0 looks at no pointer


# ---- counts
@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_count_against_brute_force(ratio):
    L, M, H, K = rr.geometry(*ratio)
    for n in list(range(0, 3 * K + 1)) + [1027, 10 ** 6 + 1]:
        brute = 0
        while brute * M < n * L:                    # output m exists while its instant m M / L lies in front of sample n
            brute += 1
        assert mfcc_amd.resample_count(n, *ratio) == brute == rr.count(n, L, M)


# ---- the host entry against the index rule
def lengths_of(H, K):
    return [0, 1, H - 1, H, H + 1, K, K + 1, 1027]


@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_host_against_rule(ratio):
    L, M, H, K = rr.geometry(*ratio)
    t = mfcc_amd.resample_taps(*ratio)
    rng = np.random.default_rng(L * 1031 + M)
    for n in lengths_of(H, K):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        got = mfcc_amd.resample(x, *ratio)
        assert got.dtype == np.int16 and got.shape == (rr.count(n, L, M),)
        assert np.array_equal(got, rr.resample(t, x, L, M)), n


@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_host_constant_line(ratio):
    L, M, H, K = rr.geometry(*ratio)
    for c in (12345, -32768, 32767, -1):
        n = 4 * K + 1027
        got = mfcc_amd.resample(np.full(n, c, np.int16), *ratio)
        m = np.arange(len(got))
        inside = (m * M // L - H + 1 >= 0) & (m * M // L + H < n)              # every tap on the line
        assert inside.sum() > 100 and (got[inside] == c).all()


@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_host_worst_case_saturates_without_wrap(ratio):
    """the input that makes one output's sum -32768 * sum|T| (32767 under the negative taps), for a few phases"""
    L, M, H, K = rr.geometry(*ratio)
    t = mfcc_amd.resample_taps(*ratio)
    for m in sorted({(H // M + 2) * L + p for p in (0, 1, L // 2, L - 1)}):        # q >= H: every tap on the line
        q, p = m * M // L, m * M % L
        n = q + H + 1 + K
        x = np.zeros(n, np.int16)
        x[q - H + 1:q + H + 1] = np.where(t[p] > 0, -32768, 32767)
        acc = rr.accumulate(t, x, L, M, 0, rr.count(n, L, M))
        assert acc[m] == -(32768 * t[p][t[p] > 0].astype(np.int64).sum() - 32767 * t[p][t[p] < 0].astype(np.int64).sum())
        assert acc[m] < -32768 * 16384 and np.abs(acc).max() < 2 ** 31 - 8192  # saturates; fits 32 bits with the rounding term
        got = mfcc_amd.resample(x, *ratio)
        assert got[m] == -32768 and np.array_equal(got, rr.finish(acc))
        got = mfcc_amd.resample((-x.astype(np.int32)).clip(-32768, 32767).astype(np.int16), *ratio)
        assert got[m] == 32767


def test_tone_quality():
    """1 kHz, amplitude 20000, 8 -> 16 kHz against the analytic tone.  The bound is the design's: half an LSB of the
    output rounding, the taps' quantisation, and the distance of every phase's response at that frequency from the
    pure delay e^{j w p / L} it stands for."""
    i, o, A, f = 8000, 16000, 20000.0, 1000.0
    L, M, H, K = rr.geometry(i, o)
    t, g = mfcc_amd.resample_taps(i, o), rr.design(i, o)
    w = 2 * np.pi * f / i
    n = 4000
    x = np.rint(A * np.sin(w * np.arange(n) + 0.3))
    y = mfcc_amd.resample(x.astype(np.int16), i, o).astype(np.float64)
    m = np.arange(len(y))
    ideal = A * np.sin(w * m * M / L + 0.3)
    k = np.arange(K)
    G = (g * np.exp(1j * w * (k - H + 1))[None, :]).sum(axis=1)
    resp = np.abs(G - np.exp(1j * w * np.arange(L) / L)).max()
    quant = np.abs(t / 16384.0 - g).sum(axis=1).max()
    bound = 0.5 + A * quant + A * resp
    inside = (m * M // L - H + 1 >= 0) & (m * M // L + H < n)
    err = np.abs(y - ideal)[inside].max()
    print("tone: error %.2f, bound %.2f (quantisation %.2f, response %.2f)" % (err, bound, A * quant, A * resp))
    assert inside.sum() > 7000 and err <= bound


def random_chunks(rng, total, k):
    """k chunk lengths that sum to `total`, empty and 1-sample chunks among them"""
    cuts = np.sort(rng.integers(0, total + 1, k - 1))
    lens = np.diff(np.concatenate([[0], cuts, [total]])).astype(int).tolist()
    lens[int(rng.integers(0, k))] = 0                       # (the sum no longer matters: the lengths are what is pushed)
    lens[int(rng.integers(0, k))] = 1
    return lens


def stream_plan(ratio, seen, offsets, flush):
    lib = _lib.load()
    seen = np.asarray(seen, np.uint64)
    off = None if offsets is None else np.asarray(offsets, np.uint64)
    oo = np.full(len(seen) + 1, 99, np.uint64)
    rc = lib.mfcc_hip_resampler_plan(ratio[0], ratio[1], _lib.ptr(seen), _lib.ptr(off), len(seen), int(flush), _lib.ptr(oo))
    return rc, oo


@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_stream_plan_against_brute_force(ratio):
    """E(c) and mfcc_hip_resampler_plan: what a line emits push by push is what the one-shot rule can compute from the
    samples it has -- output m needs x[q + H], so it exists once c > q + H -- counted one output at a time"""
    L, M, H, K = rr.geometry(*ratio)

    def brute_emitted(c):
        m = 0
        while m * M // L + H < c and m * M < c * L:
            m += 1
        return m

    for c in range(0, 3 * K + 1):
        assert rr.emitted(c, L, M, H) == brute_emitted(c)
        assert stream_plan(ratio, [c], None, True) == (OK, pytest.approx([0, rr.count(c, L, M) - brute_emitted(c)]))
    rng = np.random.default_rng(M * 7 + L)
    for _ in range(6):
        lines = 4
        chunks = [random_chunks(rng, int(rng.integers(2, 3 * K)), 6) for _ in range(lines)]
        seen = [0] * lines
        for step in range(6):
            lens = [chunks[u][step] for u in range(lines)]
            off = np.concatenate([[0], np.cumsum(lens)]) + 5
            rc, oo = stream_plan(ratio, seen, off, False)
            assert rc == OK and oo[0] == 0
            assert [int(v) for v in np.diff(oo.astype(np.int64))] == [brute_emitted(c + n) - brute_emitted(c) for c, n in zip(seen, lens)]
            rc, fl = stream_plan(ratio, seen, off, True)
            assert rc == OK and [int(v) for v in np.diff(fl.astype(np.int64))] == \
                [rr.count(c + n, L, M) - brute_emitted(c + n) for c, n in zip(seen, lens)]
            seen = [c + n for c, n in zip(seen, lens)]
    # the brute-force stream of the reference module agrees with its own one-shot rule
    t = mfcc_amd.resample_taps(*ratio)
    x = rng.integers(-32768, 32768, 2 * K + 77).astype(np.int16)
    lens = random_chunks(rng, len(x), 7)
    x = x[:sum(lens)] if sum(lens) <= len(x) else np.concatenate([x, x])[:sum(lens)]
    parts = np.split(x, np.cumsum(lens)[:-1])
    outs, last = rr.stream(t, parts, L, M)
    assert np.array_equal(np.concatenate(outs + [last]), mfcc_amd.resample(x, *ratio))


def test_stream_plan_refusals():
    assert stream_plan((0, 16000), [0], [0, 1], False)[0] == INVALID
    assert stream_plan((16000, 16001), [0], [0, 1], False)[0] == UNSUPPORTED
    assert stream_plan((8000, 16000), [0, 0], [0, 5, 4], False)[0] == INVALID           # decreasing
    assert stream_plan((8000, 16000), [0], None, False)[0] == INVALID                   # a push needs offsets
    assert stream_plan((8000, 16000), [1 << 40], [0, 1], False)[0] == INVALID
    lib = _lib.load()
    assert lib.mfcc_hip_resampler_plan(8000, 16000, None, None, 1, 1, None) == INVALID
    oo = np.full(1, 9, np.uint64)
    assert lib.mfcc_hip_resampler_plan(8000, 16000, None, None, 0, 0, _lib.ptr(oo)) == OK and oo[0] == 0


# ---- resample_plan.hpp through its driver
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("resample_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "resample_plan_driver.cpp")]
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
    a, b = run(drivers[0], lines), run(drivers[1], lines)
    assert a == b
    return a


def test_plan_geometry_and_counts(drivers):
    ratios = rr.RATIOS + [(16000, 1000), (1024, 1), (1, 1024), (48000, 8000), (1023, 128), (1000, 67), (1023, 1024)]
    got = both(drivers, [("geom", i, o) for i, o in ratios] + [("geom", 16000, 16001), ("geom", 0, 5), ("geom", 1001, 1000)])
    for (i, o), v in zip(ratios, got):
        L, M, H, K = rr.geometry(i, o)
        span = -(-((TILE - 1) * M) // L) + K + 9
        span = (span + 7) // 8 * 8
        taps = (L * K + 7) // 8 * 8                                           # in LDS where table and samples fit 63 KiB
        lds = 0 if span > MAX_SPAN else 2 * span + (2 * taps if 2 * (span + taps) <= 63 * 1024 else 0)
        assert v == [0, L, M, H, K, int(span <= MAX_SPAN), span, lds] and lds <= 64 * 1024
        assert geometry_of(i, o) == (OK, L, M, K)
    assert [v[0] for v in got[len(ratios):]] == [2, 1, 2]
    assert all(v[5] == 1 for v in got[:len(rr.RATIOS)])                       # every listed ratio runs the staged kernel
    assert got[len(rr.RATIOS)][5] == 0                                        # 16 : 1 does not
    for i, o in rr.RATIOS:
        L, M, H, K = rr.geometry(i, o)
        cs = list(range(0, 3 * K + 1)) + [10 ** 9 + 7, (1 << 40) - 1]
        got = both(drivers, [("count", L, M, H, c) for c in cs])
        assert got == [[rr.count(c, L, M), rr.emitted(c, L, M, H)] for c in cs]


def one_shot(ratio, a_in, n, a_out):
    """a segment of the driver's plan request: in n out m0 m1 c0 hist hist_new"""
    L, M, H, K = rr.geometry(*ratio)
    return (a_in, n, a_out, 0, rr.count(n, L, M), 0, 0, 0)


def check_plan(ratio, segs, v):
    """a plan's answer against the invariants the kernel relies on"""
    L, M, H, K = rr.geometry(*ratio)
    span = (-(-((TILE - 1) * M) // L) + K + 9 + 7) // 8 * 8
    assert v[0] == 1
    n_tiles, seg_ll, tile_off, total, nbytes = v[1:6]
    assert seg_ll == tile_off == 8 * len(segs) and total == tile_off + 2 * n_tiles and nbytes == 8 * total + 64
    recs, tiles = v[6:6 + total], v[6 + total:]
    assert len(tiles) == 6 * n_tiles
    for s, sg in enumerate(segs):
        assert recs[8 * s:8 * s + 8] == list(sg)
    nxt = [0] * len(segs)                              # the next output of every segment, counted from its m0
    hist = [0] * len(segs)
    for i in range(n_tiles):
        s, t, ma, mb, base, groups = tiles[6 * i:6 * i + 6]
        assert recs[tile_off + 2 * i:tile_off + 2 * i + 2] == [s, t]
        a_in, n, a_out, m0, m1, c0, h_old, h_new = segs[s]
        if t == -1:                                    # the history tile: once, in front of the segment's other tiles
            assert h_new and not hist[s] and nxt[s] == 0
            hist[s] = 1
            continue
        n_out = m1 - m0
        assert ma == nxt[s] and ma < mb <= n_out and mb - ma <= TILE       # exactly once, in order, never empty
        nxt[s] = mb
        lead = (a_out // 2) % 8
        assert ma == max(t * TILE - lead, 0) and (mb == n_out or (a_out // 2 + mb) % 8 == 0)
        # every sample the tile's outputs read, the second dword of the last pair included, is staged; in samples of the
        # chunk: negative ones are history
        lo, hi = (m0 + ma) * M // L - H + 1 - c0, (m0 + mb - 1) * M // L + H + 2 - c0
        assert base <= lo and hi <= base + 8 * groups and 8 * groups <= span
        assert (a_in // 2 + base) % 8 == 0 and lo - base < 8                 # the 16-byte loads are aligned
        assert lo >= -(K - 1) or not c0                                       # nothing in front of the history
        assert hi - 2 <= n - 1 + H                                            # no output reads more than H zeros behind the chunk
    assert nxt == [sg[4] - sg[3] for sg in segs] and hist == [int(bool(sg[7])) for sg in segs]


def test_plan_tiles(drivers):
    rng = np.random.default_rng(5)
    lines, cases = [], []
    for ratio in rr.RATIOS + [(48000, 8000)]:
        L, M, H, K = rr.geometry(*ratio)
        n_for = lambda m: -(-m * M // L)              # the shortest input with at least m outputs
        lens = [0, 1, H, K + 1, n_for(TILE - 1), n_for(TILE), n_for(TILE + 1), n_for(2 * TILE + 3)]
        for lst in (lens, lens[::-1], [0, 0, 5, 0], [n_for(3 * TILE)], []):
            segs = [one_shot(ratio, 4096 * (s + 1) * 64 + 2 * int(rng.integers(0, 8)), n,
                             1 << 30 | 2 * int(rng.integers(0, 8)) + 65536 * s) for s, n in enumerate(lst)]
            lines.append(["plan", ratio[0], ratio[1], 0, 0, len(segs)] + [v for sg in segs for v in sg])
            cases.append((ratio, segs))
    for (ratio, segs), v in zip(cases, both(drivers, lines)):
        check_plan(ratio, segs, v)
    # every output offset against every input offset, one segment
    ratio = (44100, 16000)
    cases = [[one_shot(ratio, 1 << 20 | 2 * a, 6000, 1 << 24 | 2 * b)] for a in range(8) for b in range(8)]
    lines = [["plan", ratio[0], ratio[1], 0, 0, 1] + list(c[0]) for c in cases]
    for segs, v in zip(cases, both(drivers, lines)):
        check_plan(ratio, segs, v)


def test_plan_stream_segments(drivers):
    """the segments of a line's pushes and of its flush: chunk after chunk, the outputs E(c) .. E(c + n) with K - 1
    samples of history, the history tile, the flush on no chunk at all"""
    rng = np.random.default_rng(9)
    lines, cases = [], []
    for ratio in rr.RATIOS:
        L, M, H, K = rr.geometry(*ratio)
        c, segs = 0, []
        for n in [1, 0, H - 1, 1, K + 3, 5000, 1, 2 * TILE * M // L + 7]:
            if n:
                segs.append((1 << 20 | 2 * int(rng.integers(0, 8)), n, 1 << 30 | 2 * int(rng.integers(0, 8)),
                             rr.emitted(c, L, M, H), rr.emitted(c + n, L, M, H), c, (1 << 16) if c else 0, 1 << 17))
            c += n
        segs.append((0, 0, 1 << 30 | 6, rr.emitted(c, L, M, H), rr.count(c, L, M), c, 1 << 16, 0))       # the flush
        lines.append(["plan", ratio[0], ratio[1], 0, 0, len(segs)] + [v for sg in segs for v in sg])
        cases.append((ratio, segs))
    for (ratio, segs), v in zip(cases, both(drivers, lines)):
        check_plan(ratio, segs, v)


def test_plan_limits(drivers):
    seg = list(one_shot((8000, 16000), 1 << 20, 5000, 1 << 24))
    big = [1 << 20, 1 << 40, 1 << 24, 0, 1 << 41, 0, 0, 0]
    got = both(drivers, [["plan", 8000, 16000, 5001, 0, 1] + seg, ["plan", 8000, 16000, 5000, 0, 1] + seg,
                         ["plan", 8000, 16000, 0, 6, 1] + seg, ["plan", 8000, 16000, 0, 5, 1] + seg,
                         ["plan", 8000, 16000, 0, 0, 1] + big, ["plan", 8000, 16000, 0, 0, 1] + seg[:3] + [7, 6, 0, 0, 0]])
    assert [v[0] for v in got] == [1, 0, 1, 0, 0, 0] and got[0][1] == 5              # 10000 outputs: 5 tiles


def test_plan_driver_runs_the_rule(drivers):
    """the host form of the rule from the header alone (the sanitized build reads x only inside [0, n))"""
    rng = np.random.default_rng(11)
    for ratio in [(8000, 16000), (44100, 16000), (7, 5)]:
        L, M, H, K = rr.geometry(*ratio)
        t = mfcc_amd.resample_taps(*ratio)
        for n in (1, H, K + 1, 300):
            x = rng.integers(-32768, 32768, n)
            n_out = rr.count(n, L, M)
            got = both(drivers, [["run", ratio[0], ratio[1], 0, n_out, n] + list(x), ["run", ratio[0], ratio[1], n_out // 3, n_out, n] + list(x)])
            want = rr.resample(t, x, L, M)
            assert np.array_equal(got[0], want) and np.array_equal(got[1], want[n_out // 3:])
