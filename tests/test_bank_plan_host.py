"""What a stream bank's push, flush and reset decide from lengths and settings, on the CPU: mfcc_amd/csrc/bank_plan.hpp
has no HIP in it, so a few lines of C++ (tests/bank_plan_driver.cpp) print its layout and every record, and this test
holds them against the rules restated below -- N independent sessions (the Session of tests/test_stream_bank_host.py
with the frame count `seen` and the rows `held` back by the delta lag) -- and against invariants that do not depend on
the restatement.  The records name rows of device buffers: a slip here is an out-of-bounds write on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_stream_bank_host import Session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mfcc_amd", "csrc")

OK, INVALID, SMALL = 0, -101, -106                    # include/mfcc_hip.h
NO_EDGE = (1 << 63) - 1                               # mfcc_online::kNoEdge
UNSET, BLANK = 12345, -7777                           # the driver's fill of frame_offsets and of the descriptor block
REC_LL = dict(bank=5, gather=3, cmvn=8, delta=8, carry=8, pcen=5)
TABLES = list(REC_LL)                                 # the order of the tables in the block
N_STREAMS = 7

GEOMETRIES = [(512, 170), (1024, 341), (128, 1), (256, 256), (400, 160)]
# kind -> W, elem, S (CMVN run; 0: none), L (lag = order * window), order, g (rows per delta tile), PCEN.  S and g are
# numbers to the planner: small ones make pushes that span many runs and tiles
KINDS = {
    "plain":          dict(W=13, elem=4, S=0, L=0, order=0, g=0, pcen=0),
    "plain_fixed":    dict(W=13, elem=2, S=0, L=0, order=0, g=0, pcen=0),
    "cmvn":           dict(W=13, elem=4, S=4, L=0, order=0, g=0, pcen=0),
    "delta1":         dict(W=13, elem=4, S=0, L=2, order=1, g=3, pcen=0),
    "delta2":         dict(W=13, elem=4, S=0, L=4, order=2, g=5, pcen=0),
    "cmvn_delta2":    dict(W=13, elem=4, S=8, L=4, order=2, g=3, pcen=0),
    "pcen":           dict(W=32, elem=4, S=0, L=0, order=0, g=0, pcen=1),
    "pcen_cmvn_delta1": dict(W=32, elem=4, S=4, L=2, order=1, g=59, pcen=1),
}


def up256(b):
    return (b + 255) // 256 * 256


class Stream(Session):
    def __init__(self, nfft, hop):
        super().__init__(nfft, hop)
        self.seen = self.held = 0


class Bank:
    """The restated rules: what a bank of the kind `k` at frame length / hop `geo` does with a push or an end."""

    def __init__(self, geo, k):
        self.flen, self.hop = geo
        self.k = k
        self.norm, self.online = k["S"] > 0, bool(k["S"] or k["order"] or k["pcen"])
        self.post = bool(k["S"] or k["order"])
        self.wo = k["W"] * (1 + k["order"])
        self.streams = [Stream(*geo) for _ in range(N_STREAMS)]

    def settings(self):
        k = self.k
        return [self.flen, self.hop, k["W"], k["elem"], k["S"], k["L"], k["order"], k["g"], int(self.norm), k["pcen"]]

    def state(self):
        return [s.queued for s in self.streams] + [s.seen for s in self.streams] + [s.held for s in self.streams]

    def _passes(self, t, u, row0, seen, held, nf, rows, out_row, last):
        """records of the passes behind the frame launch for one stream: nf fresh rows, `rows` of them (and of the held
        ones) leave for out_row"""
        k = self.k
        if k["pcen"] and nf:
            t["pcen"].append((u, row0, seen, nf, row0 if self.post else out_row))
        if self.norm and nf:
            S = k["S"]
            for t0 in range(seen // S * S, seen + nf, S):          # runs of S rows in absolute frame numbers
                t["cmvn"].append((u, row0, seen, nf, t0, min(t0 + S, seen + nf), row0 if k["order"] else out_row, 0))
        if k["order"]:
            for i in range(0, rows, k["g"]):
                t["delta"].append((u, row0, seen, nf, seen - held + i, min(k["g"], rows - i), out_row + i, last))

    def _layout(self, t, n_active, nfmax, stride, lockstep, direct):
        k = self.k
        off, lay = 0, {}
        for name in TABLES:
            lay[name] = (off, len(t[name]))
            off += REC_LL[name] * len(t[name])
        rows = n_active * nfmax * k["W"] * k["elem"]
        rows_bytes = up256(rows) if self.online else (0 if direct else rows)
        raw_off = up256(off * 8)
        stat_off = raw_off + (rows_bytes if self.online else 0)
        lay.update(desc_ll=off, n_rec=len(t["bank"]), n_active=n_active, nfmax=nfmax, stride=stride, lockstep=int(lockstep),
                   direct=int(direct), in_bytes=n_active * stride * 2 + 256 if n_active else 0,
                   out_bytes=stat_off + rows_bytes + 64, raw_off=raw_off, stat_off=stat_off)
        return lay

    def push(self, lens, offsets, shift):
        """(frame_offsets, pending_after, held_after, raw_offsets, tables, layout); the sessions move on"""
        L = self.k["L"]
        before = [(s.queued, s.seen, s.held) for s in self.streams]
        nfs = [s.push(int(n)) for s, n in zip(self.streams, lens)]
        emitted = [max(0, s.held + nf - L) for s, nf in zip(self.streams, nfs)]
        fo = [0] + list(np.cumsum(emitted))
        active = [u for u in range(N_STREAMS) if lens[u] and nfs[u]]
        idle = [u for u in range(N_STREAMS) if lens[u] and not nfs[u]]
        nfmax = max([nfs[u] for u in active], default=0)
        t = {name: [] for name in TABLES}
        for u in active + idle:
            t["bank"].append((u, int(offsets[u]) - shift, int(lens[u]), before[u][0], nfs[u]))
        lockstep = bool(active) and len({nfs[u] for u in active}) == 1
        for a, u in enumerate(active):
            pending, seen, held = before[u]
            if not self.online:
                if not lockstep:                                    # a table has records exactly when its pass runs
                    t["gather"].append((a * nfmax, fo[u], nfs[u]))
                continue
            self._passes(t, u, a * nfmax, seen, held, nfs[u], emitted[u], fo[u], NO_EDGE)
            if self.post:                                           # into ring or tail
                t["carry"].append((u, a * nfmax, seen, nfs[u], 0, 0, 0, 0))
        stride = 1 + max([before[u][0] + int(lens[u]) for u in active], default=0)
        lay = self._layout(t, len(active), nfmax, stride, lockstep, lockstep and not self.online) if t["bank"] else None
        for s, nf, e in zip(self.streams, nfs, emitted):
            s.seen += nf
            s.held += nf - e
        return (fo, [s.queued for s in self.streams], [s.held for s in self.streams], [0] + list(np.cumsum(nfs)), t, lay)

    def end(self, lst, emit, give):
        """(frame_offsets, tables, layout); the listed sessions are back in the reset state"""
        nf = 1 if emit and give else 0
        rows = [self.streams[u].held + nf if give else 0 for u in lst]
        fo = [0] + list(np.cumsum(rows))
        t = {name: [] for name in TABLES}
        for i, u in enumerate(lst):
            s = self.streams[u]
            t["bank"].append((u, 0, 0, s.queued, nf))
            if self.online and rows[i]:
                self._passes(t, u, i * nf, s.seen, s.held, nf, rows[i], fo[i], s.seen + nf - 1)
        lay = self._layout(t, nf * len(lst), nf, self.flen + 1, True, not self.online) if lst else None
        for u in lst:
            self.streams[u].queued = self.streams[u].seen = self.streams[u].held = 0
        return fo, t, lay


def parse(line, n_fo, push):
    """A line of the driver: rc, frame_offsets, and after success the rest as a dict"""
    v = [int(x) for x in line.split()]
    rc, fo, v = v[0], v[1:1 + n_fo], v[1 + n_fo:]
    if rc != OK:
        assert not v
        return rc, fo, None
    got = {}
    if push:
        n = N_STREAMS
        got["pending_after"], got["held_after"], got["raw_offsets"], v = v[:n], v[n:2 * n], v[2 * n:3 * n + 1], v[3 * n + 1:]
    lay = {name: (v[2 * i], v[2 * i + 1]) for i, name in enumerate(TABLES)}
    names = ["desc_ll", "n_rec", "n_active", "nfmax", "stride", "lockstep", "direct", "in_bytes", "out_bytes", "raw_off",
             "stat_off"]
    lay.update(zip(names, v[12:23]))
    got["layout"], got["block"] = lay, v[23:]
    assert len(got["block"]) == (lay["desc_ll"] if lay["n_rec"] else 0)
    return rc, fo, got


def tables_of(lay, block):
    out = {}
    for name in TABLES:
        off, n = lay[name]
        w = REC_LL[name]
        out[name] = [tuple(block[off + i * w: off + (i + 1) * w]) for i in range(n)]
    return out


def check_invariants(bank, lay, t, fo, state, push, cover):
    """What must hold whatever the restatement says.  state: (pending, seen, held) per stream BEFORE the operation"""
    k = bank.k
    W, S, g = k["W"], k["S"], k["g"]
    # the tables: in order, disjoint, within the block and covering it
    off = 0
    for name in TABLES:
        assert lay[name][0] == off, name
        off += REC_LL[name] * lay[name][1]
    assert off == lay["desc_ll"]
    n_active, nfmax = lay["n_active"], lay["nfmax"]
    rec = t["bank"]
    assert len(rec) == lay["n_rec"] and len({r[0] for r in rec}) == len(rec)
    if push:                                           # active records first, both classes in stream order
        assert all(r[4] > 0 for r in rec[:n_active]) and all(r[4] == 0 and r[2] > 0 for r in rec[n_active:])
        assert [r[0] for r in rec[:n_active]] == sorted(r[0] for r in rec[:n_active])
        assert [r[0] for r in rec[n_active:]] == sorted(r[0] for r in rec[n_active:])
        assert all(1 + r[3] + r[2] <= lay["stride"] for r in rec[:n_active])          # the row of the work buffer holds it
        assert all(1 + r[3] + r[2] <= bank.flen for r in rec[n_active:])              # the state row does
        assert len(t["carry"]) == (n_active if bank.post else 0)
        assert len(t["gather"]) == (0 if bank.online or lay["lockstep"] else n_active)
        assert lay["direct"] == (lay["lockstep"] and not bank.online)
    else:
        assert not t["carry"] and not t["gather"]                                     # carry records: pushes only
        assert all(1 + r[3] <= lay["stride"] for r in rec)
    # rows of the work buffer's result
    for name in ("cmvn", "delta", "carry", "pcen"):
        for r in t[name]:
            assert r[1] + r[3] <= n_active * nfmax and r[1] % max(nfmax, 1) == 0, (name, r)
    assert all(r[0] + r[2] <= n_active * nfmax for r in t["gather"])
    # the final pass writes every returned row once
    total = fo[-1]
    if k["order"]:
        spans = [(r[6], r[6] + r[5]) for r in t["delta"]]
    elif S:
        spans = [(r[6] + max(r[4], r[2]) - r[2], r[6] + r[5] - r[2]) for r in t["cmvn"]]
    elif k["pcen"]:
        spans = [(r[4], r[4] + r[3]) for r in t["pcen"]]
    elif lay["direct"]:
        spans = [(a * nfmax, (a + 1) * nfmax) for a in range(n_active)]
    else:
        spans = [(r[1], r[1] + r[2]) for r in t["gather"]]
    spans = sorted(s for s in spans if s[0] != s[1])
    assert [s[0] for s in spans] == [0] * bool(spans) + [s[1] for s in spans[:-1]] and (spans[-1][1] if spans else 0) == total
    by_stream = lambda name: {u: [r for r in t[name] if r[0] == u] for u in {r[0] for r in t[name]}}
    # CMVN: the runs partition the fresh rows at multiples of S in absolute frame numbers
    for u, rs in by_stream("cmvn").items():
        seen, nf = rs[0][2], rs[0][3]
        assert seen == state[1][u] and nf > 0
        assert all(r[4] % S == 0 and seen - S < r[4] and r[5] == min(r[4] + S, seen + nf) for r in rs)
        assert [r[4] for r in rs[1:]] == [r[5] for r in rs[:-1]] and rs[0][4] <= seen < rs[0][5] and rs[-1][5] == seen + nf
        cover["run_before_seen"] += rs[0][4] < seen
        cover["runs3"] += len(rs) >= 3
    # deltas: the tiles partition the emitted rows in steps of g
    for u, rs in by_stream("delta").items():
        seen, held = state[1][u], state[2][u]
        assert rs[0][4] == seen - held and all(0 < r[5] <= g for r in rs) and all(r[5] == g for r in rs[:-1])
        assert [r[4] for r in rs[1:]] == [r[4] + r[5] for r in rs[:-1]]
        last = rs[0][7]
        assert all(r[7] == last for r in rs)
        if push:
            assert last == NO_EDGE and rs[-1][4] + rs[-1][5] + k["L"] <= seen + rs[0][3]     # no row past the fresh ones
        else:
            assert last == seen + rs[0][3] - 1 and rs[-1][4] + rs[-1][5] == last + 1
        cover["tiles2"] += len(rs) >= 2
    # the scratch covers every area the layout names
    rows_bytes = n_active * nfmax * W * k["elem"]
    assert lay["in_bytes"] >= n_active * lay["stride"] * 2
    assert lay["raw_off"] >= lay["desc_ll"] * 8 and lay["raw_off"] % 256 == 0 and lay["stat_off"] % 256 == 0
    if not lay["direct"]:
        assert lay["raw_off"] + rows_bytes <= lay["out_bytes"]
    if bank.online:
        assert lay["raw_off"] + rows_bytes <= lay["stat_off"] and lay["stat_off"] + rows_bytes <= lay["out_bytes"]
    assert lay["desc_ll"] * 8 <= lay["out_bytes"]


def schedule(bank, rng, emit):
    """about 200 rounds of pushes with flushes and resets of subsets in between: (kind of case, line, what to expect)"""
    flen, hop = bank.flen, bank.hop
    sizes = [0, 1, 2, 7, hop - 1, hop, hop + 1, flen - 1, flen, flen + 1, 3 * flen + 5]
    out = []
    for rnd in range(200):
        if rnd % 9 == 8:
            lst = [int(u) for u in rng.permutation(N_STREAMS)[:int(rng.integers(0, N_STREAMS + 1))]]
            give = int(rng.integers(3) > 0)
            state = bank.state()
            head = bank.settings() + [N_STREAMS, emit, give, 1, 1 << 40, len(lst)] + state + lst
            out.append(("end", head, state, (emit, give, lst), bank.end(lst, emit, give)))
            continue
        if rnd % 7 == 3:                                            # lockstep: one length for all
            lens = np.full(N_STREAMS, rng.choice(sizes[4:]))
            for s in bank.streams:                                  # ... from one state
                s.queued = bank.streams[0].queued
        else:
            lens = rng.choice(sizes, N_STREAMS)
        if rnd % 17 == 0:
            lens[rng.integers(N_STREAMS)] = int(rng.integers(0, 5 * flen))
        if rnd % 23 == 5:
            lens[:] = 0
        offsets = np.zeros(N_STREAMS + 1, dtype=np.int64)
        offsets[0] = int(rng.integers(0, 100))                      # the chunks need not start at sample 0 of the buffer
        offsets[1:] = offsets[0] + np.cumsum(lens)
        shift = int(rng.integers(0, offsets[0] + 1))
        state = bank.state()
        head = bank.settings() + [N_STREAMS, 1, 1, 1 << 40, shift] + state + [int(o) for o in offsets]
        out.append(("push", head, state, lens, bank.push(lens, offsets, shift)))
    return out


def refusals():
    """(line, n_fo, rc, frame_offsets expected; None where the plan did not get to)"""
    bank = Bank((512, 170), KINDS["cmvn_delta2"])
    n = N_STREAMS
    zeros = [0] * n
    good = [0, 600, 1300, 1300, 2000, 4380, 4480, 5080]             # frames 1 2 0 2 11 0 1; lag 4: returned 0 0 0 0 7 0 0
    fo_good = [0, 0, 0, 0, 0, 7, 7, 7]
    assert [(b - a - 512) // 170 + 1 if b - a >= 512 else 0 for a, b in zip(good, good[1:])] == [1, 2, 0, 2, 11, 0, 1]

    def push(pending, held, offsets, samples=1, out=1, cap=1 << 40):
        return ["push"] + bank.settings() + [n, samples, out, cap, 0] + pending + zeros + held + offsets

    cases = []
    dec = list(good)
    dec[6] = 4000                                                   # stream 5's chunk ends before it begins
    cases.append((push(zeros, zeros, dec), n + 1, INVALID, fo_good[:6] + [None] * 2))
    cases.append((push(zeros, zeros, dec, cap=0), n + 1, INVALID, fo_good[:6] + [None] * 2))      # ... before BUFFER_SMALL
    cases.append((push([0, 0, 512] + [0] * 4, zeros, good), n + 1, INVALID, [0, 0, 0] + [None] * 5))
    cases.append((push([0, 0, 511] + [0] * 4, zeros, good), n + 1, OK, None))
    cases.append((push(zeros, [0, 0, 0, 5, 0, 0, 0], good), n + 1, INVALID, [0, 0, 0, 0] + [None] * 4))
    wo = bank.wo
    cases.append((push(zeros, zeros, good, cap=7 * wo - 1), n + 1, SMALL, fo_good))
    cases.append((push(zeros, zeros, good, cap=7 * wo), n + 1, OK, fo_good))
    cases.append((push(zeros, zeros, good, out=0), n + 1, SMALL, fo_good))
    cases.append((push(zeros, zeros, good, samples=0, out=0), n + 1, SMALL, fo_good))             # ... before the samples
    cases.append((push(zeros, zeros, good, samples=0), n + 1, INVALID, fo_good))
    cases.append((push(zeros, zeros, [40] * (n + 1), samples=0, out=0, cap=0), n + 1, OK, [0] * (n + 1)))   # no work
    few = [0, 600, 1200, 1200, 1200, 1200, 1200, 1200]              # samples, but no row returned: no buffer needed
    cases.append((push(zeros, zeros, few, out=0, cap=0), n + 1, OK, [0] * (n + 1)))

    def end(held, lst, emit=1, give=1, out=1, cap=1 << 40):
        return ["end"] + bank.settings() + [n, emit, give, out, cap, len(lst)] + zeros + [9] * n + held + lst

    held = [4, 0, 2, 0, 0, 1, 0]
    cases.append((end(held, [2, 0, 5], cap=10 * wo - 1), 4, SMALL, [0, 3, 8, 10]))
    cases.append((end(held, [2, 0, 5], cap=10 * wo), 4, OK, [0, 3, 8, 10]))
    cases.append((end(held, [2, 0, 5], out=0), 4, SMALL, [0, 3, 8, 10]))
    cases.append((end(held, [2, 0, 5], emit=0, cap=7 * wo - 1), 4, SMALL, [0, 2, 6, 7]))
    cases.append((end(held, [1, 3], emit=0, out=0, cap=0), 3, OK, [0, 0, 0]))                     # nothing held, no tail frame
    cases.append((end(held, [2, 0, 5], emit=0, give=0, out=0, cap=0), 4, OK, [0, 0, 0, 0]))       # a reset returns nothing
    cases.append((end(held, [], out=0, cap=0), 1, OK, [0]))
    return cases


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no g++ or clang++")
    d = tmp_path_factory.mktemp("bank_plan")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "bank_plan_driver.cpp")]
    subprocess.run(base + ["-O1", "-o", str(d / "driver")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "driver_san")],
                   check=True)
    return str(d / "driver"), str(d / "driver_san")


@pytest.fixture(scope="module")
def scheduled():
    """every schedule once: [(bank, [case, ...])] and the driver's input"""
    runs = []
    for gi, geo in enumerate(GEOMETRIES):
        for ki, (name, k) in enumerate(KINDS.items()):
            bank = Bank(geo, k)
            rng = np.random.default_rng(geo[0] * 1000 + geo[1] * 10 + ki)
            runs.append((name, bank, schedule(bank, rng, emit=(gi + ki) % 2)))
    text = "".join(" ".join(str(v) for v in [c[0]] + c[1]) + "\n" for _, _, cases in runs for c in cases)
    return runs, text


def test_header_has_no_hip():
    src = open(os.path.join(CSRC, "bank_plan.hpp")).read()
    assert "hip/" not in src and "__device__" not in src and "__global__" not in src
    for name in ("kernel_stream_bank.hpp", "kernel_stream_bank_online.hpp", "kernel_pcen.hpp"):
        assert '#include "bank_plan.hpp"' in open(os.path.join(CSRC, name)).read(), name


def test_records_and_layout_equal_the_restatement(drivers, scheduled):
    runs, text = scheduled
    lines = subprocess.run([drivers[0]], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == sum(len(cases) for _, _, cases in runs)
    cover = dict.fromkeys(["lockstep", "mixed", "no_frame", "idle_next_to_active", "nothing", "run_before_seen", "runs3", "tiles2",
                           "flush_held_lag", "flush_held_0", "reset", "flush_no_tail", "shifted"], 0)
    it = iter(lines)
    for name, bank, cases in runs:
        L = bank.k["L"]
        for kind, head, state, arg, want in cases:
            st = (state[:N_STREAMS], state[N_STREAMS:2 * N_STREAMS], state[2 * N_STREAMS:])
            push = kind == "push"
            rc, fo, got = parse(next(it), N_STREAMS + 1 if push else len(arg[2]) + 1, push)
            assert rc == OK, (name, head)
            if push:
                w_fo, w_pa, w_ha, w_rfo, w_t, w_lay = want
                assert (fo, got["pending_after"], got["held_after"], got["raw_offsets"]) == (w_fo, w_pa, w_ha, w_rfo), (name, head)
            else:
                w_fo, w_t, w_lay = want
                assert fo == w_fo, (name, head)
            lay = got["layout"]
            if w_lay is None:
                assert lay["n_rec"] == 0 and not got["block"]
                cover["nothing"] += 1
                continue
            assert lay == w_lay, (name, head, lay, w_lay)
            assert BLANK not in got["block"]
            t = tables_of(lay, got["block"])
            assert t == w_t, (name, head)
            check_invariants(bank, lay, t, fo, st, push, cover)
            if push:
                cover["lockstep"] += lay["lockstep"] and lay["n_active"] > 1
                cover["mixed"] += lay["n_active"] > 1 and not lay["lockstep"]
                cover["no_frame"] += lay["n_active"] == 0
                cover["idle_next_to_active"] += 0 < lay["n_active"] < lay["n_rec"]
                cover["shifted"] += head[len(bank.settings()) + 4] > 0
            else:
                emit, give, lst = arg
                cover["reset"] += not give
                cover["flush_no_tail"] += bool(give and not emit and fo[-1])
                if give and L:
                    cover["flush_held_lag"] += any(st[2][u] == L for u in lst)
                    cover["flush_held_0"] += any(st[2][u] == 0 for u in lst)
    assert all(cover.values()), cover


def test_refusals_keep_their_precedence(drivers):
    cases = refusals()
    text = "".join(" ".join(str(v) for v in c[0]) + "\n" for c in cases)
    lines = subprocess.run([drivers[0]], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for (case, n_fo, want_rc, want_fo), line in zip(cases, lines):
        rc, fo, got = parse(line, n_fo, case[0] == "push")
        assert rc == want_rc, case
        if want_fo is not None:                                     # filled up to the offending stream, and no further
            assert fo == [UNSET if v is None else v for v in want_fo], (case, fo)
        assert (got is not None) == (rc == OK)


def test_driver_runs_clean_under_the_sanitizers(drivers, scheduled):
    """the same input through the driver built with -fsanitize=address,undefined, as a program of its own: a record
    written past its table's end, or past the block's, ends it"""
    text = scheduled[1] + "".join(" ".join(str(v) for v in c[0]) + "\n" for c in refusals())
    plain = subprocess.run([drivers[0]], input=text, capture_output=True, text=True, check=True)
    san = subprocess.run([drivers[1]], input=text, capture_output=True, text=True)
    assert san.returncode == 0, san.stderr[-2000:]
    assert san.stdout == plain.stdout
