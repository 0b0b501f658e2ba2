"""Every route of the stream bank's one push and one end function (mfcc_amd/csrc/bank_plan.hpp, bank_advance / bank_end
in mfcc_hip.hip), at the smallest shape that tells them apart: which area of the scratch the frame launch writes, which
record table each pass reads, which rows leave for the caller.  The arithmetic itself is held on the CPU
(tests/test_bank_plan_host.py); this file is wrong only if a route picks the wrong area or table.

One schedule per bank kind and framing, through both entry points.  The first push holds every record class at once: a
stream without samples, one that only accumulates, one that completes exactly one frame and two that complete
different larger counts (a mixed push: a plain bank gathers).  Then a lockstep push (a plain bank's frame launch
writes the caller's rows itself) in which one stream's fresh rows start inside a CMVN run and span three, a flush of
two streams, a push to every stream, a reset of one, a push, and the flush of everything.

The reference is the bank-less one: the one-shot call on each stream's concatenated samples, then the direct
``pcen_rows`` / ``normalize_rows`` / ``deltas_rows`` entries.  Bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_families as kf
import online_ref as on
from kernel_families import open_handle, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADS = ["notebook", "stream"]
PCEN = dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6)
WINDOW = 40
CMVN = dict(normalize="meanvar", normalize_window=WINDOW)
# kind -> (family, MFCC() keywords, stream_bank() keywords)
KINDS = {
    "plain":           ("f512", {}, {}),
    "plain_fixed":     ("x512", {}, dict(fixed=True)),
    "cmvn":            ("f512", {}, CMVN),
    "delta1":          ("f512", {}, dict(deltas=1, delta_window=2)),
    "delta2":          ("f512", {}, dict(deltas=2, delta_window=2)),
    "cmvn_delta2":     ("f512", {}, dict(deltas=2, delta_window=2, **CMVN)),
    "pcen":            ("f512", dict(output="logmel"), dict(pcen=PCEN)),
    "pcen_cmvn_delta1": ("f512", dict(output="logmel"), dict(pcen=PCEN, deltas=1, delta_window=2, **CMVN)),
}
N = 5
NFFT, HOP = 512, 170


def run_rows(window):
    """mfcc_slide::run_rows, read from the header"""
    src = open(os.path.join(ROOT, "mfcc_amd", "csrc", "kernel_normalize_sliding.hpp")).read()
    body = re.search(r"inline int run_rows\(int window\) \{(.*?)\n\}", src, flags=re.S).group(1)
    div = int(re.search(r"const int s = window / (\d+);", body).group(1))
    lo, hi = (int(v) for v in re.search(r"return s < (\d+) \? \1 : \(s > (\d+) \? \2 : s\);", body).groups())
    return min(max(window // div, lo), hi)


def frames_for(pending, n_frames, extra):
    """samples that complete ``n_frames`` frames on top of ``pending`` ones, and ``extra`` < hop more"""
    return NFFT + (n_frames - 1) * HOP - pending + extra


# the schedule: ("push", lengths) / ("flush", streams) / ("reset", streams); the lockstep push is filled in below
FIRST = [0, 300, frames_for(0, 1, 50), frames_for(0, 30, 60), frames_for(0, 7, 11)]
LOCK_FRAMES = 36


def schedule():
    model = on.Model(on.BY_ID["f512"], N, 0)
    model.push(FIRST)
    lock = [frames_for(q, LOCK_FRAMES, 3 + 20 * u) for u, q in enumerate(model.queued)]
    assert model.push(lock) == [LOCK_FRAMES] * N
    return [("push", FIRST), ("push", lock), ("flush", [3, 1]), ("push", [900, 2500, 1300, 3100, 600]), ("reset", [2]),
            ("push", [0, 800, 1500, 0, 4000]), ("flush", None)]


def test_the_schedule_holds_every_route():
    S = run_rows(WINDOW)
    ops = schedule()
    model = on.Model(on.BY_ID["f512"], N, 0)
    nf = model.push(ops[0][1])
    assert nf[0] == 0 and ops[0][1][0] == 0 and nf[1] == 0 and ops[0][1][1] > 0 and nf[2] == 1      # every record class
    assert nf[3] > 1 and nf[4] > 1 and nf[3] != nf[4]                                               # mixed
    seen = nf[3]
    assert seen % S and (seen + LOCK_FRAMES - 1) // S - seen // S + 1 >= 3       # inside a run, and over three of them
    assert model.push(ops[1][1]) == [LOCK_FRAMES] * N                            # lockstep
    for u in ops[2][1]:
        model.queued[u] = 0
    nf = model.push(ops[3][1])
    assert all(ops[3][1]) and len(set(nf)) > 2
    assert max(max(op[1]) for op in ops if op[0] == "push") < 7000


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def lives(ops, xs):
    """Per stream, the spans of its samples between two ends: [(first sample, last + 1, how it ended)]"""
    pos, start, out = [0] * N, [0] * N, [[] for _ in range(N)]
    for op, arg in ops:
        if op == "push":
            pos = [p + k for p, k in zip(pos, arg)]
            continue
        for u in range(N) if arg is None else arg:
            out[u].append((start[u], pos[u], op))
            start[u] = pos[u]
    assert pos == [len(x) for x in xs] and start == pos
    return out


@pytest.fixture(scope="module")
def signals(wav_pcm):
    total = [sum(arg[u] for op, arg in schedule() if op == "push") for u in range(N)]
    kinds = ["speech", "noise", "uniform", "silences", "speech"]
    return [kf.signal(k, n, 40 + u, wav_pcm) for u, (k, n) in enumerate(zip(kinds, total))]


@pytest.fixture(scope="module")
def raw_rows(mfcc_amd, signals):
    """The one-shot rows of every life of every stream, per (family, handle keywords, framing): computed once"""
    cache = {}

    def get(fid, kw, pad):
        key = (fid, tuple(sorted(kw.items())), pad)
        if key not in cache:
            fam = on.BY_ID[fid]
            with open_handle(mfcc_amd, fam, pad, **kw) as m:
                cache[key] = [[(kf.run(m, fam, x[a:b]), how) for a, b, how in spans]
                              for x, spans in zip(signals, lives(schedule(), signals))]
        return cache[key]
    return get


def reference(m, raw, bank_kw):
    """What the bank-less library makes of one life's raw rows: PCEN, the causal CMVN, the deltas, by the direct entries"""
    import torch
    if not set(bank_kw) - {"fixed"} or not len(raw):
        return raw
    rows = torch.from_numpy(raw).cuda()
    if "pcen" in bank_kw:
        rows = m.pcen_rows(rows, **PCEN)
    if "normalize" in bank_kw:
        rows = m.normalize_rows(rows, mode=bank_kw["normalize"], window=bank_kw["normalize_window"], min_window=1, center=False)
    if bank_kw.get("deltas"):
        rows = m.deltas_rows(rows, order=bank_kw["deltas"], window=bank_kw["delta_window"])
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def push_host(lib, bank, chunks, shift):
    """mfcc_hip_bank_push with host arrays whose first chunk does not start at sample 0 of the buffer"""
    lens = [len(c) for c in chunks]
    offsets = (shift + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    flat = np.concatenate([np.full(shift, 12345, np.int16)] + chunks)
    nf = int(bank.num_frames(lens)[-1])
    out = np.full((nf, bank.num_features), 99, np.int16 if bank.fixed else np.float32)
    fo = np.zeros(N + 1, np.uint64)
    assert lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(offsets), _ptr(out), out.size, _ptr(fo)) == 0
    assert int(fo[-1]) == nf
    return [out[int(fo[u]):int(fo[u + 1])] for u in range(N)]


def push_device(lib, bank, chunks, shift):
    import torch
    lens = [len(c) for c in chunks]
    offsets = (shift + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    flat = torch.from_numpy(np.concatenate([np.full(shift, 12345, np.int16)] + chunks + [np.zeros(8, np.int16)])).cuda()
    out, fo = bank.push_packed(flat, offsets)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return [o[int(fo[u]):int(fo[u + 1])] for u in range(N)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_route_gives_the_one_shot_rows(mfcc_amd, signals, raw_rows, kind, pad):
    fid, handle_kw, bank_kw = KINDS[kind]
    fam = on.BY_ID[fid]
    lib = mfcc_amd.load_library()
    ops = schedule()
    with open_handle(mfcc_amd, fam, pad, **handle_kw) as m:
        want = [[(reference(m, raw, bank_kw), how) for raw, how in life] for life in raw_rows(fid, handle_kw, pad)]
        for name, push in (("host", push_host), ("device", push_device)):
            with m.stream_bank(N, **bank_kw) as bank:
                assert bank.lag == on.lag_of(bank_kw) and bank.online == bool(set(bank_kw) - {"fixed"})
                got, life, pos = [[] for _ in range(N)], [0] * N, [0] * N
                for k, (op, arg) in enumerate(ops):
                    if op == "push":
                        chunks = [x[p:p + n] for x, p, n in zip(signals, pos, arg)]
                        pos = [p + n for p, n in zip(pos, arg)]
                        for u, r in enumerate(push(lib, bank, chunks, shift=37 + k)):
                            got[u].append(r)
                        continue
                    lst = list(range(N)) if arg is None else arg
                    tails = bank.flush(arg) if op == "flush" else (bank.reset(arg) or [None] * len(lst))
                    for u, tail in zip(lst, tails):
                        one, how = want[u][life[u]]
                        assert how == op
                        if op == "flush":
                            assert same(on.cat(got[u] + [tail], one), one), (kind, pad, name, u, k)
                        else:                                      # a reset: what it had returned is the head of those rows
                            rows = on.cat(got[u], one)
                            assert len(rows) and same(rows, one[:len(rows)]), (kind, pad, name, u, k)
                        got[u], life[u] = [], life[u] + 1
                    assert not bank.pending[lst].any() and not bank.held[lst].any()
                assert life == [len(w) for w in want] and not any(got)
