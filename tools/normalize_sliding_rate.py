"""Cost of sliding-window normalization (MFCC(normalize="meanvar", normalize_window=600)) against the per-segment
passes on the same rows, and the end-to-end cost of such a handle over a raw one.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/normalize_sliding_rate.py [--iters I] [--rounds R]

config2: 64 x 9.6 M samples, 512/170/32, 13 cepstra (dense, process_i16_dev).  config5: 10 000 utterances of five
lengths (160 000 - 997 * (u % 5) samples) on the ragged device path (process_ragged_i16_dev).
For each config the raw rows are made once, then I calls each of normalize_rows(window=600, min_window=100, centered)
-- normalize_sliding_kernel -- and of the in-place per-segment normalize_rows -- normalize_stats_kernel,
normalize_finalize_kernel, normalize_apply_kernel -- run on them, so that the profiler's kernel statistics hold both on
the same rows in the same process; the yardstick is the sum of the three.  The raw, per-segment MEAN_VAR and windowed
MEAN_VAR handles are also timed in turn (HIP events around back-to-back calls, median of R rounds); under the profiler
those figures carry its overhead.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mfcc_amd  # noqa: E402

KW = dict(nfft=512, nfilters=32, nceptrums=13)
WIN = dict(normalize_window=600, normalize_min_window=100, normalize_center=True)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(calls, rounds, iters):
    for f in calls.values():                          # warm-up: clocks up, code, tables and scratch resident
        timed(f, 3)
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            ms[k].append(timed(f, iters))
    return {k: dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))
            for k, v in ms.items()}


def run(handles, produce, sliding_pass, segment_pass, rows, rounds, iters):
    raw, seg, win = handles
    res = {"rows": int(rows.numel() // rows.shape[-1]), "width": int(rows.shape[-1])}
    res.update(measure({"off": lambda: produce(raw), "meanvar": lambda: produce(seg), "meanvar_window": lambda: produce(win),
                        "sliding_pass": sliding_pass, "segment_passes": segment_pass}, rounds, iters))
    res["window_overhead_pct"] = round(100 * (res["meanvar_window"]["ms"] / res["off"]["ms"] - 1), 2)
    res["segment_overhead_pct"] = round(100 * (res["meanvar"]["ms"] / res["off"]["ms"] - 1), 2)
    res["pass_ratio"] = round(res["sliding_pass"]["ms"] / res["segment_passes"]["ms"], 3)
    for h in handles:
        h.close()
    return res


def handles():
    return mfcc_amd.MFCC(**KW), mfcc_amd.MFCC(normalize="meanvar", **KW), mfcc_amd.MFCC(normalize="meanvar", **WIN, **KW)


def config2(rounds, iters, nch=64, n=9_600_000):
    g = torch.Generator(device="cuda").manual_seed(0)
    pcm = (torch.randn((nch, n), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    hs = handles()
    rows = hs[0].process(pcm)
    work, out = rows.clone(), torch.empty_like(rows)
    res = run(hs, lambda h: h.process(pcm, out=out),
              lambda: hs[0].normalize_rows(rows, window=600, min_window=100, center=True, out=out),
              lambda: hs[0].normalize_rows(work), rows, rounds, iters)
    return res


def config5(rounds, iters, n_utt=10_000, n=160_000):
    lens = [n - 997 * (u % 5) for u in range(n_utt)]
    offs = np.zeros(n_utt + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    g = torch.Generator(device="cuda").manual_seed(0)
    flat = (torch.randn(int(offs[-1]), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    hs = handles()
    rows, fo = hs[0].process_packed(flat, offs)
    work, out = rows.clone(), torch.empty_like(rows)
    return run(hs, lambda h: h.process_packed(flat, offs, out=out),
               lambda: hs[0].normalize_rows(rows, fo, window=600, min_window=100, center=True, out=out),
               lambda: hs[0].normalize_rows(work, fo), rows, rounds, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    line = {"metric": "normalize_sliding_rate", "device": torch.cuda.get_device_name(0)}
    line["config2"] = config2(a.rounds, a.iters)
    torch.cuda.empty_cache()
    line["config5"] = config5(a.rounds, a.iters)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
