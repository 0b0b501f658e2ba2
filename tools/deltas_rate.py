"""Rate of the delta pass (MFCC(deltas=2), deltas_kernel) against normalization's apply pass on the same static rows,
and the end-to-end cost of an order-2 handle over a raw one.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/deltas_rate.py [--iters I] [--rounds R]

config2: 64 x 9.6 M samples, 512/170/32, 13 cepstra (dense, process_i16_dev).  config5: 10 000 utterances of five
lengths (160 000 - 997 * (u % 5) samples) on the ragged device path (process_ragged_i16_dev).
For each config the static rows are made once, then I calls each of deltas_rows(order 2, window 2) and of
normalize_rows (stats, finalize and apply) run on them, so that the profiler's kernel statistics hold both kernels on
the same rows in the same process.  Rate = algorithmic bytes over kernel time: 4W read + 4W(1 + K) written per row for
the delta pass, 4W read + 4W written for apply (tools/deltas_rate_summary.py reads the rocprofv3 statistics).  The raw
and order-2 handles are also timed in turn (HIP events around back-to-back calls, median of R rounds); under the
profiler those figures carry its overhead.  Prints one JSON line."""
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


def run(raw, m, produce, deltas_pass, normalize_pass, rows, rounds, iters):
    res = {"rows": int(rows.shape[0] if rows.dim() == 2 else rows.shape[0] * rows.shape[1]),
           "width": int(rows.shape[-1])}
    res.update(measure({"off": lambda: produce(raw), "order2": lambda: produce(m), "delta_pass": deltas_pass,
                        "normalize_passes": normalize_pass}, rounds, iters))
    res["overhead_pct"] = round(100 * (res["order2"]["ms"] / res["off"]["ms"] - 1), 2)
    return res


def config2(rounds, iters, nch=64, n=9_600_000):
    g = torch.Generator(device="cuda").manual_seed(0)
    pcm = (torch.randn((nch, n), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    raw, m = mfcc_amd.MFCC(**KW), mfcc_amd.MFCC(deltas=2, **KW)
    nf = raw.num_frames(n)
    rows = raw.process(pcm)
    work = rows.clone()
    out = torch.empty((nch, nf, 13), device="cuda")
    out3 = torch.empty((nch, nf, 39), device="cuda")
    res = run(raw, m, lambda h: h.process(pcm, out=out if h is raw else out3),
              lambda: m.deltas_rows(rows, order=2, window=2, out=out3),
              lambda: m.normalize_rows(work), rows, rounds, iters)
    res["kernel"] = m.kernel_name()
    raw.close()
    m.close()
    return res


def config5(rounds, iters, n_utt=10_000, n=160_000):
    lens = [n - 997 * (u % 5) for u in range(n_utt)]
    offs = np.zeros(n_utt + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    g = torch.Generator(device="cuda").manual_seed(0)
    flat = (torch.randn(int(offs[-1]), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    raw, m = mfcc_amd.MFCC(**KW), mfcc_amd.MFCC(deltas=2, **KW)
    rows, fo = raw.process_packed(flat, offs)
    work = rows.clone()
    out = torch.empty_like(rows)
    out3 = torch.empty((rows.shape[0], 39), device="cuda")
    res = run(raw, m, lambda h: h.process_packed(flat, offs, out=out if h is raw else out3),
              lambda: m.deltas_rows(rows, fo, order=2, window=2, out=out3),
              lambda: m.normalize_rows(work, fo), rows, rounds, iters)
    raw.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    line = {"metric": "deltas_rate", "device": torch.cuda.get_device_name(0)}
    line["config2"] = config2(a.rounds, a.iters)
    torch.cuda.empty_cache()
    line["config5"] = config5(a.rounds, a.iters)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
