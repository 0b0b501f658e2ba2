"""Cost of per-segment normalization (MFCC(normalize="meanvar")), same process, same input, timed in turn.

    python tools/normalize_rate.py [--rounds R] [--iters I]

config2: 64 x 9.6 M samples, 512/170/32, 13 cepstra (dense, process_i16_dev).  config5: 10 000 utterances of five
lengths (160 000 - 997 * (u % 5) samples) on the ragged device path (process_ragged_i16_dev).
For each config: a raw handle and a MEAN_VAR handle, timed alternately R rounds of I calls (HIP events around
back-to-back calls on one stream), median round; and the two passes alone (normalize_rows on the resident rows),
reported as effective TB/s over 2 reads + 1 write of the rows.  Prints one JSON line."""
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


def measure(calls, rows_bytes, frames, rounds, iters):
    for f in calls.values():                          # warm-up: clocks up, code, tables and scratch resident
        timed(f, 3)
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            ms[k].append(timed(f, iters))
    res = {"frames": frames, "rows_MB": round(rows_bytes / 1e6, 1)}
    for k in calls:
        med = statistics.median(ms[k])
        res[k] = dict(ms=round(med, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4))
    res["overhead_pct"] = round(100 * (res["meanvar"]["ms"] / res["off"]["ms"] - 1), 2)
    res["passes_TBps"] = round(3 * rows_bytes / (res["passes_only"]["ms"] * 1e-3) / 1e12, 3)
    return res


def config2(rounds, iters, nch=64, n=9_600_000):
    g = torch.Generator(device="cuda").manual_seed(0)
    pcm = (torch.randn((nch, n), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    raw, m = mfcc_amd.MFCC(**KW), mfcc_amd.MFCC(normalize="meanvar", **KW)
    nf = raw.num_frames(n)
    out = torch.empty((nch, nf, 13), device="cuda")
    rows = torch.empty_like(out)
    raw.process(pcm, out=rows)
    calls = {"off": lambda: raw.process(pcm, out=out), "meanvar": lambda: m.process(pcm, out=out),
             "passes_only": lambda: m.normalize_rows(rows)}
    res = measure(calls, rows.numel() * 4, nf * nch, rounds, iters)
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
    raw, m = mfcc_amd.MFCC(**KW), mfcc_amd.MFCC(normalize="meanvar", **KW)
    out, fo = raw.process_packed(flat, offs)
    rows = out.clone()
    calls = {"off": lambda: raw.process_packed(flat, offs, out=out),
             "meanvar": lambda: m.process_packed(flat, offs, out=out),
             "passes_only": lambda: m.normalize_rows(rows, fo)}
    res = measure(calls, rows.numel() * 4, int(fo[-1]), rounds, iters)
    raw.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    line = {"metric": "normalize_rate", "device": torch.cuda.get_device_name(0)}
    line["config2"] = config2(a.rounds, a.iters)
    torch.cuda.empty_cache()
    line["config5"] = config5(a.rounds, a.iters)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
