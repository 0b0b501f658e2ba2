"""Cost of PCEN (MFCC(output="logmel", pcen=...)), same process, same input, timed in turn.

    python tools/pcen_rate.py [--rounds R] [--iters I] > LINE
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o pcen -- python tools/pcen_rate.py --passes-only > LINE2
    python tools/pcen_rate.py --summarize OUT/.../pcen_kernel_trace.csv

corpus   the headline corpus shape: 10 000 utterances of five lengths (160 000 - 997 * (u % 5) samples, DESIGN.md
         section 6b), 512/170/32 log-mel rows, on the ragged device path: a raw handle and a PCEN handle, and the passes
         alone on the resident rows -- PCEN (pcen_rows) next to per-segment normalization (normalize_rows, meanvar), which
         also reads the rows twice and writes them once: the yardstick.
long     64 channels x 1 h at hop 160 (360 000 frames) of 40-wide rows: the same two passes alone.
online   one tick of 4096 lines in lockstep, one hop each: a bank with PCEN next to the plain bank.
R rounds of I calls, HIP events around back-to-back calls on one stream, the median round; GB/s counts 2 reads + 1 write
of the rows.  --summarize: time of each PCEN kernel of a kernel trace per (kernel, grid size).  One JSON line."""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(nfft=512, nfilters=32, nceptrums=13, output="logmel")
NFFT, HOP = 512, 170
WARM = 3


def timed(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(torch, calls, rows_bytes, rounds, iters):
    for f in calls.values():                          # warm-up: clocks up, code, tables and scratch resident
        timed(torch, f, WARM)
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            ms[k].append(timed(torch, f, iters))
    res = {"rows_MB": round(rows_bytes / 1e6, 1)}
    for k in calls:
        med = statistics.median(ms[k])
        res[k] = dict(us=round(med * 1e3, 1), us_min=round(min(ms[k]) * 1e3, 1), us_max=round(max(ms[k]) * 1e3, 1))
        if k.endswith("_passes"):
            res[k]["GBps"] = round(3 * rows_bytes / (med * 1e-3) / 1e9, 1)
    return res


def corpus(torch, mfcc_amd, rounds, iters, passes_only, n_utt=10_000, n=160_000):
    lens = [n - 997 * (u % 5) for u in range(n_utt)]
    offs = np.zeros(n_utt + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    g = torch.Generator(device="cuda").manual_seed(0)
    flat = (torch.randn(int(offs[-1]), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    with mfcc_amd.MFCC(**KW) as raw, mfcc_amd.MFCC(pcen=True, **KW) as m:
        out, fo = raw.process_packed(flat, offs)
        rows = out.clone()
        work = rows.clone()

        def pcen_passes():                            # in place on log2 energies every time
            work.copy_(rows)
            raw.pcen_rows(work, fo)

        def norm_passes():
            work.copy_(rows)
            raw.normalize_rows(work, fo)
        calls = {"copy": lambda: work.copy_(rows), "pcen_passes": pcen_passes, "meanvar_passes": norm_passes}
        if not passes_only:
            calls.update(off=lambda: raw.process_packed(flat, offs, out=out),
                         pcen=lambda: m.process_packed(flat, offs, out=out))
        res = measure(torch, calls, rows.numel() * 4, rounds, iters)
        res["frames"] = int(fo[-1])
        res["kernel"] = m.kernel_name()
    return net_of_copy(res)


def long_channels(torch, mfcc_amd, rounds, iters, nch=64, frames=360_000, width=40):
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.rand((nch, frames, width), device="cuda", generator=g) * 30 - 8
    work = torch.empty_like(rows)
    with mfcc_amd.MFCC(**KW) as raw:
        def pcen_passes():
            work.copy_(rows)
            raw.pcen_rows(work)

        def norm_passes():
            work.copy_(rows)
            raw.normalize_rows(work)
        calls = {"copy": lambda: work.copy_(rows), "pcen_passes": pcen_passes, "meanvar_passes": norm_passes}
        res = measure(torch, calls, rows.numel() * 4, rounds, iters)
    res["frames"] = nch * frames
    return net_of_copy(res)


def net_of_copy(res):
    """The passes are timed behind a copy that restores their input: take the copy's median off."""
    c = res["copy"]["us"]
    rows_bytes = res["rows_MB"] * 1e6
    for k in ("pcen_passes", "meanvar_passes"):
        net = res[k]["us"] - c
        res[k].update(us_net=round(net, 1), GBps=round(3 * rows_bytes / (net * 1e-6) / 1e9, 1))
    res["pcen_over_meanvar"] = round(res["pcen_passes"]["us_net"] / res["meanvar_passes"]["us_net"], 3)
    return res


def online(torch, mfcc_amd, rounds, iters, n_lines=4096):
    g = torch.Generator(device="cuda").manual_seed(2)
    x = (torch.randn((n_lines, NFFT + HOP), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    first = x[:, :NFFT].contiguous().reshape(-1)
    flat = x[:, NFFT:].contiguous().reshape(-1)
    offs0 = np.arange(n_lines + 1, dtype=np.uint64) * np.uint64(NFFT)
    offs = np.arange(n_lines + 1, dtype=np.uint64) * np.uint64(HOP)
    res = {"lines": n_lines}
    with mfcc_amd.MFCC(**KW) as m, m.stream_bank(n_lines) as plain, m.stream_bank(n_lines, pcen=True) as pcen:
        out = torch.empty((n_lines, m.num_features), device="cuda")
        calls = {}
        for name, bank in (("plain_bank", plain), ("pcen_bank", pcen)):
            bank.push_packed(first, offs0)                # a frame each: every timed push then completes one
            calls[name] = lambda bank=bank: bank.push_packed(flat, offs, out=out)
        for f in calls.values():
            timed(torch, f, WARM)
        ms = {k: [] for k in calls}
        for _ in range(rounds):
            for k, f in calls.items():
                ms[k].append(timed(torch, f, iters))
        for k in calls:
            res[k] = dict(us=round(statistics.median(ms[k]) * 1e3, 1), us_min=round(min(ms[k]) * 1e3, 1),
                          us_max=round(max(ms[k]) * 1e3, 1))
        # the PCEN kernel of a tick reads and writes a row and the state (2 floats per band) per line
        res["pcen_tick_bytes"] = n_lines * m.num_features * 4 * (2 + 4)
        res["pcen_extra_us"] = round(res["pcen_bank"]["us"] - res["plain_bank"]["us"], 1)
    return res


def run(rounds, iters, passes_only):
    import torch
    import mfcc_amd
    line = {"metric": "pcen_rate", "device": torch.cuda.get_device_name(0), "rounds": rounds, "iters": iters}
    line["corpus"] = corpus(torch, mfcc_amd, rounds, iters, passes_only)
    torch.cuda.empty_cache()
    line["long_64x1h_w40"] = long_channels(torch, mfcc_amd, rounds, iters)
    torch.cuda.empty_cache()
    line["online_4096"] = online(torch, mfcc_amd, rounds, iters)
    print(json.dumps(line))


def summarize(trace):
    """Duration of every PCEN kernel of a kernel trace, per (kernel, grid size): the shapes differ in their grids."""
    durs = {}
    with open(trace) as f:
        for r in csv.DictReader(f):
            k = r["Kernel_Name"]
            if "pcen" not in k:
                continue
            name = k.split("(")[0].split("::")[-1]
            grid = r.get("Grid_Size_X") or r.get("Grid_Size") or "?"
            durs.setdefault("%s grid %s" % (name, grid), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print(json.dumps({k: dict(n=len(v), mean_us=round(statistics.mean(v) / 1e3, 2),
                              median_us=round(statistics.median(v) / 1e3, 2), min_us=round(min(v) / 1e3, 2))
                      for k, v in durs.items()}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes-only", action="store_true", help="leave out the frame kernels of the corpus (for a kernel trace)")
    ap.add_argument("--summarize", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        run(a.rounds, a.iters, a.passes_only)


if __name__ == "__main__":
    main()
