"""Cost of the energy VAD decision and of the voiced-row selection (MFCC(vad="select")) on the
config-2 and config-5 static rows, against normalize_apply_kernel on the same rows, and the end-to-end cost of a selecting
handle over a plain one on config 5.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o vad -- python tools/vad_rate.py > LINE
    python tools/vad_rate.py --summarize OUT/.../vad_kernel_trace.csv LINE

config2: 64 x 9.6 M samples, 512/170/32, 13 cepstra.  config5: 10 000 utterances of five lengths (160 000 - 997 * (u % 5)
samples) on the ragged device path.  The input is Gaussian noise whose amplitude switches between 30 and 3000 every
8000 samples, so that the rule (threshold 0.5 + 1.0 * mean of C0, context 5, proportion 0.6) keeps about half of the
frames; the share it keeps is in the line.  Per config the raw rows are made once, then N = 3 + rounds * iters calls each
of vad_rows (vad_mean_kernel, vad_theta_kernel, vad_decide_kernel), select_rows (vad_count_kernel, vad_scan_kernel,
vad_gather_kernel) and the in-place normalize_rows (the yardstick's normalize_apply_kernel) run on them; only then, on
config 5, a selecting handle and a plain one are timed in turn (median of alternating calls).  --summarize therefore
takes dispatches [0, N) of every kernel as config 2, [N, 2N) as config 5 and the rest as the handle's.  Gather rate:
(4 W + 4 W v) bytes per row, v = the voiced share; apply rate: 8 W bytes per row."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(nfft=512, nfilters=32, nceptrums=13)
VAD = dict(energy_threshold=0.5, energy_mean_scale=1.0, frames_context=5, proportion_threshold=0.6)
KERNELS = ["vad_mean_kernel", "vad_theta_kernel", "vad_decide_kernel", "vad_count_kernel", "vad_scan_kernel",
           "vad_gather_kernel", "normalize_apply_kernel"]


def timed(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(torch, calls, rounds, iters):
    for f in calls.values():                          # warm-up: clocks up, code, tables and scratch resident
        timed(torch, f, 3)
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            ms[k].append(timed(torch, f, iters))
    return {k: dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))
            for k, v in ms.items()}


def noise(torch, shape, seed):
    """int16 Gaussian noise, amplitude 30 or 3000 per block of 8000 samples of the last axis."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = shape[-1]
    x = torch.randn(shape, device="cuda", generator=g)
    amp = torch.where(torch.rand(shape[:-1] + ((n + 7999) // 8000,), device="cuda", generator=g) < 0.5, 30.0, 3000.0)
    x *= amp.repeat_interleave(8000, -1)[..., :n]
    return x.clamp_(-32768, 32767).to(torch.int16)


def direct(torch, m, rows, fo, rounds, iters):
    """The passes on rows already in HBM; fo None: one segment per channel of (channels, frames, W)."""
    mask = m.vad_rows(rows, fo, **VAD)
    R, W = rows.numel() // rows.shape[-1], rows.shape[-1]
    out = torch.empty((R, W), device="cuda")
    work = rows.clone()
    res = {"rows": int(R), "width": int(W), "voiced_share": round(float(mask.float().mean()), 4)}
    res.update(measure(torch, {"vad_rows": lambda: m.vad_rows(rows, fo, out=mask, **VAD),
                               "select_rows": lambda: m.select_rows(rows, mask, fo, out=out),
                               "normalize_rows": lambda: m.normalize_rows(work, fo)}, rounds, iters))
    return res


def run(rounds, iters):
    import torch
    import mfcc_amd
    line = {"metric": "vad_rate", "device": torch.cuda.get_device_name(0), "direct_calls": 3 + rounds * iters, "vad": VAD}
    with mfcc_amd.MFCC(**KW) as m:
        pcm = noise(torch, (64, 9_600_000), 0)
        rows = m.process(pcm)
        del pcm
        line["config2"] = direct(torch, m, rows, None, rounds, iters)
        del rows
        torch.cuda.empty_cache()
        n_utt, n = 10_000, 160_000
        lens = [n - 997 * (u % 5) for u in range(n_utt)]
        offs = np.zeros(n_utt + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        flat = noise(torch, (int(offs[-1]),), 1)
        rows, fo = m.process_packed(flat, offs)
        line["config5"] = direct(torch, m, rows, fo, rounds, iters)
        out = torch.empty_like(rows)
        del rows
        with mfcc_amd.MFCC(vad="select", **{"vad_" + k: v for k, v in VAD.items()}, **KW) as sel:
            # the selecting call waits for its stream, so wall time and event time agree; alternate the two handles
            def wall(h):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h.process_packed(flat, offs, out=out)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for h in (m, sel, m, sel):
                wall(h)
            t_off, t_sel = [], []
            for _ in range(rounds * 3):
                t_off.append(wall(m))
                t_sel.append(wall(sel))
            kept = int(sel.process_packed(flat, offs, out=out)[1][-1])
        line["config5"]["handle"] = dict(
            calls=len(t_off), off_ms=round(statistics.median(t_off), 4), off_ms_min=round(min(t_off), 4),
            select_ms=round(statistics.median(t_sel), 4), select_ms_min=round(min(t_sel), 4), rows_kept=kept,
            overhead_pct=round(100 * (statistics.median(t_sel) / statistics.median(t_off) - 1), 2))
    print(json.dumps(line))


def summarize(trace, line_file):
    line = json.loads([s for s in open(line_file).read().splitlines() if s.startswith('{"metric": "vad_rate"')][-1])
    N = line["direct_calls"]
    ns = {k: [] for k in KERNELS}
    with open(trace) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    ns[k].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {}
    for i, cfg in enumerate(("config2", "config5")):
        R, W, v = line[cfg]["rows"], line[cfg]["width"], line[cfg]["voiced_share"]
        o = out.setdefault(cfg, {"rows": R, "voiced_share": v})
        for k in KERNELS:
            # vad_rows also ran once before the timed calls (the mask): its kernels have N + 1 dispatches per config
            extra = 1 if k in KERNELS[:3] else 0
            part = ns[k][i * (N + extra):(i + 1) * (N + extra)]
            med = statistics.median(part)
            o[k] = dict(dispatches=len(part), median_us=round(med / 1e3, 2), min_us=round(min(part) / 1e3, 2))
            if k == "vad_gather_kernel":
                o[k]["TBps"] = round(R * (4 * W + 4 * W * v) / (med * 1e-9) / 1e12, 3)
            if k == "normalize_apply_kernel":
                o[k]["TBps"] = round(R * 8 * W / (med * 1e-9) / 1e12, 3)
        o["gather_over_apply_rate"] = round(o["vad_gather_kernel"]["TBps"] / o["normalize_apply_kernel"]["TBps"], 3)
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--summarize", nargs=2, metavar=("KERNEL_TRACE_CSV", "LINE_FILE"))
    a = ap.parse_args()
    if a.summarize:
        summarize(*a.summarize)
    else:
        run(a.rounds, a.iters)


if __name__ == "__main__":
    main()
