"""Rate of the fused 512 / hop 160 kernel of a framed handle (MFCC(win_length=400)) against the
generic kernel at the same nfft and hop, on a config-2-sized input: 64 channels x 9.6 M samples, the same samples.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o framed -- python tools/framed_rate.py > LINE
    python tools/framed_rate.py --summarize OUT/.../framed_kernel_trace.csv LINE
    python tools/framed_rate.py                      # the same calls with the profiler off: event times only

Three handles at nfft 512, hop 160, 32 filters, 13 cepstra run in turn, `rounds` times, `iters` launches each
(mfcc_hip_time_dev: HIP events around the launches on one stream):

    yardstick   MFCC(hop=160)                                   mfcc_float_generic_kernel, 512-sample frames
    generic400  MFCC(hop=160, win_length=400, impl="generic")   the same kernel with the 400-sample window table
    fused400    MFCC(hop=160, win_length=400)                   mfcc_fused512_h160_kernel

The yardstick is the kernel a plain handle at hop 160 runs; its code is the parent commit's (the per-function assembly
comparison of DESIGN.md section 4.11).  The frame counts differ by one frame per channel (59 997 of 512 samples against
59 998 of 400), so the figures are per frame.  --summarize takes the kernels' own durations from the trace: every
dispatch of the fused kernel belongs to fused400; the generic kernel's dispatches alternate in blocks of `iters` (after
the warm-up launches) between the yardstick and generic400, in the order the calls were made."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = dict(nfft=512, hop=160, nfilters=32, nceptrums=13)
HANDLES = {
    "yardstick": dict(BASE),
    "generic400": dict(BASE, win_length=400, impl="generic"),
    "fused400": dict(BASE, win_length=400),
}
WARMUP = 3


def run(rounds, iters, channels, samples):
    import torch
    import mfcc_amd
    g = torch.Generator(device="cuda").manual_seed(0)
    pcm = (torch.randn((channels, samples), device="cuda", generator=g) * 3000.0).clamp_(-32768, 32767).to(torch.int16)
    hs = {k: mfcc_amd.MFCC(**kw) for k, kw in HANDLES.items()}
    try:
        frames = {k: h.num_frames(samples) * channels for k, h in hs.items()}
        out = torch.empty((channels, max(frames.values()) // channels, 13), device="cuda")
        line = {"metric": "framed_rate", "device": torch.cuda.get_device_name(0), "channels": channels,
                "samples_per_channel": samples, "rounds": rounds, "iters": iters, "warmup": WARMUP,
                "kernel": {k: h.kernel_name() for k, h in hs.items()}, "frames": frames}
        for h in hs.values():                             # warm-up: clocks up, code and tables resident
            h.time_launches(pcm, out, warmup=0, iters=WARMUP)
        ms = {k: [] for k in hs}
        for _ in range(rounds):
            for k, h in hs.items():
                ms[k].append(h.time_launches(pcm, out, warmup=0, iters=iters))
        for k, v in ms.items():
            med = statistics.median(v)
            line[k] = dict(ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                           gframes_per_s=round(frames[k] / (med * 1e-3) / 1e9, 3))
        line["fused_over_yardstick"] = round(line["fused400"]["gframes_per_s"] / line["yardstick"]["gframes_per_s"], 2)
        # faster by more than the spread of the alternating runs: the slowest fused run against the fastest yardstick run
        line["faster_beyond_spread"] = bool(max(ms["fused400"]) / frames["fused400"] < min(ms["yardstick"]) / frames["yardstick"])
    finally:
        for h in hs.values():
            h.close()
    print(json.dumps(line))


def summarize(trace, line_file):
    line = json.loads([s for s in open(line_file).read().splitlines() if s.startswith('{"metric": "framed_rate"')][-1])
    iters, rounds, frames = line["iters"], line["rounds"], line["frames"]
    gen, fused = [], []
    with open(trace) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            if "mfcc_fused512_h160_kernel" in r["Kernel_Name"]:
                fused.append(ns)
            elif "mfcc_float_generic_kernel" in r["Kernel_Name"]:
                gen.append(ns)
    # call order: warm-up of yardstick, generic400, fused400; then per round yardstick, generic400, fused400
    assert len(gen) == 2 * (WARMUP + rounds * iters) and len(fused) == WARMUP + rounds * iters, (len(gen), len(fused))
    timed_gen = gen[2 * WARMUP:]
    part = {"yardstick": [], "generic400": [], "fused400": fused[WARMUP:]}
    for r in range(rounds):
        part["yardstick"] += timed_gen[(2 * r) * iters:(2 * r + 1) * iters]
        part["generic400"] += timed_gen[(2 * r + 1) * iters:(2 * r + 2) * iters]
    out = {}
    for k, v in part.items():
        med = statistics.median(v)
        out[k] = dict(kernel=line["kernel"][k], dispatches=len(v), median_us=round(med / 1e3, 2),
                      min_us=round(min(v) / 1e3, 2), max_us=round(max(v) / 1e3, 2),
                      gframes_per_s=round(frames[k] / (med * 1e-9) / 1e9, 3))
    out["fused_over_yardstick"] = round(out["fused400"]["gframes_per_s"] / out["yardstick"]["gframes_per_s"], 2)
    out["faster_beyond_spread"] = bool(max(part["fused400"]) / frames["fused400"] < min(part["yardstick"]) / frames["yardstick"])
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--samples", type=int, default=9_600_000)
    ap.add_argument("--summarize", nargs=2, metavar=("KERNEL_TRACE_CSV", "LINE_FILE"))
    a = ap.parse_args()
    if a.summarize:
        summarize(*a.summarize)
    else:
        run(a.rounds, a.iters, a.channels, a.samples)


if __name__ == "__main__":
    main()
