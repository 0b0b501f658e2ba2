"""Rate of the fused 512 / hop 160 kernel for HTK-style banks (MFCC(mel="htk")) against the
generic kernel on the same handle, on a config-2-sized input: 64 channels x 9.6 M samples at 400 / 160 / 512, the same
samples for every handle.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o melbank -- python tools/melbank_rate.py > LINE
    python tools/melbank_rate.py --summarize OUT/.../melbank_kernel_trace.csv LINE
    python tools/melbank_rate.py                      # the same calls with the profiler off: event times only

Nine handles run in turn, `rounds` times, `iters` launches each (mfcc_hip_time_dev: HIP events around the launches on
one stream): HTK 40 (20 - 8000 Hz) and HTK 64 (125 - 7500 Hz), each as cepstra (13) and as log-mel rows, each on
mfcc_fused512_h160_mb_kernel and with impl="generic"; and the 32-filter notebook handle on mfcc_fused512_h160_kernel.

The yardstick of a fused handle is the generic kernel on the same handle (`<name>_generic`); its device code is the
parent commit's (the assembly comparison of DESIGN.md section 4.12).  --summarize takes the kernels' own durations from
the trace: the library launches one kernel per timed call, so the dispatches of its kernels, in start order, are the
calls in the order the line records them (`order`: runs of [handle, timed, launches])."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ASR = dict(nfft=512, hop=160, win_length=400, nceptrums=13)
HTK40 = dict(ASR, nfilters=40, mel="htk", fmin=20, fmax=8000)
HTK64 = dict(ASR, nfilters=64, mel="htk", fmin=125, fmax=7500)
HANDLES = {"notebook32": dict(ASR, nfilters=32)}
for _name, _kw in (("htk40", HTK40), ("htk64", HTK64)):
    for _out in ("cepstra", "logmel"):
        HANDLES["%s_%s" % (_name, _out)] = dict(_kw, output=_out)
        HANDLES["%s_%s_generic" % (_name, _out)] = dict(_kw, output=_out, impl="generic")
FUSED = [k for k in HANDLES if k.startswith("htk") and not k.endswith("_generic")]
WARMUP = 3


def _verdict(out, per_frame_min, per_frame_max):
    for k in FUSED:
        out[k + "_over_generic"] = round(out[k]["gframes_per_s"] / out[k + "_generic"]["gframes_per_s"], 2)
        # faster by more than the spread of the alternating runs: the slowest fused run against the fastest generic run
        out[k + "_faster_beyond_spread"] = bool(per_frame_max[k] < per_frame_min[k + "_generic"])
        out[k + "_of_notebook32"] = round(out[k]["gframes_per_s"] / out["notebook32"]["gframes_per_s"], 3)


def run(rounds, iters, channels, samples):
    import torch
    import mfcc_amd
    g = torch.Generator(device="cuda").manual_seed(0)
    pcm = (torch.randn((channels, samples), device="cuda", generator=g) * 3000.0).clamp_(-32768, 32767).to(torch.int16)
    hs = {k: mfcc_amd.MFCC(**kw) for k, kw in HANDLES.items()}
    try:
        frames = {k: h.num_frames(samples) * channels for k, h in hs.items()}
        outs = {w: torch.empty((channels, frames["notebook32"] // channels, w), device="cuda") for w in (13, 40, 64)}
        line = {"metric": "melbank_rate", "device": torch.cuda.get_device_name(0), "channels": channels,
                "samples_per_channel": samples, "rounds": rounds, "iters": iters, "warmup": WARMUP,
                "kernel": {k: h.kernel_name() for k, h in hs.items()}, "frames": frames, "order": []}
        for k, h in hs.items():                           # warm-up: clocks up, code and tables resident
            h.time_launches(pcm, outs[h.num_features], warmup=0, iters=WARMUP)
            line["order"].append([k, 0, WARMUP])
        ms = {k: [] for k in hs}
        for _ in range(rounds):
            for k, h in hs.items():
                ms[k].append(h.time_launches(pcm, outs[h.num_features], warmup=0, iters=iters))
                line["order"].append([k, 1, iters])
        for k, v in ms.items():
            med = statistics.median(v)
            line[k] = dict(ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                           gframes_per_s=round(frames[k] / (med * 1e-3) / 1e9, 3))
        _verdict(line, {k: min(v) / frames[k] for k, v in ms.items()}, {k: max(v) / frames[k] for k, v in ms.items()})
    finally:
        for h in hs.values():
            h.close()
    print(json.dumps(line))


def summarize(trace, line_file):
    line = json.loads([s for s in open(line_file).read().splitlines() if s.startswith('{"metric": "melbank_rate"')][-1])
    frames, order = line["frames"], [(k, timed) for k, timed, n in line["order"] for _ in range(n)]
    with open(trace) as f:
        rows = sorted((r for r in csv.DictReader(f) if "mfcc_" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(order), (len(rows), len(order))
    part = {k: [] for k in HANDLES}
    for r, (k, timed) in zip(rows, order):
        assert line["kernel"][k] in r["Kernel_Name"], (k, r["Kernel_Name"])
        if timed:
            part[k].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {}
    for k, v in part.items():
        med = statistics.median(v)
        out[k] = dict(kernel=line["kernel"][k], dispatches=len(v), median_us=round(med / 1e3, 2),
                      min_us=round(min(v) / 1e3, 2), max_us=round(max(v) / 1e3, 2),
                      gframes_per_s=round(frames[k] / (med * 1e-9) / 1e9, 3))
    _verdict(out, {k: min(v) / frames[k] for k, v in part.items()}, {k: max(v) / frames[k] for k, v in part.items()})
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
