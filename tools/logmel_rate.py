"""Kernel rate of the log-mel output against the cepstra output, same process, same input, timed in turn.

    python tools/logmel_rate.py [--rounds R] [--iters I]

Configs 2 (64 x 9.6 M samples, 512/170/32) and 4 (64 x 57.6 M, 1024/341/40, power scale 1/nfft) of BASELINE.json.
For each config a cepstra handle (13 coefficients) and a log-mel handle are warmed up, then timed alternately R rounds
of I launches each (MFCC.time_launches: HIP events around back-to-back launches); the median round counts.  Prints
one JSON line: frames/s of each output, their ratio and the kernel names the handles report."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mfcc_amd  # noqa: E402

CONFIGS = {
    "config2": dict(samples=9_600_000, nfft=512, nfilters=32, power_scale=512.0),
    "config4": dict(samples=57_600_000, nfft=1024, nfilters=40, power_scale=0.0),
}


def measure(name, cfg, nch, rounds, iters):
    n = cfg["samples"]
    g = torch.Generator(device="cuda").manual_seed(0)
    pcm = (torch.randn((nch, n), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    kw = dict(nfft=cfg["nfft"], nfilters=cfg["nfilters"], nceptrums=13, power_scale=cfg["power_scale"])
    handles = {out: mfcc_amd.MFCC(output=out, **kw) for out in ("cepstra", "logmel")}
    nf = handles["cepstra"].num_frames(n)
    outs = {k: torch.empty((nch, nf, m.num_features), device="cuda") for k, m in handles.items()}
    for k, m in handles.items():                       # warm-up: clocks up, code and tables resident
        m.time_launches(pcm, outs[k], warmup=5, iters=10)
    ms = {k: [] for k in handles}
    for _ in range(rounds):
        for k, m in handles.items():
            ms[k].append(m.time_launches(pcm, outs[k], warmup=1, iters=iters))
    res = {"frames": nf * nch}
    for k, m in handles.items():
        med = statistics.median(ms[k])
        res[k] = dict(kernel=m.kernel_name(), ms=round(med, 4), gframes_per_s=round(nf * nch / med / 1e6, 3),
                      ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4))
    res["logmel_over_cepstra"] = round(res["cepstra"]["ms"] / res["logmel"]["ms"], 4)
    for m in handles.values():
        m.close()
    del pcm, outs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--channels", type=int, default=64)
    a = ap.parse_args()
    line = {"metric": "logmel_rate", "device": torch.cuda.get_device_name(0)}
    for name, cfg in CONFIGS.items():
        line[name] = measure(name, cfg, a.channels, a.rounds, a.iters)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
