"""Cost of a push of the filterbank stream bank against the one-shot filterbank call, and the wide delta kernel next to
the narrow one.

    python tools/fbank_bank_rate.py [--lines N] [--rounds R]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/fbank_bank_rate.py --part deltas

N lines (default 4096) in lockstep on the 512 / 160 / 400 handle with the HTK matrix of 80 bands in log2, device entry
(push_packed into a tensor of the caller's).

--part rate (the default): per chunk of one hop, 100 ms and 1 s of samples per line, in ONE process and timed in turn,
HIP events around T back-to-back calls, median of R rounds: a plain bank's push, the push of an online bank (meanvar over
600 rows, deltas of order 2, window 2; its window and ring are filled first, so every row pays the whole window), and
the one-shot ``filterbank`` call that computes the same frames -- (lines, L - hop + chunk) samples, what a bank in steady
state has of each line when the chunk arrives.

--part deltas: one-hop ticks of two banks with deltas 2 x 2 alone, 64 bands (online_deltas_kernel) and 128 bands
(online_deltas_wide_kernel); under the profiler the kernel statistics give the two kernels' times.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mfcc_amd  # noqa: E402

NFFT, HOP, FLEN = 512, 160, 400
KW = dict(nfft=NFFT, hop=HOP, win_length=FLEN, nfilters=8, nceptrums=8)
ONLINE = dict(normalize="meanvar", normalize_window=600, deltas=2, delta_window=2)
CHUNKS = {"hop": (HOP, 50), "100ms": (1600, 20), "1s": (16000, 5)}                # samples per line, calls per timing


def timed(call, ticks):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ticks):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ticks * 1e3


def summary(v):
    return dict(us=round(statistics.median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1))


def samples(rng, n):
    return torch.from_numpy(rng.integers(-3000, 3000, n).astype(np.int16)).cuda()


def rate(m, n, rounds, rng):
    first, off_first = samples(rng, n * FLEN), np.arange(n + 1, dtype=np.uint64) * FLEN
    res = {}
    with m.stream_bank(n, filterbank=True) as plain, m.stream_bank(n, filterbank=True, **ONLINE) as online:
        banks = {"plain": plain, "online": online}
        fill, off_fill = samples(rng, n * 16000), np.arange(n + 1, dtype=np.uint64) * 16000
        for b in banks.values():
            b.push_packed(first, off_first)
            for _ in range(8):                                                    # 800 rows: window and ring are full
                b.push_packed(fill, off_fill)
        torch.cuda.synchronize()
        assert (online.held == online.lag).all()
        del fill
        for name, (chunk, ticks) in CHUNKS.items():
            frames = chunk // HOP
            x, off = samples(rng, n * chunk), np.arange(n + 1, dtype=np.uint64) * chunk
            whole = samples(rng, n * (FLEN - HOP + chunk)).view(n, FLEN - HOP + chunk)
            outs = {k: torch.empty((n * frames, b.num_features), device="cuda") for k, b in banks.items()}
            one = torch.empty((n, frames, m.num_bands), device="cuda")
            calls = {k: (lambda b=b, o=outs[k]: b.push_packed(x, off, out=o)) for k, b in banks.items()}
            calls["one_shot"] = lambda: m.filterbank(whole, out=one)
            us = {k: [] for k in calls}
            for c in calls.values():                                              # scratch areas grow here, not in the timing
                c()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, c in calls.items():
                    us[k].append(timed(c, ticks))
            res[name] = dict({k: summary(v) for k, v in us.items()}, frames_per_line=frames, calls=ticks)
    return res


def deltas(mfcc, n, rounds, rng):
    res = {}
    first, off_first = samples(rng, n * FLEN), np.arange(n + 1, dtype=np.uint64) * FLEN
    x, off = samples(rng, n * HOP), np.arange(n + 1, dtype=np.uint64) * HOP
    for bands in (64, 128):
        with mfcc.MFCC(**KW) as m:
            m.set_filterbank(mfcc.htk_filterbank(bands, nfft=NFFT), "log2")
            with m.stream_bank(n, filterbank=True, deltas=2, delta_window=2) as bank:
                out = torch.empty((n, bank.num_features), device="cuda")
                bank.push_packed(first, off_first)
                for _ in range(8):
                    bank.push_packed(x, off, out=out if int(bank.num_frames([HOP] * n)[-1]) else None)
                torch.cuda.synchronize()
                us = [timed(lambda: bank.push_packed(x, off, out=out), 50) for _ in range(rounds)]
                res["deltas2x2_%d_bands" % bands] = summary(us)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", choices=["rate", "deltas"], default="rate")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"lines": a.lines, "part": a.part}
    if a.part == "rate":
        with mfcc_amd.MFCC(**KW) as m:
            m.set_filterbank(mfcc_amd.htk_filterbank(80, nfft=NFFT), "log2")
            res.update(kernel=m.filterbank_kernel_name(), **rate(m, a.lines, a.rounds, rng))
    else:
        res.update(deltas(mfcc_amd, a.lines, a.rounds, rng))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
