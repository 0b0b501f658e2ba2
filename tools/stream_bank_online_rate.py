"""Cost of a tick of the online stream bank against the plain bank's, and the per-kernel times of the online passes.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/stream_bank_online_rate.py [--lines N] [--ticks T]

N lines (default 4096) in lockstep on the headline handle (512/170/32, 13 cepstra), one hop of samples per line and
tick, device entry (push_packed).  In ONE process: a plain bank and an online bank (meanvar over N = 600, deltas of
order 2, window 2) are first run --fill ticks (default 800: the window and the ring of 750 rows are then full, so every
tick pays the whole window) and then timed in turn, HIP events around T back-to-back pushes, median of R rounds; under
the profiler those figures carry its overhead, the kernel statistics do not.  Ring traffic per tick is taken from the
shapes: every line re-reads at most N + S = 750 raw rows of W floats (lines x 750 x W x 4 bytes; a run in progress
re-reads N + the rows since its start, N + S / 2 on average).  Prints one JSON line."""
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
ONLINE = dict(normalize="meanvar", normalize_window=600, deltas=2, delta_window=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=int, default=800)
    a = ap.parse_args()
    hop, n = 170, a.lines
    rng = np.random.default_rng(1)
    first = torch.from_numpy(rng.integers(-3000, 3000, n * 512).astype(np.int16)).cuda()
    chunk = torch.from_numpy(rng.integers(-3000, 3000, n * hop).astype(np.int16)).cuda()
    off_first = np.arange(n + 1, dtype=np.uint64) * 512
    off = np.arange(n + 1, dtype=np.uint64) * hop
    res = {"lines": n, "ticks": a.ticks, "fill": a.fill}
    with mfcc_amd.MFCC(**KW) as m, m.stream_bank(n) as plain, m.stream_bank(n, **ONLINE) as online:
        banks = {"plain": plain, "online": online}
        outs = {k: torch.empty((n, b.num_features), device="cuda") for k, b in banks.items()}
        for k, b in banks.items():
            b.push_packed(first, off_first)                        # one frame per line; the online bank holds it back
            for _ in range(a.fill):
                b.push_packed(chunk, off, out=outs[k] if int(b.num_frames([hop] * n)[-1]) else None)
        torch.cuda.synchronize()
        assert (online.held == online.lag).all()

        def timed(k):
            b, out = banks[k], outs[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.ticks):
                b.push_packed(chunk, off, out=out)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.ticks * 1e3

        us = {k: [] for k in banks}
        for _ in range(a.rounds):
            for k in banks:
                us[k].append(timed(k))
        for k, v in us.items():
            res[k] = dict(us_per_tick=round(statistics.median(v), 1), us_min=round(min(v), 1), us_max=round(max(v), 1))
        W = 13
        res["ring_bytes_per_tick_max"] = n * 750 * W * 4
        res["ring_bytes_per_tick_mean"] = n * 675 * W * 4
    print(json.dumps(res))


if __name__ == "__main__":
    main()
