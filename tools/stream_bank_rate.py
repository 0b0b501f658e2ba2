"""Cost of one push of a stream bank (MFCC.stream_bank) on the headline handle (512/170/32, 13
cepstra), 16 kHz lines in lockstep, chunks of one hop, 100 ms and 1 s.

    python tools/stream_bank_rate.py > LINE
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o bank -- python tools/stream_bank_rate.py --device-only > LINE2
    python tools/stream_bank_rate.py --summarize OUT/.../bank_kernel_trace.csv LINE2

device: 4096 lines on the device entry (push_packed into a caller's tensor), device events around `iters` pushes, next to
the one-shot `process` over a (4096, pending + chunk) tensor -- the frame kernel alone over the same samples, the
floor -- alternating, the median of `rounds`.  The bank is first fed a frame so that every timed push completes frames.
host: 64 lines; a host clock around one tick = 64 MfccStream.push calls (each ends in a synchronise; the only online
path before the bank) and around one bank.push of the same 64 chunks, alternating.
--summarize: per chunk size the bank_advance_kernel dispatches of the trace in order (warm-up and timed pushes alike),
the bytes one of them moves from the shapes -- per line, read history + pending + chunk and write them as a row of W
(1 + pending + chunk samples each way), then read and write the carry (1 + pending' samples each way), 2 bytes a sample,
pending taken at its mean over the pushes -- and every kernel of the run that is not a frame kernel or bank_advance."""
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
NFFT, HOP = 512, 170
CHUNKS = {"hop": HOP, "100ms": 1600, "1s": 16000}
WARM = 3


def timed(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(v, digits=4):
    return dict(med=round(statistics.median(v), digits), min=round(min(v), digits), max=round(max(v), digits))


def device(torch, m, n_lines, rounds, iters):
    res = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, chunk in CHUNKS.items():
        x = (torch.randn((n_lines, NFFT + chunk), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
        offs = np.arange(n_lines + 1, dtype=np.uint64) * np.uint64(chunk)
        flat = x[:, :chunk].contiguous().reshape(-1)
        with m.stream_bank(n_lines) as bank:
            bank.push_packed(x[:, :NFFT].contiguous().reshape(-1), np.arange(n_lines + 1, dtype=np.uint64) * np.uint64(NFFT))
            pend0 = int(bank.pending[0])
            out = torch.empty((n_lines * (chunk // HOP + 1), m.num_features), device="cuda")
            pends, nfs = [pend0], []

            def push():                                   # the plan of a lockstep push, kept here: lengths only
                nf = (pends[-1] + chunk - NFFT) // HOP + 1
                nfs.append(nf)
                pends.append(pends[-1] + chunk - nf * HOP)
                bank.push_packed(flat, offs, out=out[:n_lines * nf])
            one = x[:, :pend0 + chunk].contiguous()
            one_out = m.process(one)

            def floor():
                m.process(one, out=one_out)
            timed(torch, push, WARM)
            timed(torch, floor, WARM)
            ms_p, ms_f = [], []
            for _ in range(rounds):
                ms_p.append(timed(torch, push, iters))
                ms_f.append(timed(torch, floor, iters))
            assert pends[-1] == int(bank.pending[0])
            res[name] = dict(chunk=chunk, lines=n_lines, pushes=len(nfs), pending_mean=round(float(np.mean(pends[:-1])), 1),
                             frames_per_line_mean=round(float(np.mean(nfs)), 2), floor_samples=pend0 + chunk,
                             floor_frames_per_line=int(one_out.shape[1]), push_ms=stats(ms_p), floor_ms=stats(ms_f),
                             push_over_floor=round(statistics.median(ms_p) / statistics.median(ms_f), 3))
    return res


def host(torch, m, n_lines, rounds):
    res = {}
    rng = np.random.default_rng(1)
    for name, chunk in CHUNKS.items():
        x = np.clip(np.rint(rng.standard_normal((n_lines, chunk)) * 3000), -32768, 32767).astype(np.int16)
        chunks = [np.ascontiguousarray(r) for r in x]
        sessions = [m.stream() for _ in range(n_lines)]
        with m.stream_bank(n_lines) as bank:
            def tick_sessions():
                t0 = time.perf_counter()
                for s, c in zip(sessions, chunks):
                    s.push(c)
                return (time.perf_counter() - t0) * 1e3

            def tick_bank():
                t0 = time.perf_counter()
                bank.push(chunks)
                return (time.perf_counter() - t0) * 1e3
            for _ in range(WARM + 1):
                tick_sessions()
                tick_bank()
            ts, tb = [], []
            for _ in range(rounds * 5):
                ts.append(tick_sessions())
                tb.append(tick_bank())
        for s in sessions:
            s.close()
        res[name] = dict(chunk=chunk, lines=n_lines, ticks=len(ts), sessions_ms=stats(ts), bank_ms=stats(tb),
                         sessions_over_bank=round(statistics.median(ts) / statistics.median(tb), 2))
    return res


def run(rounds, iters, device_only):
    import torch
    import mfcc_amd
    line = {"metric": "stream_bank_rate", "device": torch.cuda.get_device_name(0), "rounds": rounds, "iters": iters}
    with mfcc_amd.MFCC(**KW) as m:
        line["kernel"] = m.kernel_name()
        line["device_4096"] = device(torch, m, 4096, rounds, iters)
        if not device_only:
            line["host_64"] = host(torch, m, 64, rounds)
    print(json.dumps(line))


def summarize(trace, line_file):
    line = json.loads([s for s in open(line_file).read().splitlines() if s.startswith('{"metric": "stream_bank_rate"')][-1])
    adv, other = [], {}
    with open(trace) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            k = r["Kernel_Name"]
            if "bank_advance_kernel" in k:
                adv.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            elif line["kernel"] not in k:
                other[k[:100]] = other.get(k[:100], 0) + 1
    out, pos = {}, 0
    for name, c in line["device_4096"].items():
        part = adv[pos + 1:pos + 1 + c["pushes"]]          # the first dispatch of a bank is the frame that fills it
        pos += 1 + c["pushes"]
        med = statistics.median(part)
        pend = c["pending_mean"]                           # pending is stationary: the mean carry is as long
        nbytes = c["lines"] * 2 * 2 * ((1 + pend + c["chunk"]) + (1 + pend))
        out[name] = dict(dispatches=len(part), median_us=round(med / 1e3, 2), min_us=round(min(part) / 1e3, 2),
                         bytes=int(nbytes), TBps=round(nbytes / (med * 1e-9) / 1e12, 3))
    out["bank_advance_dispatches"] = len(adv)
    out["gather_rows_dispatches"] = sum(v for k, v in other.items() if "gather_rows_kernel" in k)
    out["other_kernels"] = other
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="the 4096-line device measurement alone (for a kernel trace)")
    ap.add_argument("--summarize", nargs=2, metavar=("KERNEL_TRACE_CSV", "LINE_FILE"))
    a = ap.parse_args()
    if a.summarize:
        summarize(*a.summarize)
    else:
        run(a.rounds, a.iters, a.device_only)


if __name__ == "__main__":
    main()
