"""Rate of the sample decode (mfcc_hip_decode_dev) next to a device-to-device copy of the same
bytes, and what the separate pass costs a ULAW handle on the headline shape.

    python tools/decode_rate.py [--log2n 28] [--runs 20] [--out profiles/decode_rate.txt]

decode   per format 2^log2n samples through mfcc_hip_decode_dev, HIP events around every single call on one stream,
         3 warm-ups, the median of `runs`.  A byte format moves 3 B per sample (1 read, 2 written), a 4-byte one 6 B.
copy     the yardstick, same process, timed the same way: a device-to-device copy that reads and writes the same total,
         i.e. of half those bytes.
headline mfcc_hip_time_dev of a ULAW handle over an S16 handle on 64 channels x 9 600 000 samples at 512/170/32/13: the
         decode pass in front of the frame kernel.
One JSON line on stdout; --out appends a readable table to a text file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM = 3
TORCH_DTYPE = {"ulaw": "uint8", "alaw": "uint8", "u8": "uint8", "i2s32": "int32", "s32": "int32", "f32": "float32"}
SIZE = {"ulaw": 1, "alaw": 1, "u8": 1, "i2s32": 4, "s32": 4, "f32": 4}


def each_ms(torch, fn, runs):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms, nbytes):
    med = statistics.median(ms)
    return dict(ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), GBps=round(nbytes / (med * 1e-3) / 1e9, 1))


def rates(torch, mfcc_amd, n, runs):
    import ctypes as C
    from mfcc_amd import _lib as L
    lib = L.load()
    res = {}
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        for fmt in SIZE:
            g = torch.Generator(device="cuda").manual_seed(3)
            raw = torch.randint(0, 256, (n * SIZE[fmt],), device="cuda", dtype=torch.uint8, generator=g)
            if fmt == "f32":
                src = (torch.rand(n, device="cuda", generator=g) * 2.2 - 1.1)
            else:
                src = raw.view(getattr(torch, TORCH_DTYPE[fmt]))
            out = torch.empty(n, device="cuda", dtype=torch.int16)
            moved = n * (SIZE[fmt] + 2)
            half = torch.empty(moved // 2, device="cuda", dtype=torch.uint8)
            other = torch.empty_like(half)
            code = getattr(L, "SAMPLE_" + fmt.upper())

            def decode():
                with m._on_torch_stream(out.device):
                    L.check(lib.mfcc_hip_decode_dev(m._h, code, C.c_void_p(src.data_ptr()), n, C.c_void_p(out.data_ptr())))
            r = dict(bytes_per_sample=SIZE[fmt] + 2, copy=stats(each_ms(torch, lambda: other.copy_(half), runs), moved),
                     decode=stats(each_ms(torch, decode, runs), moved))
            r["decode_over_copy"] = round(r["decode"]["ms"] / r["copy"]["ms"], 3)
            res[fmt] = r
            del raw, src, out, half, other
            torch.cuda.empty_cache()
    return res


def headline(torch, mfcc_amd, nch=64, n=9_600_000, warmup=3, iters=10, rounds=5):
    g = torch.Generator(device="cuda").manual_seed(4)
    kw = dict(nfft=512, nfilters=32, nceptrums=13)
    ulaw = torch.randint(0, 256, (nch, n), device="cuda", dtype=torch.uint8, generator=g)
    pcm = mfcc_amd.decode(ulaw, "ulaw")
    with mfcc_amd.MFCC(**kw) as m16, mfcc_amd.MFCC(sample_format="ulaw", **kw) as mu:
        out = torch.empty((nch, m16.num_frames(n), 13), device="cuda")
        t16 = [m16.time_launches(pcm, out, warmup=warmup, iters=iters) for _ in range(rounds)]
        ref = out.clone()
        tu = [mu.time_launches(ulaw, out, warmup=warmup, iters=iters) for _ in range(rounds)]
        same = bool(torch.equal(out, ref))
        a, b = statistics.median(t16), statistics.median(tu)
    return dict(channels=nch, samples=n, s16_ms=round(a, 4), ulaw_ms=round(b, 4), extra_ms=round(b - a, 4),
                ulaw_over_s16=round(b / a, 3), decode_bytes=nch * n * 3,
                extra_GBps=round(nch * n * 3 / ((b - a) * 1e-3) / 1e9, 1) if b > a else None, same_bits=same)


def table(line):
    rows = ["decode_rate: %s, 2^%d samples, median of %d single calls (HIP events), %d warm-ups"
            % (line["device"], line["log2n"], line["runs"], WARM),
            "%-6s %5s %12s %12s %12s %12s %8s" % ("format", "B/smp", "copy ms", "copy GB/s", "decode ms", "decode GB/s", "dec/copy")]
    for fmt, r in line["formats"].items():
        rows.append("%-6s %5d %12.4f %12.1f %12.4f %12.1f %8.3f" % (fmt, r["bytes_per_sample"], r["copy"]["ms"], r["copy"]["GBps"],
                                                                  r["decode"]["ms"], r["decode"]["GBps"], r["decode_over_copy"]))
    h = line["headline"]
    rows.append("headline %d x %d samples, 512/170/32/13, mfcc_hip_time_dev: s16 %.4f ms, ulaw %.4f ms, extra %.4f ms "
                "(x %.3f; the decode moves %.0f MB: %s GB/s), same bits: %s"
                % (h["channels"], h["samples"], h["s16_ms"], h["ulaw_ms"], h["extra_ms"], h["ulaw_over_s16"],
                   h["decode_bytes"] / 1e6, h["extra_GBps"], h["same_bits"]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--out", metavar="TXT", help="append the table to this file")
    a = ap.parse_args()
    import torch
    import mfcc_amd
    line = {"metric": "decode_rate", "device": torch.cuda.get_device_name(0), "log2n": a.log2n, "runs": a.runs}
    line["formats"] = rates(torch, mfcc_amd, 1 << a.log2n, a.runs)
    torch.cuda.empty_cache()
    line["headline"] = None if a.no_headline else headline(torch, mfcc_amd)
    print(json.dumps(line))
    if a.out and line["headline"]:
        with open(a.out, "a") as f:
            f.write(table(line))


if __name__ == "__main__":
    main()
