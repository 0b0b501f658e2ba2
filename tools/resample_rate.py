"""Rate of the sample-rate conversion (mfcc_hip_resample_dev) next to a device-to-device copy of
the same bytes, and what the separate pass costs a handle with an input rate on the headline shape.

    python tools/resample_rate.py [--log2n 27] [--runs 20] [--out profiles/resample_rate.txt]

resample per ratio 2^log2n input samples through mfcc_hip_resample_dev, HIP events around every single call on one
         stream, 3 warm-ups, the median of `runs` with min and max.  A call reads 2 n and writes 2 n_out bytes and does K
         multiply-adds per output.
copy     the yardstick, same process, timed the same way: a device-to-device copy that reads and writes the same total,
         i.e. of half those bytes.
headline mfcc_hip_time_dev of an S16 handle on 64 channels x 9 600 000 samples at 512/170/32/13, and of the same handle
         with input_rate = 8000 on 64 x 4 800 000: the resampling pass in front of the frame kernel.
One JSON line on stdout; --out appends a readable table to a text file."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM = 3
RATIOS = [(8000, 16000), (48000, 16000), (44100, 16000), (16000, 8000), (11025, 16000)]


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


def stats(ms):
    return dict(ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def rates(torch, mfcc_amd, n, runs):
    from mfcc_amd import _lib as L
    lib = L.load()
    res = {}
    g = torch.Generator(device="cuda").manual_seed(3)
    src = torch.randint(-32768, 32768, (n,), device="cuda", dtype=torch.int16, generator=g)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        for i, o in RATIOS:
            n_out = mfcc_amd.resample_count(n, i, o)
            K = mfcc_amd.resample_taps(i, o).shape[1]
            out = torch.empty(n_out, device="cuda", dtype=torch.int16)
            moved = 2 * (n + n_out)
            half = torch.empty(moved // 2, device="cuda", dtype=torch.uint8)
            other = torch.empty_like(half)

            def resample():
                with m._on_torch_stream(out.device):
                    L.check(lib.mfcc_hip_resample_dev(m._h, i, o, C.c_void_p(src.data_ptr()), n, C.c_void_p(out.data_ptr()), n_out))
            r = dict(K=K, n_out=n_out, bytes=moved, copy=stats(each_ms(torch, lambda: other.copy_(half), runs)),
                     resample=stats(each_ms(torch, resample, runs)))
            sec = r["resample"]["ms"] * 1e-3
            r["Gout_per_s"] = round(n_out / sec / 1e9, 2)
            r["GMAC_per_s"] = round(n_out * K / sec / 1e9, 1)
            r["GBps"] = round(moved / sec / 1e9, 1)
            r["copy_GBps"] = round(moved / (r["copy"]["ms"] * 1e-3) / 1e9, 1)
            r["resample_over_copy"] = round(r["resample"]["ms"] / r["copy"]["ms"], 3)
            res["%d_%d" % (i, o)] = r
            del out, half, other
            torch.cuda.empty_cache()
    return res


def headline(torch, mfcc_amd, nch=64, n=9_600_000, rate=8000, warmup=3, iters=10, rounds=5):
    g = torch.Generator(device="cuda").manual_seed(4)
    kw = dict(nfft=512, nfilters=32, nceptrums=13)
    n_in = n * rate // 16000
    low = (torch.randn((nch, n_in), device="cuda", generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    with mfcc_amd.MFCC(**kw) as m16, mfcc_amd.MFCC(input_rate=rate, **kw) as mr:
        pcm = torch.stack([mfcc_amd.resample(low[c], rate, 16000, mfcc=m16) for c in range(nch)])
        assert pcm.shape == (nch, n)
        out = torch.empty((nch, m16.num_frames(n), 13), device="cuda")
        t16 = [m16.time_launches(pcm, out, warmup=warmup, iters=iters) for _ in range(rounds)]
        ref = out.clone()
        tr = [mr.time_launches(low, out, warmup=warmup, iters=iters) for _ in range(rounds)]
        same = bool(torch.equal(out, ref))
        a, b = statistics.median(t16), statistics.median(tr)
    return dict(channels=nch, samples=n, input_rate=rate, input_samples=n_in, s16_ms=round(a, 4), s16_ms_range=[round(min(t16), 4), round(max(t16), 4)],
                rated_ms=round(b, 4), rated_ms_range=[round(min(tr), 4), round(max(tr), 4)], extra_ms=round(b - a, 4),
                rated_over_s16=round(b / a, 3), same_bits=same)


def table(line):
    rows = ["resample_rate: %s, 2^%d input samples, median [min, max] of %d single calls (HIP events), %d warm-ups"
            % (line["device"], line["log2n"], line["runs"], WARM),
            "%-12s %4s %22s %9s %9s %8s %22s %9s %8s" % ("ratio", "K", "resample ms", "Gout/s", "GMAC/s", "GB/s", "copy ms", "copy GB/s", "rs/copy")]
    for k, r in line["ratios"].items():
        a, c = r["resample"], r["copy"]
        rows.append("%-12s %4d %22s %9.2f %9.1f %8.1f %22s %9.1f %8.3f"
                    % (k, r["K"], "%.4f [%.4f, %.4f]" % (a["ms"], a["ms_min"], a["ms_max"]), r["Gout_per_s"], r["GMAC_per_s"],
                       r["GBps"], "%.4f [%.4f, %.4f]" % (c["ms"], c["ms_min"], c["ms_max"]), r["copy_GBps"], r["resample_over_copy"]))
    h = line["headline"]
    if h:
        rows.append("headline 512/170/32/13, mfcc_hip_time_dev: s16 %d x %d samples %.4f ms %s; input_rate %d on %d x %d samples "
                    "%.4f ms %s: extra %.4f ms (x %.3f), same bits: %s"
                    % (h["channels"], h["samples"], h["s16_ms"], h["s16_ms_range"], h["input_rate"], h["channels"],
                       h["input_samples"], h["rated_ms"], h["rated_ms_range"], h["extra_ms"], h["rated_over_s16"], h["same_bits"]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--note", default="", help="a line in front of the table")
    ap.add_argument("--out", metavar="TXT", help="append the table to this file")
    a = ap.parse_args()
    import torch
    import mfcc_amd
    line = {"metric": "resample_rate", "device": torch.cuda.get_device_name(0), "log2n": a.log2n, "runs": a.runs}
    line["ratios"] = rates(torch, mfcc_amd, 1 << a.log2n, a.runs)
    torch.cuda.empty_cache()
    line["headline"] = None if a.no_headline else headline(torch, mfcc_amd)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write((a.note + "\n" if a.note else "") + table(line))


if __name__ == "__main__":
    main()
