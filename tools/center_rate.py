"""Rate of the centring stage (mfcc_hip_center_dev) next to a device-to-device copy of the same
bytes, and what the extra pass costs a centred handle.

    python tools/center_rate.py [--log2n 28] [--runs 20] [--out profiles/center_rate.txt]

stage    2^log2n samples through mfcc_hip_center_dev (reflect, 512/170) for S16 and ULAW, HIP events around every single
         call on one stream, 3 warm-ups, the median of `runs`.  S16 moves 4 B per sample (2 read, 2 written), ULAW 3 B.
copy     the yardstick, same process, timed the same way: a device-to-device copy that reads and writes the same total,
         i.e. of half those bytes.
headline mfcc_hip_time_dev on 64 channels x 9 600 000 samples at 512/170/32/13, the same handle and tensors centred and
         uncentred; the centred rows are compared, bit for bit, with the uncentred handle's rows on a signal padded by
         torch indexing (not by the kernel under test).
spectrum power_spectrum at 512/160/400 on 64 channels x 960 000 samples, likewise, HIP events around single calls.
One JSON line on stdout; --out appends a readable table to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from decode_rate import WARM, each_ms, stats             # noqa: E402  (the same timing as the decode's record)

SIZE = {"s16": 2, "ulaw": 1}
TORCH_DTYPE = {"s16": "int16", "ulaw": "uint8"}


def rates(torch, mfcc_amd, n, runs):
    import ctypes as C
    from mfcc_amd import _lib as L
    lib = L.load()
    res = {}
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        n_out = mfcc_amd.api.center_geometry(n, "reflect", m._params, m.win_length)[2]
        for fmt in SIZE:
            g = torch.Generator(device="cuda").manual_seed(3)
            src = torch.randint(0, 256, (n * SIZE[fmt],), device="cuda", dtype=torch.uint8, generator=g).view(
                getattr(torch, TORCH_DTYPE[fmt]))
            out = torch.empty(n_out, device="cuda", dtype=torch.int16)
            moved = n * SIZE[fmt] + n_out * 2
            half = torch.empty(moved // 2, device="cuda", dtype=torch.uint8)
            other = torch.empty_like(half)
            code = getattr(L, "SAMPLE_" + fmt.upper())

            def center():
                with m._on_torch_stream(out.device):
                    L.check(lib.mfcc_hip_center_dev(m._h, L.CENTER_REFLECT, code, C.c_void_p(src.data_ptr()), n,
                                                    C.c_void_p(out.data_ptr()), n_out, None))
            r = dict(bytes_per_sample=SIZE[fmt] + 2, copy=stats(each_ms(torch, lambda: other.copy_(half), runs), moved),
                     center=stats(each_ms(torch, center, runs), moved))
            r["center_over_copy"] = round(r["center"]["ms"] / r["copy"]["ms"], 3)
            res[fmt] = r
            del src, out, half, other
            torch.cuda.empty_cache()
    return res


def reflect_pad(torch, x, nfft, hop, flen):
    """The padded signal of (channels, n) int16 by torch indexing."""
    n = x.shape[1]
    pl = nfft // 2 - (nfft - flen) // 2
    right = (n // hop) * hop + flen - pl - n
    parts = [x[:, 1:pl + 1].flip(1), x]
    if right > 0:
        parts.append(x[:, n - 1 - right:n - 1].flip(1))
    p = torch.cat(parts, dim=1)
    return p[:, :(n // hop) * hop + flen].contiguous()


def headline(torch, mfcc_amd, nch=64, n=9_600_000, warmup=3, iters=10, rounds=5):
    g = torch.Generator(device="cuda").manual_seed(4)
    pcm = torch.randint(-32768, 32768, (nch, n), device="cuda", dtype=torch.int16, generator=g)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        out = torch.empty((nch, 1 + n // m.hop, 13), device="cuda")
        plain = [m.time_launches(pcm, out, warmup=warmup, iters=iters) for _ in range(rounds)]
        m.set_center(True)
        centred = [m.time_launches(pcm, out, warmup=warmup, iters=iters) for _ in range(rounds)]
        got = m.process(pcm)
        m.set_center(None)
        same = bool(torch.equal(got, m.process(reflect_pad(torch, pcm, 512, m.hop, 512))))
    a, b = statistics.median(plain), statistics.median(centred)
    moved = nch * n * 4
    return dict(channels=nch, samples=n, plain_ms=round(a, 4), centred_ms=round(b, 4), extra_ms=round(b - a, 4),
                centred_over_plain=round(b / a, 3), center_bytes=moved,
                extra_GBps=round(moved / ((b - a) * 1e-3) / 1e9, 1) if b > a else None, same_bits=same)


def spectrum(torch, mfcc_amd, runs, nch=64, n=960_000):
    g = torch.Generator(device="cuda").manual_seed(5)
    pcm = torch.randint(-32768, 32768, (nch, n), device="cuda", dtype=torch.int16, generator=g)
    with mfcc_amd.MFCC(nfft=512, hop=160, win_length=400, nfilters=8, nceptrums=8) as m:
        out0 = torch.empty((nch, m.num_frames(n), m.num_bins), device="cuda")
        a = statistics.median(each_ms(torch, lambda: m.power_spectrum(pcm, out=out0), runs))
        m.set_center(True)
        out1 = torch.empty((nch, m.num_frames(n), m.num_bins), device="cuda")
        b = statistics.median(each_ms(torch, lambda: m.power_spectrum(pcm, out=out1), runs))
        m.set_center(None)
        same = bool(torch.equal(out1, m.power_spectrum(reflect_pad(torch, pcm, 512, 160, 400))))
    return dict(channels=nch, samples=n, plain_ms=round(a, 4), centred_ms=round(b, 4), extra_ms=round(b - a, 4),
                centred_over_plain=round(b / a, 3), same_bits=same)


def table(line):
    rows = ["center_rate: %s, 2^%d samples, median of %d single calls (HIP events), %d warm-ups"
            % (line["device"], line["log2n"], line["runs"], WARM),
            "%-6s %5s %12s %12s %12s %12s %8s" % ("format", "B/smp", "copy ms", "copy GB/s", "center ms", "center GB/s", "ctr/copy")]
    for fmt, r in line["formats"].items():
        rows.append("%-6s %5d %12.4f %12.1f %12.4f %12.1f %8.3f" % (fmt, r["bytes_per_sample"], r["copy"]["ms"], r["copy"]["GBps"],
                                                                  r["center"]["ms"], r["center"]["GBps"], r["center_over_copy"]))
    h = line["headline"]
    rows.append("headline %d x %d samples, 512/170/32/13, mfcc_hip_time_dev: uncentred %.4f ms, centred %.4f ms, extra %.4f ms "
                "(x %.3f; the stage moves %.0f MB: %s GB/s), same bits as the padded call: %s"
                % (h["channels"], h["samples"], h["plain_ms"], h["centred_ms"], h["extra_ms"], h["centred_over_plain"],
                   h["center_bytes"] / 1e6, h["extra_GBps"], h["same_bits"]))
    s = line["spectrum"]
    rows.append("power_spectrum %d x %d samples, 512/160/400: uncentred %.4f ms, centred %.4f ms, extra %.4f ms (x %.3f), "
                "same bits as the padded call: %s"
                % (s["channels"], s["samples"], s["plain_ms"], s["centred_ms"], s["extra_ms"], s["centred_over_plain"],
                   s["same_bits"]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", metavar="TXT", help="append the table to this file")
    a = ap.parse_args()
    import torch
    import mfcc_amd
    line = {"metric": "center_rate", "device": torch.cuda.get_device_name(0), "log2n": a.log2n, "runs": a.runs}
    line["formats"] = rates(torch, mfcc_amd, 1 << a.log2n, a.runs)
    torch.cuda.empty_cache()
    line["headline"] = headline(torch, mfcc_amd)
    torch.cuda.empty_cache()
    line["spectrum"] = spectrum(torch, mfcc_amd, a.runs)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write(table(line))


if __name__ == "__main__":
    main()
