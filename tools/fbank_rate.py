"""Rate of the filterbank output (mfcc_hip_fbank_i16_dev) next to the route it replaces and its
two roofs.

    python tools/fbank_rate.py [--channels 64] [--samples 9600000] [--runs 20] [--out profiles/fbank_rate.txt]

At the headline shape (64 channels x 9 600 000 samples, 512 / 170) and at 400 / 160 / 512 on the same samples, in LOG2
scale, with the HTK banks of 80 and of 128 bands (the fused kernel's fp32 form: the packed weights fit its LDS) and with
two matrices that do not fit and run its MFMA form: a dense random 128 x 257 one, and 24 bands of 129 bins each (3096
packed weights, just over the 3072 of the LDS form):

fused    mfcc_fbank512_kernel: HIP events around every single call on one stream, 3 warm-ups, the median of `runs` with
         min and max.  A call reads 2 bytes per sample and writes 4 n_bands bytes per frame.
generic  mfcc_fbank_generic_kernel on the same input (impl="generic"), timed the same way.
route    what the output replaces, end to end on the same tensors and timed the same way: power_spectrum into a
         preallocated buffer, torch.matmul with W.T into a preallocated buffer, torch.log2 in place.
copy     the store roof: a device-to-device copy of the output's bytes.
mfcc     the compute roof: mfcc_hip_time_dev of the handle's MFCC kernel (32 filters, 13 coefficients) on the same input.
One JSON line on stdout; --out appends a readable table to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM = 3
SHAPES = [("512/170", dict(nfft=512, hop=170)), ("400/160/512", dict(nfft=512, hop=160, win_length=400))]


def matrices(mfcc_amd):
    import numpy as np
    dense = np.random.default_rng(3).uniform(0.05, 1.0, (128, 257)).astype(np.float32)
    tails = np.zeros((24, 257), np.float32)
    for j in range(24):
        tails[j, 5 * j:5 * j + 129] = np.exp(-np.arange(129) / 40.0)
    return [("htk80", mfcc_amd.htk_filterbank(80)), ("htk128", mfcc_amd.htk_filterbank(128)), ("dense128", dense),
            ("tails24", tails)]


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


def shape(torch, mfcc_amd, pcm, kw, runs):
    nch, n = pcm.shape
    r = {"bands": {}}
    base = dict(nfilters=32, nceptrums=13, **kw)
    with mfcc_amd.MFCC(**base) as m, mfcc_amd.MFCC(impl="generic", **base) as g:
        nf = m.num_frames(n)
        r.update(frames=nch * nf, in_bytes=pcm.numel() * 2)
        power = torch.empty((nch, nf, m.num_bins), device="cuda", dtype=torch.float32)
        for name, W in matrices(mfcc_amd):
            nb = len(W)
            m.set_filterbank(W, "log2")
            g.set_filterbank(W, "log2")
            Wt = torch.from_numpy(W).cuda().t().contiguous()
            out = torch.empty((nch, nf, nb), device="cuda", dtype=torch.float32)
            b = dict(out_bytes=out.numel() * 4, kernels=[m.filterbank_kernel_name(), g.filterbank_kernel_name(), m.kernel_name()])
            b["fused"] = stats(each_ms(torch, lambda: m.filterbank(pcm, out=out), runs))
            first = out[:, :64].clone()
            b["generic"] = stats(each_ms(torch, lambda: g.filterbank(pcm, out=out), runs))
            fin = torch.isfinite(first) & torch.isfinite(out[:, :64])
            b["max_log2_diff_first_64_frames"] = float((out[:, :64] - first)[fin].abs().max())

            def route():
                m.power_spectrum(pcm, out=power)
                torch.matmul(power, Wt, out=out)
                torch.log2(out, out=out)
            b["route"] = stats(each_ms(torch, route, runs))
            other = torch.empty_like(out)
            b["copy"] = stats(each_ms(torch, lambda: other.copy_(out), runs))
            del other, out
            torch.cuda.empty_cache()
            sec = b["fused"]["ms"] * 1e-3
            b["Gframes_per_s"] = round(r["frames"] / sec / 1e9, 3)
            b["store_GBps"] = round(b["out_bytes"] / sec / 1e9, 1)
            for k in ("generic", "route", "copy"):
                b["fused_over_" + k] = round(b["fused"]["ms"] / b[k]["ms"], 3)
            r["bands"][name] = b
        del power
        torch.cuda.empty_cache()
        feats = torch.empty((nch, nf, 13), device="cuda", dtype=torch.float32)
        t = [m.time_launches(pcm, feats, warmup=WARM, iters=10) for _ in range(5)]
        r["mfcc"] = dict(ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))
    return r


def table(line):
    rows = ["fbank_rate: %s, %d channels x %d samples, LOG2 scale, median [min, max] of %d single calls (HIP events), "
            "%d warm-ups; mfcc: mfcc_hip_time_dev, median [min, max] of 5 x 10 launches"
            % (line["device"], line["channels"], line["samples"], line["runs"], WARM),
            "%-12s %8s %24s %24s %24s %24s %9s %10s" % ("shape", "matrix", "fused ms", "generic ms", "spectrum+matmul+log2 ms",
                                                       "copy ms (store roof)", "Gframe/s", "store GB/s")]

    def cell(s):
        return "%.4f [%.4f, %.4f]" % (s["ms"], s["ms_min"], s["ms_max"])
    for k, r in line["shapes"].items():
        for nb, b in r["bands"].items():
            rows.append("%-12s %8s %24s %24s %24s %24s %9.3f %10.1f"
                        % (k, nb, cell(b["fused"]), cell(b["generic"]), cell(b["route"]), cell(b["copy"]), b["Gframes_per_s"],
                           b["store_GBps"]))
            rows.append("%-18s fused / generic %.3f, fused / route %.3f, fused / copy %.3f; %.2f GB out; kernels %s; fused vs "
                        "generic on the first 64 frames of every channel: at most %.2e in log2"
                        % ("", b["fused_over_generic"], b["fused_over_route"], b["fused_over_copy"], b["out_bytes"] / 1e9,
                           ", ".join(b["kernels"]), b["max_log2_diff_first_64_frames"]))
        rows.append("%-12s mfcc ms (compute roof) %s; %d frames, %.2f GB in" % (k, cell(r["mfcc"]), r["frames"], r["in_bytes"] / 1e9))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--samples", type=int, default=9_600_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--note", default="", help="a line in front of the table")
    ap.add_argument("--out", metavar="TXT", help="append the table to this file")
    a = ap.parse_args()
    import torch
    import mfcc_amd
    g = torch.Generator(device="cuda").manual_seed(4)
    pcm = (torch.randn((a.channels, a.samples), device="cuda", generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    line = {"metric": "fbank_rate", "device": torch.cuda.get_device_name(0), "channels": a.channels, "samples": a.samples,
            "runs": a.runs, "shapes": {}}
    for name, kw in SHAPES:
        line["shapes"][name] = shape(torch, mfcc_amd, pcm, kw, a.runs)
        torch.cuda.empty_cache()
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write((a.note + "\n" if a.note else "") + table(line))


if __name__ == "__main__":
    main()
