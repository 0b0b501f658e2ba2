"""Rate of the power-spectrum output (mfcc_hip_spectrum_i16_dev) next to its two roofs.

    python tools/spectrum_rate.py [--channels 64] [--samples 9600000] [--runs 20] [--out profiles/spectrum_rate.txt]

At the headline shape (64 channels x 9 600 000 samples, 512 / 170) and at 400 / 160 / 512 on the same samples:

fused    mfcc_spectrum512_kernel: HIP events around every single call on one stream, 3 warm-ups, the median of `runs`
         with min and max.  A call reads 2 bytes per sample and writes 4 (nfft / 2 + 1) bytes per frame.
generic  mfcc_spectrum_generic_kernel on the same input (impl="generic"), timed the same way; its rows are held to the
         fused kernel's within the reference's bound elsewhere (tests/test_gpu_spectrum.py), here only the time counts.
copy     the store roof, same process, timed the same way: a device-to-device copy of the output's bytes (it reads as
         many as it writes, so it is a roof with slack: the kernel reads a third of what it writes).
mfcc     the compute roof: mfcc_hip_time_dev of the handle's MFCC kernel (512 / 170 / 32 / 13; at 400 / 160 the fused
         hop-160 kernel) on the same input -- the same transforms with 13 floats per frame out instead of 257.
ragged   mfcc_hip_spectrum_ragged_i16_dev at 512 / 170 on 2000 utterances of 5 .. 15 s (packed, transformed, gathered: its
         rows cross HBM twice) next to the same samples in equal lengths (channels of one dense launch).
One JSON line on stdout; --out appends a readable table to a text file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM = 3
SHAPES = [("512/170", dict(nfft=512, hop=170)), ("400/160/512", dict(nfft=512, hop=160, win_length=400))]


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
    r = {}
    base = dict(nfilters=32, nceptrums=13, **kw)
    with mfcc_amd.MFCC(**base) as m, mfcc_amd.MFCC(impl="generic", **base) as g:
        nf = m.num_frames(n)
        out = torch.empty((nch, nf, m.num_bins), device="cuda", dtype=torch.float32)
        r.update(frames=nch * nf, out_bytes=out.numel() * 4, in_bytes=pcm.numel() * 2,
                 kernels=[m.spectrum_kernel_name(), g.spectrum_kernel_name(), m.kernel_name()])
        r["fused"] = stats(each_ms(torch, lambda: m.power_spectrum(pcm, out=out), runs))
        first = out[:, :64].clone()
        r["generic"] = stats(each_ms(torch, lambda: g.power_spectrum(pcm, out=out), runs))
        # the two kernels on the same frames: the largest difference relative to the frame's largest bin
        diff = (out[:, :64] - first).abs().amax(dim=2) / first.amax(dim=2).clamp_min(1e-30)
        r["max_rel_diff_first_64_frames"] = float(diff.max())
        other = torch.empty_like(out)
        r["copy"] = stats(each_ms(torch, lambda: other.copy_(out), runs))
        del other
        torch.cuda.empty_cache()
        feats = torch.empty((nch, nf, 13), device="cuda", dtype=torch.float32)
        t = [m.time_launches(pcm, feats, warmup=WARM, iters=10) for _ in range(5)]
        r["mfcc"] = dict(ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4))
    sec = r["fused"]["ms"] * 1e-3
    r["Gframes_per_s"] = round(r["frames"] / sec / 1e9, 3)
    r["store_GBps"] = round(r["out_bytes"] / sec / 1e9, 1)
    r["copy_store_GBps"] = round(r["out_bytes"] / (r["copy"]["ms"] * 1e-3) / 1e9, 1)
    r["fused_over_generic"] = round(r["fused"]["ms"] / r["generic"]["ms"], 3)
    r["fused_over_copy"] = round(r["fused"]["ms"] / r["copy"]["ms"], 3)
    r["fused_over_mfcc"] = round(r["fused"]["ms"] / r["mfcc"]["ms"], 3)
    return r


def ragged(torch, mfcc_amd, runs, n_utt=2000, mean=160_000):
    """The ragged entry at 512 / 170 on `n_utt` utterances of 5 .. 15 s (pack -> kernel -> gather, the rows written twice)
    next to the same samples cut into equal lengths, which run as channels of one dense launch."""
    import numpy as np
    lens = np.random.default_rng(6).integers(mean // 2, mean + mean // 2, n_utt)
    total = int(lens.sum())
    g = torch.Generator(device="cuda").manual_seed(5)
    flat = (torch.randn(total, device="cuda", generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    off_r = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    off_u = (np.arange(n_utt + 1) * (total // n_utt)).astype(np.uint64)      # the same samples (but a remainder) in equal lengths
    r = {}
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        for name, off in (("ragged", off_r), ("uniform", off_u)):
            rows = sum(m.num_frames(int(v)) for v in np.diff(off.astype(np.int64)))
            out = torch.empty((rows, m.num_bins), device="cuda", dtype=torch.float32)
            r[name] = dict(rows=rows, out_bytes=rows * m.num_bins * 4,
                           **stats(each_ms(torch, lambda: m.power_spectrum_packed(flat, off, out=out), runs)))
            del out
            torch.cuda.empty_cache()
    r.update(utterances=n_utt, samples=total, ragged_over_uniform=round(r["ragged"]["ms"] / r["uniform"]["ms"], 3))
    return r


def table(line):
    rows = ["spectrum_rate: %s, %d channels x %d samples, median [min, max] of %d single calls (HIP events), %d warm-ups; "
            "mfcc: mfcc_hip_time_dev, median [min, max] of 5 x 10 launches"
            % (line["device"], line["channels"], line["samples"], line["runs"], WARM),
            "%-12s %24s %24s %24s %24s %9s %10s %10s" % ("shape", "fused ms", "generic ms", "copy ms (store roof)",
                                                        "mfcc ms (compute roof)", "Gframe/s", "store GB/s", "copy GB/s")]

    def cell(s):
        return "%.4f [%.4f, %.4f]" % (s["ms"], s["ms_min"], s["ms_max"])
    for k, r in line["shapes"].items():
        rows.append("%-12s %24s %24s %24s %24s %9.3f %10.1f %10.1f"
                    % (k, cell(r["fused"]), cell(r["generic"]), cell(r["copy"]), cell(r["mfcc"]), r["Gframes_per_s"],
                       r["store_GBps"], r["copy_store_GBps"]))
        rows.append("%-12s fused / generic %.3f, fused / copy %.3f, fused / mfcc %.3f; %d frames, %.2f GB out, %.2f GB in; "
                    "kernels %s; fused vs generic on the first 64 frames of every channel: %.2e of the frame's largest bin"
                    % ("", r["fused_over_generic"], r["fused_over_copy"], r["fused_over_mfcc"], r["frames"], r["out_bytes"] / 1e9,
                       r["in_bytes"] / 1e9, ", ".join(r["kernels"]), r["max_rel_diff_first_64_frames"]))
    g = line.get("ragged")
    if g:
        a, u = g["ragged"], g["uniform"]
        rows.append("ragged 512/170, %d utterances, %d samples: lengths of 5 .. 15 s (pack, kernel, gather) %.4f [%.4f, %.4f] ms, "
                    "%d rows, %.2f GB out and as much scratch again; equal lengths (one dense launch) %.4f [%.4f, %.4f] ms, %d rows: "
                    "ragged / uniform %.3f"
                    % (g["utterances"], g["samples"], a["ms"], a["ms_min"], a["ms_max"], a["rows"], a["out_bytes"] / 1e9,
                       u["ms"], u["ms_min"], u["ms_max"], u["rows"], g["ragged_over_uniform"]))
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
    line = {"metric": "spectrum_rate", "device": torch.cuda.get_device_name(0), "channels": a.channels, "samples": a.samples,
            "runs": a.runs, "shapes": {}}
    for name, kw in SHAPES:
        line["shapes"][name] = shape(torch, mfcc_amd, pcm, kw, a.runs)
        torch.cuda.empty_cache()
    del pcm
    torch.cuda.empty_cache()
    line["ragged"] = ragged(torch, mfcc_amd, a.runs)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write((a.note + "\n" if a.note else "") + table(line))


if __name__ == "__main__":
    main()
