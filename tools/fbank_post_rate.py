"""The filterbank post-passes against their yardsticks (diagnostic record for profiles/fbank_post_rate.txt, DESIGN.md
section 4.22): python tools/fbank_post_rate.py [--tag TEXT] [--wide-deltas-only] [--channels 64] [--samples 9600000]

64 channels x 9.6 M samples at 400 / 160 / 512, HTK 80 in log2 (and a 128-band matrix): ``filterbank`` alone and with
each setting of ``set_filterbank``; the same results from ``filterbank`` followed by the obvious torch ops on the same
tensors; a device-to-device copy of the bytes a pass moves; the narrow kernels at 64 bands through ``normalize_rows`` /
``deltas_rows``.  Every figure: HIP events around ONE call on torch's current stream, the median of 20 such calls with
[min, max], after 3 warm-up calls.  A pass's own time is the call with it minus ``filterbank`` alone (medians): the wide
kernels have no direct entry.  ``--wide-deltas-only --tag`` is for a library built with another MFCC_POST_WIDE_LDS_FLOATS
(MFCC_HIP_LIB names it): the delta tile's LDS size that was rejected, side by side with the chosen one."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mfcc_amd

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="")
ap.add_argument("--wide-deltas-only", action="store_true")
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--samples", type=int, default=9_600_000)
ap.add_argument("--out", default="profiles/fbank_post_rate.txt", help="the record: lines are appended")
args = ap.parse_args()
assert torch.cuda.is_available(), "this tool measures on the GPU: there is nothing to fall back to"
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
log = open(args.out, "a")


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def timed(fn, n=20, warm=3):
    """(median, min, max) ms of single calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def line(what, t, bytes_moved=None, base=None):
    s = "%-58s %8.3f ms [%7.3f, %7.3f]" % (what, *t)
    if base is not None:
        s += "   pass %7.3f ms" % (t[0] - base)
        if bytes_moved:
            s += "  %6.1f ps/B  %6.2f TB/s" % ((t[0] - base) * 1e9 / bytes_moved, bytes_moved / (t[0] - base) / 1e9)
    say(s)
    return t[0]


torch.manual_seed(0)
nch, n = args.channels, args.samples
pcm = (torch.randn((nch, n), device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
say("# %s%d channels x %d samples, 400 / 160 / 512, %s" % (args.tag + ": " if args.tag else "", nch, n,
                                                             torch.cuda.get_device_name(0)))


def deltas_torch(x, N):
    T = x.shape[1]
    xp = torch.cat([x[:, :1].expand(-1, N, -1), x, x[:, -1:].expand(-1, N, -1)], 1)
    d = sum(float(k) * (xp[:, N + k:N + k + T] - xp[:, N - k:N - k + T]) for k in range(1, N + 1))
    return d / (2.0 * sum(k * k for k in range(1, N + 1)))


def causal_meanvar_torch(x, N):
    """window [max(0, t - N), t + 1) by differences of cumulative sums"""
    T = x.shape[1]
    z = torch.zeros_like(x[:, :1])
    c1, c2 = torch.cat([z, x.cumsum(1)], 1), torch.cat([z, (x * x).cumsum(1)], 1)
    t = torch.arange(T, device=x.device)
    a = (t - N).clamp_(min=0)
    cnt = (t + 1 - a).to(x.dtype)[None, :, None]
    m = (c1[:, t + 1] - c1[:, a]) / cnt
    v = ((c2[:, t + 1] - c2[:, a]) / cnt - m * m).clamp_(min=1e-20)
    return (x - m) * v.rsqrt()


with mfcc_amd.MFCC(nfft=512, hop=160, win_length=400, nfilters=8, nceptrums=8) as m:
    nf = m.num_frames(n)
    for bands, W in ((80, mfcc_amd.htk_filterbank(80)), (128, mfcc_amd.htk_filterbank(128, fmin=20.0))):
        rows_b = nch * nf * bands * 4
        say("## %d bands: %d rows of %d floats, %.3f GB" % (bands, nch * nf, bands, rows_b / 1e9))
        m.set_filterbank(W)
        out1 = torch.empty((nch, nf, bands), device="cuda")
        base = line("filterbank alone (%s)" % m.filterbank_kernel_name(), timed(lambda: m.filterbank(pcm, out=out1)))
        cases = [("ΔΔ 2 x 8", dict(deltas=2, delta_window=8), 4)] if bands == 128 else \
            [("meanvar", dict(normalize="meanvar"), 3),
             ("causal meanvar 600", dict(normalize="meanvar", normalize_window=600, normalize_center=False), 2),
             ("ΔΔ 2 x 2", dict(deltas=2, delta_window=2), 4),
             ("PCEN", dict(pcen=True), 2),
             ("PCEN + causal meanvar 600 + ΔΔ 2 x 2", dict(pcen=True, normalize="meanvar", normalize_window=600,
                                                           normalize_center=False, deltas=2, delta_window=2), 8)]
        if args.wide_deltas_only:
            cases = [c for c in cases if "normalize" not in c[1] and "pcen" not in c[1]]
        for what, kw, passes in cases:                 # passes: how often the pass reads or writes W floats of every row
            m.set_filterbank(W, **kw)
            out = torch.empty((nch, nf, m.num_filterbank_columns), device="cuda")
            line("filterbank + " + what, timed(lambda: m.filterbank(pcm, out=out)), passes * rows_b, base)
            del out
        m.set_filterbank(W)
        if args.wide_deltas_only:
            continue
        x = m.filterbank(pcm, out=out1)
        if bands == 80:
            line("torch: filterbank + meanvar",
                 timed(lambda: (lambda r: (r - r.mean(1, keepdim=True)) / r.std(1, unbiased=False, keepdim=True))(m.filterbank(pcm, out=out1))),
                 None, base)
            line("torch: filterbank + causal meanvar 600 (cumsum)", timed(lambda: causal_meanvar_torch(m.filterbank(pcm, out=out1), 600)),
                 None, base)
            N = 2
        else:
            N = 8

        def dd():
            r = m.filterbank(pcm, out=out1)
            d = deltas_torch(r, N)
            return torch.cat([r, d, deltas_torch(d, N)], -1)
        line("torch: filterbank + ΔΔ 2 x %d (cat of shifted slices)" % N, timed(dd), None, base)
        say("(no torch figure for PCEN: its smoother is a recurrence over frames, a Python loop of %d steps)" % nf)
        other = torch.empty_like(x)
        line("device-to-device copy of the raw rows (%.2f GB read + written)" % (2 * rows_b / 1e9), timed(lambda: other.copy_(x)),
             2 * rows_b, 0.0)
        del other, x
        torch.cuda.empty_cache()
    if not args.wide_deltas_only:
        # the narrow kernels on rows of 64 floats, through the direct entries
        rows = torch.randn((nch, nf, 64), device="cuda")
        rb = rows.numel() * 4
        say("## 64 floats a row, the narrow kernels through the direct entries: %.3f GB" % (rb / 1e9))
        line("normalize_rows meanvar", timed(lambda: m.normalize_rows(rows, mode="meanvar")), 3 * rb, 0.0)
        for N in (2, 8):
            out = torch.empty((nch, nf, 192), device="cuda")
            line("deltas_rows 2 x %d" % N, timed(lambda: m.deltas_rows(rows, order=2, window=N, out=out)), 4 * rb, 0.0)
            del out
log.close()
