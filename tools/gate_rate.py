"""Cost of the power gate, of the window extraction and of a tracker tick (DESIGN.md sections 4.10 and 6c-quater) on
fixed-point rows of config 3's size: 64 channels x 9.6 M samples, 512/170/32, 13 coefficients, STREAM framing.

    python tools/gate_rate.py [--out profiles/gate_rate.txt]

The input is Gaussian noise whose amplitude switches between 30 and 3000 every 8000 samples (tools/vad_rate.py), so that
the gate at the reference's threshold passes part of the windows; the share is in the line.  Everything is timed with
device events after a warm-up, `iters` calls per timing, the median of `rounds` timings:
  gate     mfcc_hip_gate_dev (gate_power_kernel alone: equal-length channels need no table) at 93 / 1 and 93 / 31, all
           three outputs.  Beside it the bytes the algorithm needs, from the shapes: the rows once (2 R W) and the outputs
           once (10 per window), and what share of the 8 TB/s HBM peak that is at the measured time -- the kernel is
           HBM-bound by construction: it reads one column, but a 26-byte row shares its cache lines with that column
  windows  mfcc_hip_gate_windows_dev (vad_count_kernel, vad_scan_kernel, a synchronize, gate_gather_kernel) with a 10 %
           and a 100 % mask at both strides: wall time of the whole call and the bytes it writes per second
  tick     one push of 4096 lockstep lines with one hop of samples each: the plain fixed bank alone, then the bank with
           a tracker (93 / 1) chained behind it on the same stream, in turn"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream")
HBM_PEAK = 8e12


def timed(torch, fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def median_of(torch, fn, rounds, iters):
    timed(torch, fn, 3)
    v = [timed(torch, fn, iters) for _ in range(rounds)]
    return dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))


def noise(torch, shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = shape[-1]
    x = torch.randn(shape, device="cuda", generator=g)
    amp = torch.where(torch.rand(shape[:-1] + ((n + 7999) // 8000,), device="cuda", generator=g) < 0.5, 30.0, 3000.0)
    x *= amp.repeat_interleave(8000, -1)[..., :n]
    return x.clamp_(-32768, 32767).to(torch.int16)


def run(rounds, iters, out_path):
    import torch
    import mfcc_amd
    from mfcc_amd import wire
    line = {"metric": "gate_rate", "device": torch.cuda.get_device_name(0), "rounds": rounds, "iters": iters}
    with mfcc_amd.MFCC(**KW) as m:
        rows = m.process_fixed(noise(torch, (64, 9_600_000), 0))
        ch, T, W = rows.shape
        R = ch * T
        fo = np.arange(ch + 1, dtype=np.uint64) * np.uint64(T)
        line["rows"], line["width"] = int(R), int(W)
        for stride in (1, 31):
            wo = wire.gate_count(fo, 93, stride, offsets=True)
            n = int(wo[-1])
            power = torch.empty(n, device="cuda", dtype=torch.int64)
            gate = torch.empty(n, device="cuda", dtype=torch.uint8)
            ref = torch.empty(n, device="cuda", dtype=torch.uint8)

            def call():
                with m._on_torch_stream(rows.device):
                    rc = m._lib.mfcc_hip_gate_dev(m._h, C.c_void_p(rows.data_ptr()), W, fo.ctypes.data_as(C.c_void_p), ch, 93,
                                                  stride, wire.POWER_THRESHOLD, C.c_void_p(power.data_ptr()),
                                                  C.c_void_p(gate.data_ptr()), C.c_void_p(ref.data_ptr()))
                assert rc == 0, rc
            res = median_of(torch, call, rounds, iters)
            need = 2 * R * W + 10 * n
            res.update(windows=n, pass_share=round(float(gate.float().mean()), 4),
                       differ_share=round(float((gate != ref).float().mean()), 6), bytes_needed=need,
                       TBps=round(need / (res["ms"] * 1e-3) / 1e12, 3),
                       share_of_hbm_peak=round(need / (res["ms"] * 1e-3) / HBM_PEAK, 3))
            line["gate_93_%d" % stride] = res
            g = torch.Generator(device="cuda").manual_seed(5)
            for name, mask in (("mask10", (torch.rand(n, device="cuda", generator=g) < 0.1).to(torch.uint8)),
                               ("mask100", torch.ones(n, device="cuda", dtype=torch.uint8))):
                n_sel = int(mask.sum())
                out = torch.empty((n_sel, 93, W), device="cuda", dtype=torch.int16)

                def wall():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m.gate_windows(rows, mask, n_frames=93, stride=stride, out=out)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3
                for _ in range(3):
                    wall()
                v = [wall() for _ in range(rounds)]
                med = statistics.median(v)
                written = n_sel * (93 * W * 2 + 8)
                line["windows_93_%d_%s" % (stride, name)] = dict(
                    selected=n_sel, ms=round(med, 4), ms_min=round(min(v), 4), bytes_written=written,
                    written_TBps=round(written / (med * 1e-3) / 1e12, 3))
                del out
            del power, gate, ref
        del rows
        torch.cuda.empty_cache()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        n_lines, hop = 4096, 170
        x = noise(torch, (n_lines * 512,), 1)
        offs = np.arange(n_lines + 1, dtype=np.uint64)
        with m.stream_bank(n_lines, fixed=True) as bank, m.stream_bank(n_lines, fixed=True) as bank2, \
                m.power_gate(n_lines, n_frames=93, stride=1) as gate:
            bank.push_packed(x, offs * np.uint64(512))
            bank2.push_packed(x, offs * np.uint64(512))
            tick = x[:n_lines * hop]
            to = offs * np.uint64(hop)

            def plain():
                bank.push_packed(tick, to)

            def chained():
                r, f = bank2.push_packed(tick, to)
                gate.push(r, f)
            for _ in range(100):                                     # every line's window is full: one window per tick
                chained()
            a, b = [], []
            timed(torch, plain, 3)
            for _ in range(rounds):
                a.append(timed(torch, plain, iters))
                b.append(timed(torch, chained, iters))
            assert int(gate.num_windows(to)[-1]) == n_lines
            line["tick_4096"] = dict(bank_ms=round(statistics.median(a), 4), bank_ms_min=round(min(a), 4),
                                     bank_and_gate_ms=round(statistics.median(b), 4), bank_and_gate_ms_min=round(min(b), 4),
                                     ring_bytes=n_lines * 93 * 13 * 2)
    text = "# tools/gate_rate.py on one MI355X: python tools/gate_rate.py\n" + json.dumps(line) + "\n" + \
        json.dumps(line, indent=1) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "gate_rate.txt"))
    a = ap.parse_args()
    run(a.rounds, a.iters, a.out)


if __name__ == "__main__":
    main()
