"""Randomized differential soak (a tool; tests/test_gpu_soak_slice.py runs a fixed slice of it under pytest):
`python tests/soak_gpu.py [seed] [seconds]`.

Random channel counts, lengths, channel strides and base offsets (all alignment residues), history halo,
framing mode, n_cep 1..32 and six signal kinds (Gaussian at three levels, full-scale uniform, Gaussian
with a stretch of silence, DC, full-scale square, pure sine).  Fixed contract: the fused fixed-point
kernel against oracle/mfcc_fixed.py, bit for bit, EVERY signal kind.  Float contract: the fused 512 (random sample
rates, 16-filter banks) and 1024 (its per-rate schedules) kernels AND the generic kernel, each against the float64
oracle on every channel, and against each other.

How the float comparison is made: every float result -- the drawn n_cep, and all n_mel coefficients on the same
kernel and on the generic kernel -- is held to the per-coefficient error bound of the kernel's declared arithmetic
(oracle/error_bound.py, check()): each coefficient of each frame within the bound carried from the float64 oracle's
stages, frames with a silent band (-inf log-mel) to the oracle's exact -inf / NaN pattern.  Nothing is set aside:
DC, square and sine channels count under the float contract like the noise-like ones, at every sample rate, and the
fused 1024 kernel is compared on every frame.  The only frames the bound leaves free are those where the model
itself cannot tell a band from 0 (a constant input's bands away from DC: float64 roundoff of an exact zero); the
summary counts them.  The drawn n_cep is also compared with the first n_cep columns of the
all-coefficient run (1e-6: the same log-mel values through more DCT rows).  The summary prints the worst ratio
|error| / bound per kernel and signal kind.
Every case has its own seed, printed with the failure: `python tests/soak_gpu.py --case SEED` replays it.
FUZZ_FIXED=1 restricts the run to the fixed contract."""
import os, sys, time, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # repo root
import torch, mfcc_amd
from oracle import error_bound as eb
from oracle import mfcc_fixed as mx
from oracle import mfcc_float as mf


def signal(rng, n, kind):
    if kind == 0: x = rng.standard_normal(n) * rng.choice([30, 3000, 12000])
    elif kind == 1: x = rng.integers(-32768, 32768, n).astype(np.float64)
    elif kind == 2:
        x = rng.standard_normal(n) * 3000
        a, b = sorted(rng.integers(0, n + 1, 2)); x[a:b] = 0                     # a stretch of silence
    elif kind == 3: x = np.full(n, rng.integers(-32768, 32768), dtype=np.float64)  # DC
    elif kind == 4: x = 32767 * np.sign(np.sin(np.arange(n) * rng.uniform(0.01, 3.0)))   # full-scale square
    else: x = 20000 * np.sin(np.arange(n) * rng.uniform(0.001, 3.1))
    return np.clip(x, -32768, 32767).astype(np.int16)


WORST = {}         # (kernel, signal kind) -> largest |error| / bound seen (see the docstring)
FREE = [0, 0]      # float frames the model leaves unconstrained (a band's bound reaches its energy) / frames checked
KIND_NAMES = ["gauss", "uniform", "silence", "dc", "square", "sine"]


def pattern_ok(a, b):
    fin = np.isfinite(b)
    if not np.array_equal(np.isfinite(a), fin): return False, "finite pattern"
    if not np.array_equal(a[~fin], b[~fin], equal_nan=True): return False, "inf pattern"
    return True, ""


def bound_check(name, kind, g, ref, bound):
    """check() of one channel; returns a failure string or None, and records the ratio in WORST."""
    try:
        r = eb.check(g, ref, bound, name)
    except AssertionError as e:
        return str(e)[:600]
    free = eb.unbounded_frames(bound)
    FREE[0] += int(free.sum()); FREE[1] += len(free)
    key = (name, KIND_NAMES[kind])
    WORST[key] = max(WORST.get(key, 0.0), r)
    return None


def one_case(seed):
    """Returns a list of failure strings (empty: the case passed)."""
    rng = np.random.default_rng(seed)
    fails = []
    if rng.random() < 0.08:                      # ragged batch vs per-utterance calls, bit for bit
        nfft_r = int(rng.choice([512, 1024])); pad = str(rng.choice(["notebook", "stream"]))
        utts = [signal(rng, int(rng.integers(0, 6000)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(1, 12)))]
        nfil_r = (16 if rng.random() < 0.3 else 32) if nfft_r == 512 else 40     # 512 / 16: both fused kernels' other form
        with mfcc_amd.MFCC(nfft=nfft_r, nfilters=nfil_r, nceptrums=int(rng.integers(1, 17)),
                           pad_mode=pad, power_scale=0) as m:
            fl = m.process_batch(utts)
            fx = m.process_batch(utts, fixed=True) if nfft_r == 512 else None
            for i, u in enumerate(utts):
                if not np.array_equal(fl[i], m.process(u), equal_nan=True): fails.append("RAGGED FLOAT %d %s utt %d len %d" % (nfft_r, pad, i, len(u)))
                if fx is not None and not np.array_equal(fx[i], m.process_fixed(u)): fails.append("RAGGED FIXED %s utt %d len %d" % (pad, i, len(u)))
        return fails
    big = rng.random() < 0.5
    cfg = "x512" if os.environ.get("FUZZ_FIXED") else rng.choice(["f512", "f1024", "x512"])
    nfft, hop = (1024, 341) if cfg == "f1024" else (512, 170)
    nch = int(rng.integers(1, 5)); halo = int(rng.integers(0, 2)); pad = str(rng.choice(["notebook", "stream"]))
    n = int(rng.integers(0, 40000 if big else 3 * nfft))
    ncep = int(rng.integers(1, 33))
    stride = n + halo + int(rng.integers(0, 9)); off = int(rng.integers(0, 8))
    flat = np.zeros(off + stride * nch + 16, dtype=np.int16)
    kinds = [int(rng.integers(0, 6)) for _ in range(nch)]
    for c in range(nch): flat[off + c * stride: off + c * stride + n + halo] = signal(rng, n + halo, kinds[c])
    dev = torch.from_numpy(flat).cuda()
    view = torch.as_strided(dev, (nch, n + halo), (stride, 1), storage_offset=off)
    tag = "%s nch %d n %d halo %d %s ncep %d stride %d off %d kinds %s" % (cfg, nch, n, halo, pad, ncep, stride, off, kinds)
    if cfg == "x512":
        nfil = 16 if rng.random() < 0.3 else 32               # 16: the constructor default, the kernel's other instantiation
        ncep = min(ncep, nfil)
        tag += " nfil %d" % nfil
        with mfcc_amd.MFCC(nfft=512, nfilters=nfil, nceptrums=ncep, pad_mode=pad) as m:
            got = m.process_fixed(view, halo=halo).cpu().numpy()
        for c in range(nch if n < 6000 else 1):
            x = flat[off + c * stride: off + c * stride + n + halo]
            if halo:            # the oracle has no halo argument: put the shard one hop into a longer stream
                ref = mx.mfcc_fixed_ref(np.concatenate([np.zeros(169, np.int16), x]), nfilters=nfil, nceptrums=ncep, pad_mode=pad)[1:]
                ok = np.array_equal(got[c][: len(ref)], ref[: len(got[c])])
            else:
                ok = np.array_equal(got[c], mx.mfcc_fixed_ref(x, nfilters=nfil, nceptrums=ncep, pad_mode=pad))
            if not ok:
                fails.append("FIXED %s ch %d" % (tag, c))
                break
        return fails
    nmel = (16 if rng.random() < 0.25 else 32) if cfg == "f512" else 40
    sr = int(rng.choice([16000, 16000, 8000, 22050, 44100, 48000] if cfg == "f512" else [16000, 16000, 8000, 11025, 22050, 32000, 44100, 48000]))
    ncep = min(ncep, nmel)
    kw = dict(nfft=nfft, nfilters=nmel, pad_mode=pad, samplerate=sr, power_scale=512.0 if cfg == "f512" else 0)
    tag += " nmel %d sr %d" % (nmel, sr)
    with mfcc_amd.MFCC(nceptrums=ncep, **kw) as a, mfcc_amd.MFCC(nceptrums=nmel, **kw) as af, \
            mfcc_amd.MFCC(impl="generic", nceptrums=nmel, **kw) as bf:
        ga = a.process(view, halo=halo).cpu().numpy()
        gaf = af.process(view, halo=halo).cpu().numpy(); gbf = bf.process(view, halo=halo).cpu().numpy()
        names = (af.kernel_name(), bf.kernel_name())
        name_a = a.kernel_name()
    if ga.shape[1] == 0:
        return fails                               # no frame: nothing to compare
    for c in range(nch):
        x = flat[off + c * stride: off + c * stride + n + halo]
        xs = np.concatenate([np.zeros(hop - 1, np.int16), x]) if halo else x
        if pad == "stream":                        # the oracle's framing for the stages, like mfcc_float_ref
            nf = mf.num_frames_stream(len(xs), nfft, hop)
            xs = np.concatenate([xs, np.zeros((nf - 1) * hop + nfft - len(xs), dtype=xs.dtype)])
        ref, st = mf.mfcc_notebook(xs, nfft=nfft, hop=hop, n_mel=nmel, sample_rate=sr,
                                   power_scale=512.0 if cfg == "f512" else float(nfft), return_stages=True)
        if halo:
            ref = ref[1:]
            st = {k: (v[1:] if k in ("power", "mel", "logmel") else v) for k, v in st.items()}
        if halo and len(ref) == gaf.shape[1] - 1 and n < nfft:
            continue      # a shard shorter than a frame: the oracle's stream, one hop longer, has no frame of its own here
        runs = [(names[0], gaf[c], nmel), (names[1], gbf[c], nmel), (name_a, ga[c], ncep)]
        for name, g, k in runs:
            if len(g) != len(ref):
                fails.append("FLOAT %s %s ch %d: %d frames, oracle %d" % (name, tag, c, len(g), len(ref)))
                continue
            why = bound_check(name, kinds[c], g, ref[:, :k], eb.bound_from_stages(st, eb.model_of(name), k))
            if why:
                fails.append("FLOAT %s n_cep %d vs float64 oracle %s ch %d: %s" % (name, k, tag, c, why))
        if name_a == names[0] and len(ga[c]) == len(ref):
            # the drawn n_cep against the first columns of the all-coefficient run: the same log-mel values, fewer DCT rows
            a64 = ga[c].astype(np.float64)
            f64 = gaf[c][:, :ncep].astype(np.float64)
            ok, why = pattern_ok(a64, f64)
            fin = np.isfinite(f64)
            if ok and fin.any() and np.abs(a64[fin] - f64[fin]).max() > 1e-6 * max(np.abs(f64[fin]).max(), 1.0):
                ok, why = False, "err %.3g of %.3g" % (np.abs(a64[fin] - f64[fin]).max(), np.abs(f64[fin]).max())
            if not ok:
                fails.append("FLOAT n_cep %d vs n_cep %d of %s %s ch %d: %s" % (ncep, nmel, names[0], tag, c, why))
    return fails


def summary():
    if not WORST:
        return "no float channel compared"
    return "worst |error| / bound per float kernel and signal kind: " + ", ".join(
        "%s %s %.3f" % (k[0], k[1], v) for k, v in sorted(WORST.items())) + \
        "; frames left unconstrained (a band at the roundoff of an exact zero): %d of %d" % tuple(FREE)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        print(one_case(int(sys.argv[2])) or "case passes")
        sys.exit(0)
    seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    budget = float(sys.argv[2]) if len(sys.argv) > 2 else 120.0
    t0 = time.time(); cases = nfail = 0; t_said = t0
    while time.time() - t0 < budget:
        if time.time() - t_said > 60:                  # a line a minute: a silent GPU run is taken to be hung
            t_said = time.time(); print("...", cases, "cases,", nfail, "fails after %.0f s" % (t_said - t0), flush=True)
        seed = seed0 * 10_000_000 + cases
        cases += 1
        try:
            for f in one_case(seed):
                nfail += 1; print("MISMATCH [--case %d] %s" % (seed, f), flush=True)
        except Exception as e:
            nfail += 1; print("EXC [--case %d] %s" % (seed, repr(e)[:200]), flush=True)
    print("cases", cases, "fails", nfail, "in %.0f s;" % (time.time() - t0), summary())
