"""The float path at frame hops other than nfft / 3 (``MFCC(hop=...)``, ``mfcc_hip_params.hop``: any value 1..nfft).

The fused kernels hard-code their hop (170 / 341) and the fixed path is the RTL's, at nfft / 3 only; every other hop
runs on the generic float kernel, and everything around the kernels -- frame counts, host chunks, ragged packing,
streaming sessions, halo shards -- computes its spans from the hop.

* H1  hop invariance, bit for bit: on the generic kernel a row depends only on its own samples, so the rows of a
      hop-h handle are the rows of a hop-1 handle at every h-th sample, in both framings;
* H2  routing and refusals: an explicit default hop is the default; a fused shape at any other hop runs the generic
      kernel; ``impl="fused512"`` and every fixed entry point refuse a foreign hop;
* H3  the float64 oracle's per-coefficient / per-value bound at the non-default-hop families of
      tests/kernel_families.py, cepstra and log-mel, a lifter and a halo shard;
* H4  normalization: within the bound of tests/normalize_ref.py of the raw rows; ragged batches = per utterance;
* H5  streaming sessions at hops 1, nfft - 1 and nfft: what every push consumes and returns."""
import ctypes as C

import numpy as np
import pytest

import kernel_families as kf
import logmel_bound as lb
import normalize_ref as nr
from kernel_families import as_np, open_handle, same
from oracle import error_bound as eb
from test_gpu_error_bound import KINDS as EB_KINDS
from test_gpu_error_bound import all_kinds

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]
GENERIC = "mfcc_float_generic_kernel"
HOP_FAMS = [f for f in kf.FLOAT if f.hop != f.nfft // 3]
HOP_IDS = [f.id for f in HOP_FAMS]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _err(mfcc_amd, fn):
    """The library's error code of ``fn()`` (which must raise ``MfccHipError``)."""
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        fn()
    return e.value.code


# ------------------------------------------------------------------------------------------------ H1

H1_SHAPES = {       # MFCC() arguments; hops: the grid of _grid(nfft)
    "g64": dict(nfft=64, nfilters=8, nceptrums=8, power_scale=0),
    "g256": dict(nfft=256, nfilters=20, nceptrums=13, power_scale=0),
    "g512": dict(nfft=512, nfilters=32, nceptrums=13),
    "g1024": dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0),
    "g512_48k": dict(nfft=512, nfilters=32, nceptrums=32, samplerate=48000),               # exact-DC branch
    "g256_logmel": dict(nfft=256, nfilters=20, nceptrums=13, power_scale=0, output="logmel"),
    "g1024_logmel": dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0, output="logmel"),
}


def _grid(nfft):
    t = nfft // 3
    return sorted({1, 2, 3, nfft // 4, t - 1, t, t + 1, nfft // 2, nfft - 1, nfft})


@pytest.mark.parametrize("shape", list(H1_SHAPES))
def test_h1_rows_at_any_hop_are_the_hop_1_rows_at_every_hop_th_sample(mfcc_amd, wav_pcm, shape):
    """R1 = the rows of a hop-1 NOTEBOOK handle on x followed by nfft zeros; a hop-h handle on x must give R1[f h] for
    every frame f, bit for bit, in both framings (STREAM's padded tail frame reads zeros past n as R1 does).  Lengths
    with n - nfft a multiple of h (at h = nfft the STREAM tail frame holds no sample of x) and one that is not."""
    kw = dict(H1_SHAPES[shape], impl="generic")
    nfft = kw["nfft"]
    rng = np.random.default_rng(nfft)
    with mfcc_amd.MFCC(hop=1, **kw) as m1:
        assert m1.kernel_name() == GENERIC
        for h in _grid(nfft):
            k = int(rng.integers(40, 90))
            for n in (nfft + h * k, nfft + h * k + h // 2 + 1):
                x = kf.channels(n, h + n, wav_pcm, kinds=("speech", "silences", "uniform"))
                x[2, n // 3: n // 3 + 2 * nfft] = 0                    # silent frames in every channel
                R1 = as_np(m1.process(_dev(np.concatenate([x, np.zeros((3, nfft), np.int16)], axis=1))))
                assert R1.shape[1] == n + 1
                for pad in PADS:
                    with mfcc_amd.MFCC(hop=h, pad_mode=pad, **kw) as m:
                        assert m.kernel_name() == GENERIC and m.hop == h
                        got = as_np(m.process(_dev(x)))
                        nf = m.num_frames(n)
                        assert got.shape[:2] == (3, nf), (shape, h, n, pad)
                        assert same(got, R1[:, np.arange(nf) * h]), (shape, h, n, pad)
                        assert same(m.process(x), got), (shape, h, n, pad, "host")


# ------------------------------------------------------------------------------------------------ H2

ROUTE_SHAPES = {
    "fused512": dict(nfft=512, nfilters=32, nceptrums=13),
    "fused512_16f": dict(nfft=512, nfilters=16, nceptrums=16),
    "fused1024": dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0),
    "generic256": dict(nfft=256, nfilters=20, nceptrums=13, power_scale=0),
}


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
@pytest.mark.parametrize("shape", list(ROUTE_SHAPES))
def test_h2_an_explicit_default_hop_is_the_default(mfcc_amd, wav_pcm, shape, output):
    kw = dict(ROUTE_SHAPES[shape], output=output)
    x = kf.channels(kw["nfft"] + 333 * 97, 5, wav_pcm)
    with mfcc_amd.MFCC(**kw) as a, mfcc_amd.MFCC(hop=kw["nfft"] // 3, **kw) as b:
        assert a.kernel_name() == b.kernel_name()
        assert (a.kernel_name() == GENERIC) == shape.startswith("generic"), a.kernel_name()
        assert a.hop == b.hop == kw["nfft"] // 3
        assert same(a.process(_dev(x)), b.process(_dev(x)))


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
@pytest.mark.parametrize("shape", ["fused512", "fused512_16f", "fused1024"])
def test_h2_a_fused_shape_at_another_hop_runs_the_generic_kernel(mfcc_amd, shape, output):
    kw = dict(ROUTE_SHAPES[shape], output=output)
    with mfcc_amd.MFCC(**kw) as m:
        assert m.kernel_name() != GENERIC                               # the control: the shape is fused
    for hop in (169, 171, 160, 340, 342, 256):
        for impl in ("auto", "generic"):
            with mfcc_amd.MFCC(hop=hop, impl=impl, **kw) as m:
                assert m.kernel_name() == GENERIC, (shape, output, hop, impl)


def test_h2_impl_fused512_refuses_another_hop(mfcc_amd):
    from mfcc_amd import _lib as L
    kw = ROUTE_SHAPES["fused512"]
    with mfcc_amd.MFCC(impl="fused512", **kw) as m:                    # the control
        assert m.kernel_name() != GENERIC
    for hop in (169, 171, 160):
        assert _err(mfcc_amd, lambda: mfcc_amd.MFCC(impl="fused512", hop=hop, **kw)) == L.ERROR_UNSUPPORTED, hop


def test_h2_every_fixed_entry_point_refuses_another_hop(mfcc_amd, wav_pcm, golden_dir, tmp_path):
    """The fixed path is the RTL's, at nfft / 3 only: at hop 171 every fixed entry point refuses, writes no file, and
    the float path of the same handle still runs (on the generic kernel)."""
    import os

    from mfcc_amd import _lib as L
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    x = wav_pcm[:512 + 171 * 40].copy()
    for pad in PADS:
        with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, hop=171, pad_mode=pad) as m:
            out = tmp_path / ("fixed_%s.mfcc" % pad)
            outs = [tmp_path / ("many_%s_%d.mfcc" % (pad, i)) for i in range(2)]
            calls = {
                "process_fixed host": lambda: m.process_fixed(x),
                "process_fixed device": lambda: m.process_fixed(_dev(x)),
                "process_fixed device halo": lambda: m.process_fixed(_dev(x), halo=1),
                "process_batch host": lambda: m.process_batch([x, x[:600]], fixed=True),
                "process_batch device": lambda: m.process_batch([_dev(x), _dev(x[:600])], fixed=True),
                "stream": lambda: m.stream(fixed=True),
                "convert": lambda: m.convert(wav, str(out), fixed=True),
                "convert_many": lambda: m.convert_many([wav, wav], [str(p) for p in outs], fixed=True),
            }
            for what, fn in calls.items():
                assert _err(mfcc_amd, fn) == L.ERROR_UNSUPPORTED, (pad, what)
            assert not out.exists() and not any(p.exists() for p in outs)
            assert m.kernel_name() == GENERIC
            got = m.process(x)
            assert got.shape == (m.num_frames(len(x)), 13) and np.isfinite(got).all()
            assert m.convert(wav, str(out), fixed=False) == m.num_frames(len(wav_pcm)) and out.exists()


# ------------------------------------------------------------------------------------------------ H3

def _eb_length(fam, nfr, pad):
    if pad == "notebook":
        return fam.hop * (nfr - 1) + fam.nfft
    return fam.hop * (nfr - 2) + fam.nfft + fam.hop // 2


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", HOP_FAMS, ids=HOP_IDS)
def test_h3_cepstra_and_logmel_meet_the_oracle(mfcc_amd, wav_pcm, fam, pad):
    """Every input kind of tests/test_gpu_error_bound.py, each coefficient against its own bound and each log-mel value
    against tests/logmel_bound.py; hop 1 at 2000 frames, the others at 101 (+ 16 x 32 for the longest)."""
    nfr = 2000 if fam.hop < 16 else 16 * 6 + 5
    n = _eb_length(fam, nfr, pad)
    pcm = all_kinds(n, 11 + fam.hop, wav_pcm)
    nb = fam.notebook_kw()
    with open_handle(mfcc_amd, fam, pad) as m, \
            mfcc_amd.MFCC(**fam.kwargs(pad, output="logmel")) as ml:
        assert ml.kernel_name() == GENERIC
        got = as_np(m.process(_dev(pcm)))
        lm = as_np(ml.process(_dev(pcm)))
    assert got.shape == (len(EB_KINDS), nfr, fam.nceptrums) and lm.shape == (len(EB_KINDS), nfr, fam.nfilters)
    worst = kf.check_oracle(fam, got, pcm, pad, what="%s kinds" % pad)
    worst_lm = 0.0
    for c in range(len(pcm)):
        worst_lm = max(worst_lm, lb.check(lm[c], pcm[c], GENERIC, "%s logmel %s channel %d" % (fam.id, pad, c),
                                          pad_mode=pad, **nb))
    print("H3 %s %s: worst error / bound %.3f (cepstra), %.3f (log-mel)" % (fam.id, pad, worst, worst_lm))


@pytest.mark.parametrize("pad", PADS)
def test_h3_lifter_and_a_halo_shard_on_an_odd_stride_view(mfcc_amd, wav_pcm, pad):
    """f512_h160 with lifter 22; a halo=1 shard of every kind at frame 7, on an odd channel stride from an odd base."""
    import torch
    fam = next(f for f in HOP_FAMS if f.id == "f512_h160")
    nfr = 16 * 6 + 5
    n = _eb_length(fam, nfr, pad)
    pcm = all_kinds(n, 21, wav_pcm)
    with mfcc_amd.MFCC(lifter=22.0, **fam.kwargs(pad)) as m:
        assert m.kernel_name() == GENERIC
        got = as_np(m.process(_dev(pcm)))
    worst = 0.0
    for c in range(len(pcm)):
        ref, bound = eb.reference_and_bound(pcm[c], eb.model_of(GENERIC), n_cep=fam.nceptrums, pad_mode=pad,
                                            lifter=22.0, **fam.notebook_kw())
        worst = max(worst, eb.check(got[c], ref, bound, "lifter 22 %s channel %d" % (pad, c)))
    print("H3 f512_h160 lifter 22 %s: worst error / bound %.3f" % (pad, worst))

    k = 7
    sub = pcm[:, fam.hop * k - 1:]
    nch, ns = sub.shape
    off, stride = 3, ns + 5
    stride += 1 - stride % 2
    flat = np.zeros(off + stride * nch + 8, np.int16)
    for c in range(nch):
        flat[off + c * stride: off + c * stride + ns] = sub[c]
    view = torch.as_strided(_dev(flat), (nch, ns), (stride, 1), storage_offset=off)
    with open_handle(mfcc_amd, fam, pad) as m:
        part = as_np(m.process(view, halo=1))
        whole = as_np(m.process(_dev(pcm)))
    assert same(part, whole[:, k:]), pad
    worst = kf.check_oracle(fam, part, sub, pad, halo=1, what="halo shard at frame %d" % k)
    print("H3 f512_h160 halo=1 %s: worst error / bound %.3f" % (pad, worst))


# ------------------------------------------------------------------------------------------------ H4

NORM_FAMS = [f for f in HOP_FAMS if f.id in ("f512_h160", "g512_h257", "g256_h256", "g128_h1")]


@pytest.mark.parametrize("mode", ["mean", "meanvar"])
@pytest.mark.parametrize("fam", NORM_FAMS, ids=[f.id for f in NORM_FAMS])
def test_h4_normalized_rows_within_the_bound_of_the_raw_rows(mfcc_amd, wav_pcm, fam, mode):
    nfr = 1500 if fam.hop < 16 else 300
    pcm = all_kinds(_eb_length(fam, nfr, "notebook"), 31, wav_pcm)
    with open_handle(mfcc_amd, fam) as raw, mfcc_amd.MFCC(normalize=mode, **fam.kwargs()) as m:
        assert m.kernel_name() == GENERIC
        x, y = raw.process(pcm), m.process(pcm)
        yd = as_np(m.process(_dev(pcm)))
    nch, nf, w = x.shape
    assert y.shape == x.shape and nf == nfr
    worst = nr.check(y.reshape(-1, w), x.reshape(-1, w), np.arange(nch + 1) * nf, mode, "%s %s" % (fam.id, mode))
    assert same(yd, y)
    print("H4 %s %s: worst error / bound %.3f" % (fam.id, mode, worst))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", [None, "meanvar"])
@pytest.mark.parametrize("fam", NORM_FAMS, ids=[f.id for f in NORM_FAMS])
def test_h4_ragged_batches_equal_per_utterance_calls(mfcc_amd, wav_pcm, fam, mode, pad):
    """A corpus with 0-, 1- and 2-frame utterances at the family's hop: host and device batches equal per-utterance
    calls."""
    hop, nfft = fam.hop, fam.nfft
    rng = np.random.default_rng(hop)
    lens = [0, 1, nfft - 1, nfft, nfft + 1, nfft + hop - 1, nfft + hop, nfft + hop + 1, nfft + 2 * hop - 1]
    lens += [nfft + hop * int(f) + int(e) for f, e in zip(rng.integers(0, 200, 24), rng.integers(0, hop, 24))]
    lens += [hop * 1500 + nfft + 5, 7, 3 * nfft]
    kinds = ("speech", "noise", "silences", "uniform")
    utts = [kf.signal(kinds[i % 4], v, 300 + i, wav_pcm) for i, v in enumerate(lens)]
    with mfcc_amd.MFCC(normalize=mode, **fam.kwargs(pad)) as m:
        assert m.kernel_name() == GENERIC
        one = [m.process(u) for u in utts]
        host = m.process_batch(utts)
        dev = m.process_batch([_dev(u) for u in utts])
        import torch
        torch.cuda.synchronize()
    counts = [len(o) for o in one]
    assert counts == [m.num_frames(v) for v in lens]
    assert {1, 2} <= set(counts) and (0 in counts) == (pad == "notebook")
    for i, o in enumerate(one):
        assert same(host[i], o), (fam.id, mode, pad, "host", i, lens[i])
        assert same(dev[i], o), (fam.id, mode, pad, "device", i, lens[i])


# ------------------------------------------------------------------------------------------------ H5

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("hop", [1, 255, 256])
def test_h5_stream_session_invariants(mfcc_amd, wav_pcm, hop, pad):
    """After every push: the frames it returns are (pending + n - nfft) // hop + 1 (or none), never more than
    ``stream_max_frames``; ``pending`` is what is left after them, below nfft.  The pushes + flush = one call."""
    nfft = 256
    pcm = kf.signal("silences", nfft + hop * (3000 // hop + 40) + 77, 91, wav_pcm)
    rng = np.random.default_rng(hop)
    with mfcc_amd.MFCC(nfft=nfft, nfilters=20, nceptrums=13, power_scale=0, hop=hop, pad_mode=pad) as m:
        assert m.kernel_name() == GENERIC
        R = as_np(m.process(_dev(pcm)))
        lib = m._lib
        for pattern in ("random", "small", "large"):
            with m.stream() as s:
                rows, pos = [], 0
                while pos < len(pcm):
                    if pattern == "random":
                        c = int(rng.integers(1, 3 * nfft))
                    elif pattern == "small":
                        c = int(rng.integers(1, 4))
                    else:
                        c = int(rng.integers(nfft, 4 * nfft))
                    chunk = pcm[pos:pos + c]
                    before = s.pending
                    cap = int(lib.mfcc_hip_stream_max_frames(s._s, C.c_size_t(len(chunk))))
                    r = s.push(chunk)
                    total = before + len(chunk)
                    want = (total - nfft) // hop + 1 if total >= nfft else 0
                    assert len(r) == want <= cap, (hop, pad, pattern, pos)
                    assert s.pending == total - want * hop < nfft, (hop, pad, pattern, pos)
                    rows.append(r)
                    pos += len(chunk)
                rows.append(s.flush())
                assert s.pending == 0
                assert same(np.concatenate(rows), R), (hop, pad, pattern)
