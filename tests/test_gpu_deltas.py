"""Delta coefficients (``MFCC(deltas=...)``, ``mfcc_hip_deltas_dev``) on the GPU: every element within the stage
bound of tests/deltas_ref.py of the handle's own static rows, the end-to-end result within the bound derived from
oracle/error_bound.py, bit-identity across the dense, ragged, host, device and chunked entry points and across runs,
crafted rows through the direct entry, and the refusals of the paths it does not cover."""
import ctypes as C
import os

import numpy as np
import pytest

import deltas_ref as dr
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu
KINDS = ["wav", "noise3000", "noise30", "uniform", "square", "sine", "dc_dither", "silences"]
WINDOWS = [1, 2, 3]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def signal(kind, n, seed, wav_pcm):
    """The input kinds of tests/test_gpu_error_bound.py."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "wav":
        return np.resize(wav_pcm[seed % 5000:], n).astype(np.int16)
    if kind == "noise3000":
        x = rng.standard_normal(n) * 3000
    elif kind == "noise30":
        x = rng.standard_normal(n) * 30
    elif kind == "uniform":
        x = rng.integers(-32768, 32768, n).astype(np.float64)
    elif kind == "square":
        x = 40000 * np.sign(np.sin(t * rng.uniform(0.01, 0.3)))
    elif kind == "sine":
        x = 20000 * np.sin(t * rng.uniform(0.01, 3.0))
    elif kind == "dc_dither":
        x = rng.integers(-20000, 20000) + rng.integers(-1, 2, n).astype(np.float64)
    else:                                             # silences
        x = rng.standard_normal(n) * 3000
        for a in rng.integers(0, max(n - 3000, 1), 2):
            x[a:a + int(rng.integers(300, 3000))] = 0
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def all_kinds(n, seed, wav_pcm):
    return np.stack([signal(k, n, seed + i, wav_pcm) for i, k in enumerate(KINDS)])


def per_channel(nch, nf):
    return np.arange(nch + 1, dtype=np.int64) * nf


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def np_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


# ------------------------------------------------------------------- 1. every float kernel family
FAMILIES = {
    "fused512": dict(nfft=512, nfilters=32, nceptrums=13),
    "fused1024": dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0.0),
    "generic512": dict(nfft=512, nfilters=32, nceptrums=13, impl="generic"),
    "generic256": dict(nfft=256, nfilters=32, nceptrums=13),
    "logmel512": dict(nfft=512, nfilters=32, nceptrums=13, output="logmel"),
    "logmel1024": dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0.0, output="logmel"),
    "fused512_44k": dict(nfft=512, nfilters=32, nceptrums=13, samplerate=44100),
    "fused512_48k": dict(nfft=512, nfilters=32, nceptrums=13, samplerate=48000),
}


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_kernel_family_within_the_stage_bound(mfcc_amd, wav_pcm, family, order, window):
    import torch
    kw = FAMILIES[family]
    nfft = kw["nfft"]
    pcm = all_kinds(nfft + (nfft // 3) * 700 + 37, 3, wav_pcm)
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(deltas=order, delta_window=window, **kw) as m:
        assert (m.deltas, m.delta_window) == (order, window) and m.kernel_name() == raw.kernel_name()
        if family.startswith("generic"):
            assert "generic" in m.kernel_name()
        x, y = raw.process(pcm), m.process(pcm)
        yd = m.process(torch.from_numpy(pcm).cuda())
        torch.cuda.synchronize()
    nch, nf, w = x.shape
    assert y.shape == (nch, nf, w * (1 + order)) and y.shape[-1] == m.num_features
    worst = dr.check_stage(y.reshape(-1, w * (1 + order)), x.reshape(-1, w), per_channel(nch, nf), order, window,
                           "%s K=%d N=%d" % (family, order, window))
    print("%s K=%d N=%d: worst %.3f of the stage bound" % (family, order, window, worst))
    assert same_bits(np_of(yd), y)


# ------------------------------------------------------------------- 2. end to end against the float64 oracle
@pytest.mark.parametrize("window", WINDOWS)
def test_end_to_end_against_the_oracle(mfcc_amd, wav_pcm, window):
    """The statics are within B of the oracle (oracle/error_bound.py); D and DD within B_D, B_DD of
    tests/deltas_ref.py.  For these inputs the oracle bounds every frame: a frame without a finite bound fails."""
    n = 512 + 170 * 1499
    inputs = {"golden wav": np.asarray(wav_pcm, dtype=np.int16), "tiled wav": np.resize(wav_pcm, n).astype(np.int16),
              "noise3000": signal("noise3000", n, 1, wav_pcm), "sine": signal("sine", n, 2, wav_pcm)}
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, deltas=2, delta_window=window) as m:
        model = eb.model_of(m.kernel_name())
        got = {k: m.process(v) for k, v in inputs.items()}
    for k, x in inputs.items():
        ref, B = eb.reference_and_bound(x, model, n_cep=13)
        assert got[k].shape == (len(ref), 39)
        worst = dr.check_end_to_end(got[k], ref, B, [0, len(ref)], 2, window, "%s N=%d" % (k, window))
        print("%s N=%d: worst %.3f of the end-to-end bound" % (k, window, worst))


# ------------------------------------------------------------------- 3. ragged: host and device = per utterance
def _corpus(wav_pcm, nfft, hop, seed=7):
    rng = np.random.default_rng(seed)
    lens = [0, nfft - 1, nfft, nfft + 5, nfft - 200, 37, nfft + hop]       # 0 / 1 / 2 frames, shorter than nfft
    lens += [int(v) for v in rng.integers(0, 30000, 180)]
    lens += [160000, 96013, 480000, 33333, 70001]                         # five long lengths
    utts = []
    for i, n in enumerate(lens):
        u = signal(KINDS[i % len(KINDS)], n, 100 + i, wav_pcm) if n else np.zeros(0, np.int16)
        if i % 9 == 4 and n > 2000:
            u[:1500] = 0                                                  # leading silence: -inf / NaN rows
        utts.append(u)
    return utts


@pytest.mark.parametrize("normalize", [None, "meanvar"])
@pytest.mark.parametrize("kw", [dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream"),
                                dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="notebook"),
                                dict(nfft=256, nfilters=32, nceptrums=13, pad_mode="stream")],
                         ids=["fused512_stream", "fused512_notebook", "generic256_stream"])
def test_ragged_host_and_device_equal_per_utterance(mfcc_amd, wav_pcm, kw, normalize):
    import torch
    utts = _corpus(wav_pcm, kw["nfft"], kw["nfft"] // 3)
    with mfcc_amd.MFCC(deltas=2, normalize=normalize, **kw) as m, mfcc_amd.MFCC(normalize=normalize, **kw) as st:
        one = [m.process(u) for u in utts]
        host = m.process_batch(utts)
        dev = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        torch.cuda.synchronize()
        static = [st.process(u) for u in utts]
    assert len(one) == len(host) == len(dev) == len(utts)
    assert sum(len(r) == 1 for r in one) >= 2
    if kw["pad_mode"] == "notebook":
        assert any(len(r) == 0 for r in one)
    assert any(not np.isfinite(r).all() for r in static)
    for i in range(len(utts)):
        assert one[i].shape == (len(static[i]), 39), i
        assert same_bits(host[i], one[i]), i
        assert same_bits(np_of(dev[i]), one[i]), i
        if len(one[i]):
            dr.check_stage(one[i], static[i], [0, len(one[i])], 2, 2, "utterance %d" % i)


# ------------------------------------------------------------------- 4. dense: host = device = per channel, chunking
def test_dense_host_device_and_per_channel_agree_under_chunking(mfcc_amd, wav_pcm, monkeypatch):
    import torch
    pcm = all_kinds(16000 * 30, 21, wav_pcm)[:6]                          # 6 x 960 KB: one channel per 1 MB chunk
    hour = signal("silences", 16000 * 3600, 5, wav_pcm)                   # frame-range chunks cut it
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, deltas=2) as m, \
            mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as raw:
        dev = m.process(torch.from_numpy(pcm).cuda())
        dev_h = m.process(torch.from_numpy(hour).cuda())
        torch.cuda.synchronize()
        dev, dev_h = np_of(dev), np_of(dev_h)
        whole = m.process(pcm)
        whole_h = m.process(hour)
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        chunked = m.process(pcm)
        chunked_h = m.process(hour)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        each = [m.process(c) for c in pcm]
        raw_h = raw.process(hour)
    assert same_bits(whole, dev) and same_bits(chunked, dev)
    for c in range(len(pcm)):
        assert same_bits(each[c], dev[c])
    nf = mfcc_amd.num_frames(len(hour))
    assert dev_h.shape == (nf, 39)
    assert same_bits(whole_h, dev_h) and same_bits(chunked_h, dev_h)
    assert not np.isfinite(raw_h).all()
    dr.check_stage(dev_h, raw_h, [0, nf], 2, 2, "one hour")


# ------------------------------------------------------------------- 5. full size, and a second run
@pytest.mark.parametrize("cfg", ["config2", "config4_channel"])
def test_full_size_within_the_stage_bound_and_repeatable(mfcc_amd, cfg):
    import torch
    if cfg == "config2":
        nch, n, kw = 64, 9_600_000, dict(nfft=512, nfilters=32, nceptrums=13)
    else:
        nch, n, kw = 1, 57_600_000, dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0.0, output="logmel")
    g = torch.Generator(device="cuda").manual_seed(3)
    pcm = (torch.randn((nch, n), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    pcm[:, 1_000_000:1_200_000] = 0                                        # silent frames: -inf / NaN rows
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(deltas=2, **kw) as m:
        x = raw.process(pcm)
        y1 = m.process(pcm)
        y2 = m.process(pcm)
        torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    nf, w = x.shape[1], x.shape[2]
    assert (nf, w) == ((56_468, 13) if cfg == "config2" else (168_912, 40))
    assert y1.shape == (nch, nf, 3 * w)
    del pcm, y2
    x, y = x.cpu().numpy(), y1.cpu().numpy()
    assert not np.isfinite(x).all()
    for c0 in range(0, nch, 8):                                            # 8 channels at a time: host memory
        c1 = min(nch, c0 + 8)
        dr.check_stage(y[c0:c1].reshape(-1, 3 * w), x[c0:c1].reshape(-1, w), per_channel(c1 - c0, nf), 2, 2, cfg)


# ------------------------------------------------------------------- 6. the direct entry on crafted rows
def _crafted_lengths():
    lens = list(range(71))
    for k in range(1, 13):
        lens += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    return lens + [20011]


@pytest.mark.parametrize("window", [1, 2, 8])
@pytest.mark.parametrize("width", [1, 13, 64])
def test_deltas_dev_on_crafted_rows(mfcc_amd, width, window):
    import torch
    rng = np.random.default_rng(width * 100 + window)
    lens = _crafted_lengths()
    rng.shuffle(lens)
    off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.uint64)      # the first segment starts at row 3
    R = int(off[-1]) + 4
    x = (rng.standard_normal((R, width)) * rng.uniform(0.5, 40, width) + rng.uniform(-50, 50, width)).astype(np.float32)
    if width >= 4:
        x[:, 1] = np.nan
        x[:, 2] = -np.inf
        x[:, 3] = (1e4 + 1e-2 * rng.standard_normal(R)).astype(np.float32)
    x[rng.choice(R, R // 50, replace=False), width - 1] = np.nan
    x[rng.choice(R, R // 70, replace=False), 0] = -np.inf
    sentinel = np.float32(-12345.5)
    a, b = int(off[0]), int(off[-1])
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        for order in (1, 2):
            wo = width * (1 + order)
            t = torch.from_numpy(x).cuda()
            out = torch.full((R, wo), float(sentinel), device="cuda")
            assert m.deltas_rows(t, off, order=order, window=window, out=out) is out
            # the same rows at another alignment: input and output shifted by one row
            big = torch.from_numpy(np.concatenate([np.zeros((1, width), np.float32), x])).cuda()
            obig = torch.full((R + 1, wo), float(sentinel), device="cuda")
            m.deltas_rows(big[1:], off, order=order, window=window, out=obig[1:])
            # no segments: a no-op
            out0 = torch.full((R, wo), float(sentinel), device="cuda")
            m.deltas_rows(t, np.array([5], np.uint64), order=order, window=window, out=out0)
            torch.cuda.synchronize()
            y, y_shift, y0 = out.cpu().numpy(), obig[1:].cpu().numpy(), out0.cpu().numpy()
            assert (y0 == sentinel).all()
            assert same_bits(y_shift, y)
            assert (y[:a] == sentinel).all() and (y[b:] == sentinel).all()     # rows outside the segments untouched
            worst = dr.check_stage(y[a:b], x[a:b], off.astype(np.int64) - a, order, window,
                                   "width %d K=%d N=%d" % (width, order, window))
            print("width %d K=%d N=%d: worst %.3f of the stage bound" % (width, order, window, worst))


def test_deltas_dev_arguments(mfcc_amd):
    import torch
    from mfcc_amd import _lib as L
    lib = mfcc_amd.load_library()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        t = torch.zeros((10, 13), device="cuda")
        o = torch.zeros((10, 39), device="cuda")
        p, q = C.c_void_p(t.data_ptr()), C.c_void_p(o.data_ptr())
        off = (C.c_size_t * 3)(0, 6, 4)
        assert lib.mfcc_hip_deltas_dev(m._h, p, 13, q, off, 2, 2, 2) == L.ERROR_INVALID_PARAM          # decreasing
        off = (C.c_size_t * 3)(0, 4, 8)
        for width, order, window in [(0, 2, 2), (65, 2, 2), (13, 0, 2), (13, 3, 2), (13, 2, 0), (13, 2, 9)]:
            assert lib.mfcc_hip_deltas_dev(m._h, p, width, q, off, 2, order, window) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_deltas_dev(m._h, None, 13, q, off, 2, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_deltas_dev(m._h, p, 13, None, off, 2, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_deltas_dev(m._h, C.c_void_p(t.data_ptr() + 2), 13, q, off, 2, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_deltas_dev(m._h, p, 13, C.c_void_p(o.data_ptr() + 2), off, 2, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_deltas_dev(m._h, C.c_void_p(o.data_ptr()), 13, q, off, 2, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_deltas_dev(m._h, C.c_void_p(o.data_ptr() + 4 * 13 * 10), 13, q, off, 2, 2, 2) == \
            L.ERROR_INVALID_PARAM                                                                   # overlapping
        assert lib.mfcc_hip_deltas_dev(m._h, None, 13, None, None, 0, 2, 2) == L.SUCCESS
        for order, window in [(3, 2), (-1, 2), (1, 0), (1, 9)]:
            assert lib.mfcc_hip_set_deltas(m._h, order, window) == L.ERROR_INVALID_PARAM
        with pytest.raises(ValueError):
            m.deltas_rows(t, order=3)
        with pytest.raises(ValueError):
            m.deltas_rows(t, order=2, out=torch.zeros((10, 26), device="cuda"))
        torch.cuda.synchronize()
        assert not o.any() and m.deltas == 0


# ------------------------------------------------------------------- 7. refusals and state
def test_refusals_busy_and_state(mfcc_amd, wav_pcm, golden_dir, tmp_path):
    import torch
    from mfcc_amd import _lib as L
    pcm = wav_pcm[:512 + 170 * 200].copy()
    dpcm = torch.from_numpy(pcm).cuda()
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream", deltas=2) as m:
        assert m.num_features == 39
        for call in [lambda: m.process_fixed(pcm), lambda: m.process_fixed(dpcm), lambda: m.stream(),
                     lambda: m.stream(fixed=True),
                     lambda: m.process_batch([pcm, pcm[:3000]], fixed=True),
                     lambda: m.process_batch([dpcm, dpcm[:3000]], fixed=True),
                     lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=False),
                     lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=True),
                     lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=False),
                     lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=True),
                     lambda: m.process(dpcm, halo=1)]:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == L.ERROR_UNSUPPORTED
        assert not os.path.exists(tmp_path / "a.mfcc") and not os.path.exists(tmp_path / "b.mfcc")
        # time_dev times what process_i16_dev enqueues, the delta pass included
        out = torch.empty((1, m.num_frames(len(pcm)), 39), device="cuda")
        assert m.time_launches(dpcm[None, :], out, warmup=1, iters=2) > 0
        torch.cuda.synchronize()
        want = m.process(pcm)
        assert same_bits(out[0].cpu().numpy(), want)
        # order 0 again: the bits of a handle that never had deltas
        m.set_deltas(0)
        assert m.deltas == 0 and m.num_features == 13
        back = m.process(pcm)
        with m.stream() as s:                                             # sessions are allowed again
            s.push(pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream") as fresh:
        assert same_bits(back, fresh.process(pcm))
        with fresh.stream() as s:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                fresh.set_deltas(2)
            assert e.value.code == L.ERROR_BUSY
            s.push(pcm)
        assert fresh.deltas == 0
        fresh.set_deltas(1, 3)
        assert (fresh.deltas, fresh.delta_window, fresh.num_features) == (1, 3, 26)
        dr.check_stage(fresh.process(pcm), back, [0, len(back)], 1, 3, "after BUSY")


def test_non_default_torch_stream_is_honoured(mfcc_amd, wav_pcm):
    import torch
    pcm = all_kinds(512 + 170 * 3000, 9, wav_pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, deltas=2) as m, \
            mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as raw:
        want = m.process(pcm)
        x = raw.process(pcm)
        s = torch.cuda.Stream()
        host = torch.from_numpy(pcm).pin_memory()
        rows_h = torch.from_numpy(x.reshape(-1, 13).copy()).pin_memory()
        with torch.cuda.stream(s):
            d = host.to("cuda", non_blocking=True)                        # produced on s, consumed on s
            y = m.process(d)
            rows = rows_h.to("cuda", non_blocking=True)
            z = m.deltas_rows(rows, per_channel(len(pcm), x.shape[1]), order=2, window=2)
        s.synchronize()
        assert same_bits(y.cpu().numpy(), want)
        assert same_bits(z.cpu().numpy(), want.reshape(-1, 39))
