"""Per-segment normalization (``MFCC(normalize=...)``, ``mfcc_hip_normalize_dev``) on the GPU: every element within
the bound of tests/normalize_ref.py of the handle's own normalize-off rows, the end-to-end result within a bound
derived from oracle/error_bound.py, bit-identity across the dense, ragged, host, device and chunked entry points and
across runs, crafted rows through the direct entry, and the refusals of the paths it does not cover."""
import os

import numpy as np
import pytest

import normalize_ref as nr
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu
MODES = ["mean", "meanvar"]
KINDS = ["wav", "noise3000", "noise30", "uniform", "square", "sine", "dc_dither", "silences"]


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


# ------------------------------------------------------------------- 1. every float kernel family, both modes
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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_kernel_family_within_the_bound_of_its_raw_rows(mfcc_amd, wav_pcm, family, mode):
    import torch
    kw = FAMILIES[family]
    nfft = kw["nfft"]
    pcm = all_kinds(nfft + (nfft // 3) * 700 + 37, 3, wav_pcm)
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(normalize=mode, **kw) as m:
        assert m.normalize == mode and m.kernel_name() == raw.kernel_name()
        if family.startswith("generic"):
            assert "generic" in m.kernel_name()
        x, y = raw.process(pcm), m.process(pcm)
        xw, yw = raw.process(wav_pcm), m.process(wav_pcm)
        yd = m.process(torch.from_numpy(pcm).cuda())
        torch.cuda.synchronize()
    nch, nf, w = x.shape
    assert y.shape == x.shape and w == m.num_features
    nr.check(y.reshape(-1, w), x.reshape(-1, w), per_channel(nch, nf), mode, "%s %s" % (family, mode))
    nr.check(yw, xw, [0, len(xw)], mode, "%s %s golden wav" % (family, mode))
    assert same_bits(yd.cpu().numpy(), y)


# ------------------------------------------------------------------- 2. end to end against the float64 oracle
def test_end_to_end_against_the_normalized_oracle(mfcc_amd, wav_pcm):
    """x = kernel rows, r = oracle rows, |x - r| <= b elementwise (oracle/error_bound.py).  Per column j of a segment
    of N rows: |mu_x - mu_r| = |mean_i (x - r)| <= mean_i b_ij, and |sigma_x - sigma_r| <= rms_i(x - r) <= rms_i b_ij
    (sigma * sqrt(N) is the L2 norm of the centred column, and centring does not lengthen a vector).  So
        |(x - mu_x) / sigma_x - (r - mu_r) / sigma_r|
            <= (b_ij + mean_i b_ij) / sigma_j + |z_ij| rms_i(b_ij) / sigma_j      (to first order in b / sigma)
    plus the normalization's own rounding, 2^-22 (|mu| + |x - mu|) / sigma' (tests/normalize_ref.py).  A factor
    1.25 on the first part covers the second-order terms."""
    n = 512 + 170 * 1499
    pcm = np.stack([np.resize(wav_pcm, n).astype(np.int16), signal("noise3000", n, 1, wav_pcm),
                    signal("sine", n, 2, wav_pcm)])
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar") as m:
        got = m.process(pcm)
        model = eb.model_of(m.kernel_name())
    for c in range(len(pcm)):
        ref, b = eb.reference_and_bound(pcm[c], model, n_cep=13)
        assert np.isfinite(ref).all() and np.isfinite(b).all()
        z, mu, sd = nr.normalize(ref, [0, len(ref)], "meanvar")
        sig = sd[0]
        tol = ((b + b.mean(axis=0)) / sig + np.abs(z) * np.sqrt((b * b).mean(axis=0)) / sig) * 1.25 + \
            nr.bound(ref, mu, sd)
        err = np.abs(got[c].astype(np.float64) - z)
        assert (err <= tol).all(), "channel %d: worst %.3g of the bound" % (c, float((err / tol).max()))


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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", [dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream"),
                                dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="notebook"),
                                dict(nfft=256, nfilters=32, nceptrums=13, pad_mode="stream")],
                         ids=["fused512_stream", "fused512_notebook", "generic256_stream"])
def test_ragged_host_and_device_equal_per_utterance(mfcc_amd, wav_pcm, kw, mode):
    import torch
    utts = _corpus(wav_pcm, kw["nfft"], kw["nfft"] // 3)
    with mfcc_amd.MFCC(normalize=mode, **kw) as m, mfcc_amd.MFCC(**kw) as raw:
        one = [m.process(u) for u in utts]
        host = m.process_batch(utts)
        dev = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        torch.cuda.synchronize()
        raw_rows = [raw.process(u) for u in utts]
    assert len(one) == len(host) == len(dev) == len(utts)
    assert sum(len(r) == 1 for r in one) >= 2
    if kw["pad_mode"] == "notebook":
        assert any(len(r) == 0 for r in one)
    assert any(not np.isfinite(r).all() for r in raw_rows)
    for i in range(len(utts)):
        assert same_bits(host[i], one[i]), i
        assert same_bits(dev[i].cpu().numpy(), one[i]), i
        if len(one[i]):
            nr.check(one[i], raw_rows[i], [0, len(one[i])], mode, "utterance %d" % i)


# ------------------------------------------------------------------- 4. dense: host = device = per channel, chunking
def test_dense_host_device_and_per_channel_agree_under_chunking(mfcc_amd, wav_pcm, monkeypatch):
    import torch
    pcm = all_kinds(16000 * 30, 21, wav_pcm)[:6]                          # 6 x 960 KB: one channel per 1 MB chunk
    hour = signal("silences", 16000 * 3600, 5, wav_pcm)                   # frame-range chunks cut it
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar") as m:
        dev = m.process(torch.from_numpy(pcm).cuda())
        dev_h = m.process(torch.from_numpy(hour).cuda())
        torch.cuda.synchronize()
        dev, dev_h = dev.cpu().numpy(), dev_h.cpu().numpy()
        whole = m.process(pcm)
        whole_h = m.process(hour)
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        chunked = m.process(pcm)
        chunked_h = m.process(hour)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        each = [m.process(c) for c in pcm]
    assert same_bits(whole, dev) and same_bits(chunked, dev)
    for c in range(len(pcm)):
        assert same_bits(each[c], dev[c])
    assert dev_h.shape == (mfcc_amd.num_frames(len(hour)), 13)
    assert same_bits(whole_h, dev_h) and same_bits(chunked_h, dev_h)


# ------------------------------------------------------------------- 5. full size, and a second run
@pytest.mark.parametrize("cfg", ["config2", "config4_channel"])
def test_full_size_within_the_bound_and_repeatable(mfcc_amd, cfg):
    import torch
    if cfg == "config2":
        nch, n, kw = 64, 9_600_000, dict(nfft=512, nfilters=32, nceptrums=13)
    else:
        nch, n, kw = 1, 57_600_000, dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0.0, output="logmel")
    g = torch.Generator(device="cuda").manual_seed(3)
    pcm = (torch.randn((nch, n), device="cuda", generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16)
    pcm[:, 1_000_000:1_200_000] = 0                                        # silent frames: -inf / NaN rows
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(normalize="meanvar", **kw) as m:
        x = raw.process(pcm)
        y1 = m.process(pcm)
        y2 = m.process(pcm)
        torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    nf, w = x.shape[1], x.shape[2]
    assert (nf, w) == ((56_468, 13) if cfg == "config2" else (168_912, 40))
    del pcm
    x, y = x.cpu().numpy(), y1.cpu().numpy()
    assert not np.isfinite(x).all()
    for c0 in range(0, nch, 8):                                            # 8 channels at a time: host memory
        c1 = min(nch, c0 + 8)
        nr.check(y[c0:c1].reshape(-1, w), x[c0:c1].reshape(-1, w), per_channel(c1 - c0, nf), "meanvar", cfg)


# ------------------------------------------------------------------- 6. the direct entry on crafted rows
@pytest.mark.parametrize("width", [1, 13, 64])
@pytest.mark.parametrize("mode", MODES)
def test_normalize_dev_on_crafted_rows(mfcc_amd, width, mode):
    import torch
    rng = np.random.default_rng(width)
    tr = 8192 // width                                                     # rows per tile of the stats pass
    lens = [0, 1, 2, 3, tr - 1, tr, tr + 1, 0, 2 * tr + 5, 5, 20011]
    off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.uint64)      # the first segment starts at row 3
    R = int(off[-1]) + 4
    x = (rng.standard_normal((R, width)) * rng.uniform(0.5, 40, width) + rng.uniform(-50, 50, width)).astype(np.float32)
    cols = {"const": 0, "nan": 1, "ninf": 2, "offset": 3}
    if width >= 4:
        x[:, cols["const"]] = -3.5
        x[:, cols["nan"]] = np.nan
        x[:, cols["ninf"]] = -np.inf
        x[:, cols["offset"]] = (1e4 + 1e-2 * rng.standard_normal(R)).astype(np.float32)
    x[rng.choice(R, R // 50, replace=False), width - 1] = np.nan
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        t = torch.from_numpy(x).cuda()
        m.normalize_rows(t, off, mode=mode)
        # the same segments at another alignment (the rows shifted by one row, the pointer by `width` floats)
        big = torch.from_numpy(np.concatenate([np.zeros((1, width), np.float32), x])).cuda()
        m.normalize_rows(big[1:], off, mode=mode)
        # no segments, and mode NONE: no-ops
        t0 = torch.from_numpy(x).cuda()
        m.normalize_rows(t0, np.array([5], np.uint64), mode=mode)
        m.normalize_rows(t0, off, mode=None)
        torch.cuda.synchronize()
        y, y_shift, y0 = t.cpu().numpy(), big[1:].cpu().numpy(), t0.cpu().numpy()
    assert same_bits(y0, x)
    assert same_bits(y_shift, y)
    a, b = int(off[0]), int(off[-1])
    assert same_bits(y[:a], x[:a]) and same_bits(y[b:], x[b:])              # rows outside the segments untouched
    nr.check(y[a:b], x[a:b], off.astype(np.int64) - a, mode, "width %d" % width)
    if width >= 4:
        assert np.all(y[a:b, cols["const"]] == 0.0)
        assert np.isnan(y[:, cols["nan"]]).all() and np.isneginf(y[:, cols["ninf"]]).all()


def test_normalize_dev_arguments(mfcc_amd):
    import ctypes as C
    import torch
    from mfcc_amd import _lib as L
    lib = mfcc_amd.load_library()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        t = torch.zeros((10, 13), device="cuda")
        p = C.c_void_p(t.data_ptr())
        off = (C.c_size_t * 3)(0, 6, 4)
        assert lib.mfcc_hip_normalize_dev(m._h, p, 13, off, 2, 2) == L.ERROR_INVALID_PARAM       # decreasing
        off = (C.c_size_t * 3)(0, 4, 8)
        assert lib.mfcc_hip_normalize_dev(m._h, p, 0, off, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_normalize_dev(m._h, p, 65, off, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_normalize_dev(m._h, p, 13, off, 2, 3) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_normalize_dev(m._h, None, 13, off, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_normalize_dev(m._h, C.c_void_p(t.data_ptr() + 2), 13, off, 2, 2) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_normalize_dev(m._h, None, 13, None, 0, 2) == L.SUCCESS
        assert lib.mfcc_hip_set_normalize(m._h, 3) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_set_normalize(m._h, -1) == L.ERROR_INVALID_PARAM
        torch.cuda.synchronize()
        assert not t.any()


# ------------------------------------------------------------------- 7. refusals and state
def test_refusals_busy_and_state(mfcc_amd, wav_pcm, golden_dir, tmp_path):
    import torch
    from mfcc_amd import _lib as L
    pcm = wav_pcm[:512 + 170 * 200].copy()
    dpcm = torch.from_numpy(pcm).cuda()
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream", normalize="meanvar") as m:
        for call in [lambda: m.process_fixed(pcm), lambda: m.process_fixed(dpcm), lambda: m.stream(),
                     lambda: m.stream(fixed=True),
                     lambda: m.process_batch([pcm, pcm[:3000]], fixed=True),
                     lambda: m.process_batch([dpcm, dpcm[:3000]], fixed=True),
                     lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=False),
                     lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=True),
                     lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=False),
                     lambda: m.process(dpcm, halo=1)]:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == L.ERROR_UNSUPPORTED
        assert not os.path.exists(tmp_path / "a.mfcc")
        # time_dev times what process_i16_dev enqueues, normalization included
        out = torch.empty((1, m.num_frames(len(pcm)), 13), device="cuda")
        assert m.time_launches(dpcm[None, :], out, warmup=1, iters=2) > 0
        torch.cuda.synchronize()
        want = m.process(pcm)
        assert same_bits(out[0].cpu().numpy(), want)
        # NONE again: the bits of a handle that never normalized
        m.set_normalize(None)
        assert m.normalize is None
        back = m.process(pcm)
        with m.stream() as s:                                             # sessions are allowed again
            s.push(pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream") as fresh:
        assert same_bits(back, fresh.process(pcm))
        with fresh.stream() as s:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                fresh.set_normalize("mean")
            assert e.value.code == L.ERROR_BUSY
            s.push(pcm)
        fresh.set_normalize("mean")
        assert fresh.normalize == "mean"
        nr.check(fresh.process(pcm), back, [0, len(back)], "mean", "after BUSY")


def test_non_default_torch_stream_is_honoured(mfcc_amd, wav_pcm):
    import torch
    pcm = all_kinds(512 + 170 * 3000, 9, wav_pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar") as m, \
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
            m.normalize_rows(rows, per_channel(len(pcm), x.shape[1]))
        s.synchronize()
        assert same_bits(y.cpu().numpy(), want)
        assert same_bits(rows.cpu().numpy(), want.reshape(-1, 13))
