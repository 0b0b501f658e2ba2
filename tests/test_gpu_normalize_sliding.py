"""Sliding-window normalization (``MFCC(normalize_window=...)``, ``mfcc_hip_normalize_sliding_dev``) on the GPU, case
by case as tests/test_gpu_normalize.py (whose signals, kernel families and corpus it uses): every element within the
bound of tests/normalize_sliding_ref.py of the handle's own raw rows, the end-to-end result within a bound derived
from oracle/error_bound.py, bit-identity across the dense, ragged, host, device and chunked entry points and across
runs, crafted rows through the direct entry, deltas on top, and the refusals of the paths it does not cover."""
import ctypes as C
import os

import numpy as np
import pytest

import normalize_ref as nr
import normalize_sliding_ref as sr
import test_gpu_normalize as tn
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu
MODES = tn.MODES
WINDOWS = {"centered600": (600, 100, True), "causal600": (600, 100, False), "centered7": (7, 3, True)}
same_bits, per_channel = tn.same_bits, tn.per_channel


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def wkw(N, M, center):
    return dict(normalize_window=N, normalize_min_window=M, normalize_center=center)


# ------------------------------------------------------------------- 1. every float kernel family, both modes
@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", list(tn.FAMILIES))
def test_every_kernel_family_within_the_bound_of_its_raw_rows(mfcc_amd, wav_pcm, family, mode, win):
    import torch
    kw = tn.FAMILIES[family]
    N, M, center = WINDOWS[win]
    nfft = kw["nfft"]
    pcm = tn.all_kinds(nfft + (nfft // 3) * 700 + 37, 3, wav_pcm)
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(normalize=mode, **wkw(N, M, center), **kw) as m:
        assert (m.normalize, m.normalize_window, m.normalize_min_window, m.normalize_center) == (mode, N, M, center)
        assert m.kernel_name() == raw.kernel_name()
        x, y = raw.process(pcm), m.process(pcm)
        xw, yw = raw.process(wav_pcm), m.process(wav_pcm)
        yd = m.process(torch.from_numpy(pcm).cuda())
        torch.cuda.synchronize()
    nch, nf, w = x.shape
    assert y.shape == x.shape and w == m.num_features
    worst = sr.check(y.reshape(-1, w), x.reshape(-1, w), per_channel(nch, nf), mode, N, M, center,
                     "%s %s %s" % (family, mode, win))
    worst_w = sr.check(yw, xw, [0, len(xw)], mode, N, M, center, "%s %s %s golden wav" % (family, mode, win))
    print("%s %s %s: worst %.3f / %.3f (wav) of the bound" % (family, mode, win, worst, worst_w))
    assert same_bits(yd.cpu().numpy(), y)


# ------------------------------------------------------------------- 2. end to end against the float64 oracle
def _window_mean(v, a, b):
    cs = np.concatenate([np.zeros((1,) + v.shape[1:]), np.cumsum(v, axis=0)])
    return (cs[b] - cs[a]) / (b - a)[:, None]


@pytest.mark.parametrize("win", ["centered600", "causal600"])
def test_end_to_end_against_the_normalized_oracle(mfcc_amd, wav_pcm, win):
    """The bound of tests/test_gpu_normalize.py::test_end_to_end_against_the_normalized_oracle, per row with the
    row's own window: x = kernel rows, r = oracle rows, |x - r| <= b elementwise.  For row i with window [a, b):
    |mu_x - mu_r| <= mean_{[a, b)} b and |sigma_x - sigma_r| <= rms_{[a, b)} b, so
        |y - z| <= (b_ij + mean_i b) / sigma_i + |z_ij| rms_i(b) / sigma_i        (to first order in b / sigma)
    plus the normalization's own rounding; the factor 1.25 on the first part covers the second-order terms.  (b is
    positive: its prefix sums lose nothing.)"""
    N, M, center = WINDOWS[win]
    n = 512 + 170 * 1499
    pcm = np.stack([np.resize(wav_pcm, n).astype(np.int16), tn.signal("noise3000", n, 1, wav_pcm),
                    tn.signal("sine", n, 2, wav_pcm)])
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar", **wkw(N, M, center)) as m:
        got = m.process(pcm)
        model = eb.model_of(m.kernel_name())
    for c in range(len(pcm)):
        ref, b = eb.reference_and_bound(pcm[c], model, n_cep=13)
        assert np.isfinite(ref).all() and np.isfinite(b).all()
        z, mu, sd = sr.normalize(ref, [0, len(ref)], "meanvar", N, M, center)
        wa, wb = sr._windows_np(len(ref), N, M, center)
        mean_b, rms_b = _window_mean(b, wa, wb), np.sqrt(_window_mean(b * b, wa, wb))
        tol = ((b + mean_b) / sd + np.abs(z) * rms_b / sd) * 1.25 + sr.bound(ref, mu, sd)
        err = np.abs(got[c].astype(np.float64) - z)
        print("%s channel %d: worst %.3g of the bound" % (win, c, float((err / tol).max())))
        assert (err <= tol).all(), "channel %d: worst %.3g of the bound" % (c, float((err / tol).max()))


# ------------------------------------------------------------------- 3. ragged: host and device = per utterance
@pytest.mark.parametrize("center", [True, False], ids=["centered", "causal"])
@pytest.mark.parametrize("kw", [dict(nfft=256, nfilters=32, nceptrums=13, pad_mode="stream"),
                                dict(nfft=256, nfilters=32, nceptrums=13, pad_mode="notebook"),
                                dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream")],
                         ids=["generic256_stream", "generic256_notebook", "fused512_stream"])
def test_ragged_host_and_device_equal_per_utterance(mfcc_amd, wav_pcm, kw, center):
    import torch
    utts = tn._corpus(wav_pcm, kw["nfft"], kw["nfft"] // 3)
    with mfcc_amd.MFCC(normalize="meanvar", **wkw(600, 100, center), **kw) as m, mfcc_amd.MFCC(**kw) as raw:
        one = [m.process(u) for u in utts]
        host = m.process_batch(utts)
        dev = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        torch.cuda.synchronize()
        raw_rows = [raw.process(u) for u in utts]
    assert len(one) == len(host) == len(dev) == len(utts)
    assert sum(len(r) == 1 for r in one) >= 2 and any(0 < len(r) < 600 for r in one) and any(len(r) > 600 for r in one)
    if kw["pad_mode"] == "notebook":
        assert any(len(r) == 0 for r in one)
    assert any(not np.isfinite(r).all() for r in raw_rows)
    for i in range(len(utts)):
        assert same_bits(host[i], one[i]), i
        assert same_bits(dev[i].cpu().numpy(), one[i]), i
        if len(one[i]):
            sr.check(one[i], raw_rows[i], [0, len(one[i])], "meanvar", 600, 100, center, "utterance %d" % i)


# ------------------------------------------------------------------- 4. dense: host = device = per channel, chunking
def test_dense_host_device_and_per_channel_agree_under_chunking(mfcc_amd, wav_pcm, monkeypatch):
    import torch
    pcm = tn.all_kinds(16000 * 30, 21, wav_pcm)[:6]                       # 6 x 960 KB: one channel per 1 MB chunk
    hour = tn.signal("silences", 16000 * 3600, 5, wav_pcm)                # frame-range chunks cut it
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar", **wkw(600, 100, True)) as m:
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
    assert same_bits(whole_h, dev_h) and same_bits(chunked_h, dev_h)     # a chunk edge is not a segment edge


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
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(normalize="meanvar", **wkw(600, 100, True), **kw) as m:
        x = raw.process(pcm)
        y1 = m.process(pcm)
        y2 = m.process(pcm)
        torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    nf, w = x.shape[1], x.shape[2]
    assert (nf, w) == ((56_468, 13) if cfg == "config2" else (168_912, 40))
    del pcm, y2
    x, y = x.cpu().numpy(), y1.cpu().numpy()
    assert not np.isfinite(x).all()
    worst = 0.0
    for c0 in range(0, nch, 8):                                            # 8 channels at a time: host memory
        c1 = min(nch, c0 + 8)
        worst = max(worst, sr.check(y[c0:c1].reshape(-1, w), x[c0:c1].reshape(-1, w), per_channel(c1 - c0, nf),
                                    "meanvar", 600, 100, True, cfg))
    print("%s: worst %.3f of the bound" % (cfg, worst))


# ------------------------------------------------------------------- 6. the direct entry on crafted rows
def _crafted(width, N, rng):
    run = min(max(N // 4, 32), 256)               # the tile of the pass: G runs of run_rows(N) rows
    tile = (256 // width) * run
    lens = [0, 1, 2, 3, N - 1, N, N + 1, tile - 1, tile, tile + 1, 0, 2 * tile + 5, 20011]
    off = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.uint64)      # the first segment starts at row 3
    R = int(off[-1]) + 4
    x = (rng.standard_normal((R, width)) * rng.uniform(0.5, 40, width) + rng.uniform(-50, 50, width)).astype(np.float32)
    if width >= 5:
        x[:, 0] = -3.5
        x[:, 1] = np.nan
        x[:, 2] = -np.inf
        x[:, 3] = (1e4 + 1e-2 * rng.standard_normal(R)).astype(np.float32)
        step = int(off[-2]) + 10000                                        # halfway through the last segment
        x[:step, 4] = 0.0
        x[step:, 4] = (1e4 + 1e-2 * rng.standard_normal(R - step)).astype(np.float32)
    if width >= 7:
        # ... and the step down: 1e4 + 1e-2 noise, then 1e-3 noise around 0, where |mu| no longer widens the bound
        x[:step, 5] = (1e4 + 1e-2 * rng.standard_normal(step)).astype(np.float32)
        x[step:, 5] = (1e-3 * rng.standard_normal(R - step)).astype(np.float32)
    x[rng.choice(R, R // 50, replace=False), width - 1] = np.nan
    return x, off


@pytest.mark.parametrize("center", [True, False], ids=["centered", "causal"])
@pytest.mark.parametrize("N", [1, 2, 600, 16384])
@pytest.mark.parametrize("width", [1, 13, 64])
@pytest.mark.parametrize("mode", MODES)
def test_normalize_sliding_dev_on_crafted_rows(mfcc_amd, width, mode, N, center):
    import torch
    M = min(100, N)
    x, off = _crafted(width, N, np.random.default_rng(width))
    sentinel = np.float32(-12345.5)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        t = torch.from_numpy(x).cuda()
        out = torch.full(x.shape, float(sentinel), device="cuda")
        assert m.normalize_rows(t, off, mode=mode, window=N, min_window=M, center=center, out=out) is out
        # the same segments at another alignment: input shifted by one float, output by three
        big = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)])).cuda()[1:].view(x.shape)
        obig = torch.full((x.size + 3,), float(sentinel), device="cuda")[3:].view(x.shape)
        assert big.data_ptr() % 16 == 4 and obig.data_ptr() % 16 == 12 and t.data_ptr() % 16 == 0
        m.normalize_rows(big, off, mode=mode, window=N, min_window=M, center=center, out=obig)
        # no segments, and mode NONE: no-ops
        out0 = torch.full(x.shape, float(sentinel), device="cuda")
        m.normalize_rows(t, np.array([5], np.uint64), mode=mode, window=N, min_window=M, center=center, out=out0)
        m.normalize_rows(t, off, mode=None, window=N, min_window=M, center=center, out=out0)
        torch.cuda.synchronize()
        y, y_shift, y0, x_after = out.cpu().numpy(), obig.cpu().numpy(), out0.cpu().numpy(), t.cpu().numpy()
    assert same_bits(x_after, x)                                            # the input is left alone
    assert (y0 == sentinel).all()
    assert same_bits(y_shift, y)
    a, b = int(off[0]), int(off[-1])
    assert (y[:a] == sentinel).all() and (y[b:] == sentinel).all()          # rows outside the segments untouched
    worst = sr.check(y[a:b], x[a:b], off.astype(np.int64) - a, mode, N, M, center, "width %d N %d" % (width, N))
    print("width %d %s N %d %s: worst %.3f of the bound" % (width, mode, N, "centered" if center else "causal", worst))
    if width >= 5:
        assert np.all(y[a:b, 0] == 0.0)
        assert np.isnan(y[a:b, 1]).all() and np.isneginf(y[a:b, 2]).all()


# ------------------------------------------------------------------- 7. a window of twice the segment
def test_a_centered_window_of_twice_the_segment_is_within_the_bound_of_the_per_segment_result(mfcc_amd, wav_pcm):
    pcm = tn.all_kinds(512 + 170 * 700 + 37, 3, wav_pcm)
    kw = dict(nfft=512, nfilters=32, nceptrums=13)
    with mfcc_amd.MFCC(**kw) as raw, mfcc_amd.MFCC(normalize="meanvar", normalize_window=1600, **kw) as m:
        x, y = raw.process(pcm), m.process(pcm)
    nch, nf, w = x.shape
    assert 2 * nf <= 1600
    nr.check(y.reshape(-1, w), x.reshape(-1, w), per_channel(nch, nf), "meanvar", "N >= 2 T")


# ------------------------------------------------------------------- 8. deltas on top
@pytest.mark.parametrize("center", [True, False], ids=["centered", "causal"])
def test_deltas_run_on_the_sliding_normalized_statics(mfcc_amd, wav_pcm, center):
    import torch
    kw = dict(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar", **wkw(600, 100, center))
    pcm = tn.all_kinds(512 + 170 * 1500 + 37, 4, wav_pcm)
    utts = tn._corpus(wav_pcm, 512, 170)[:60]
    with mfcc_amd.MFCC(deltas=2, **kw) as m, mfcc_amd.MFCC(**kw) as st:
        y, s = m.process(pcm), st.process(pcm)
        yd = m.process(torch.from_numpy(pcm).cuda())
        want = st.deltas_rows(torch.from_numpy(s).cuda(), order=2, window=2)
        rag, rag_s = m.process_batch(utts), st.process_batch(utts)
        rag_d = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        fo = np.concatenate([[0], np.cumsum([len(r) for r in rag_s])]).astype(np.uint64)
        want_r = st.deltas_rows(torch.from_numpy(np.concatenate(rag_s)).cuda(), fo, order=2, window=2)
        torch.cuda.synchronize()
    assert y.shape[-1] == 39 and same_bits(y[..., :13], s)
    assert same_bits(y, want.cpu().numpy()) and same_bits(yd.cpu().numpy(), y)
    assert same_bits(np.concatenate(rag), want_r.cpu().numpy())
    assert same_bits(np.concatenate([r.cpu().numpy() for r in rag_d]), np.concatenate(rag))


# ------------------------------------------------------------------- 9. arguments, refusals and state
def test_entry_point_arguments(mfcc_amd):
    import torch
    from mfcc_amd import _lib as L
    lib = mfcc_amd.load_library()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        t = torch.zeros((10, 13), device="cuda")
        o = torch.zeros((20, 13), device="cuda")
        p, q = C.c_void_p(t.data_ptr()), C.c_void_p(o.data_ptr())
        fn = lib.mfcc_hip_normalize_sliding_dev
        off = (C.c_size_t * 3)(0, 6, 4)
        assert fn(m._h, p, 13, q, off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM                  # decreasing
        off = (C.c_size_t * 3)(0, 4, 8)
        for width, mode, N, M, center in [(0, 2, 600, 100, 1), (65, 2, 600, 100, 1), (13, 3, 600, 100, 1),
                                          (13, -1, 600, 100, 1), (13, 2, 0, 1, 1), (13, 2, 16385, 100, 1),
                                          (13, 2, 50, 51, 1), (13, 2, 50, 0, 1), (13, 2, 600, 100, 2),
                                          (13, 2, 600, 100, -1)]:
            assert fn(m._h, p, width, q, off, 2, mode, N, M, center) == L.ERROR_INVALID_PARAM
        assert fn(m._h, None, 13, q, off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM
        assert fn(m._h, p, 13, None, off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM
        assert fn(m._h, C.c_void_p(t.data_ptr() + 2), 13, q, off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM
        assert fn(m._h, p, 13, C.c_void_p(o.data_ptr() + 2), off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM
        assert fn(m._h, p, 13, p, off, 2, 2, 600, 100, 1) == L.ERROR_INVALID_PARAM                  # in place
        assert fn(m._h, q, 13, C.c_void_p(o.data_ptr() + 4 * 13 * 3), off, 2, 2, 600, 100, 1) == \
            L.ERROR_INVALID_PARAM                                                                   # overlapping
        assert fn(m._h, None, 13, None, None, 0, 2, 600, 100, 1) == L.SUCCESS
        assert fn(m._h, None, 13, None, off, 2, 0, 600, 100, 1) == L.SUCCESS                        # mode NONE
        for N, M, center in [(-1, 1, 1), (16385, 100, 1), (50, 51, 1), (50, 0, 1), (600, 100, 2)]:
            assert lib.mfcc_hip_set_normalize_window(m._h, N, M, center) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_set_normalize_window(m._h, 0, 0, 1) == L.SUCCESS                        # off
        with pytest.raises(ValueError):
            m.normalize_rows(t, window=0)
        with pytest.raises(ValueError):
            m.normalize_rows(t, window=600, out=torch.zeros((10, 12), device="cuda"))
        with pytest.raises(ValueError):
            m.normalize_rows(t, out=torch.zeros((10, 13), device="cuda"))
        torch.cuda.synchronize()
        assert not o.any() and not t.any() and m.normalize_window is None


def test_refusals_busy_and_state(mfcc_amd, wav_pcm, golden_dir, tmp_path):
    import torch
    from mfcc_amd import _lib as L
    pcm = wav_pcm[:512 + 170 * 900].copy()
    dpcm = torch.from_numpy(pcm).cuda()
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    kw = dict(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream")
    with mfcc_amd.MFCC(normalize="meanvar", **wkw(600, 100, False), **kw) as m:
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
        # time_dev times what process_i16_dev enqueues, the sliding pass included
        out = torch.empty((1, m.num_frames(len(pcm)), 13), device="cuda")
        assert m.time_launches(dpcm[None, :], out, warmup=1, iters=2) > 0
        torch.cuda.synchronize()
        want = m.process(pcm)
        assert same_bits(out[0].cpu().numpy(), want)
        # window off: the per-segment bits; mode off: the raw bits
        m.set_normalize_window(None)
        assert m.normalize_window is None
        per_segment = m.process(pcm)
        m.set_normalize_window(600, center=False)
        m.set_normalize(None)
        back = m.process(pcm)                                             # a window with mode NONE has no effect
        with m.stream() as s:                                             # sessions are allowed again
            s.push(pcm)
    with mfcc_amd.MFCC(normalize="meanvar", **kw) as ps, mfcc_amd.MFCC(**kw) as fresh:
        assert same_bits(per_segment, ps.process(pcm))
        assert same_bits(back, fresh.process(pcm))
        assert not same_bits(want, per_segment)
        sr.check(want, back, [0, len(back)], "meanvar", 600, 100, False, "causal handle")
        with fresh.stream() as s:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                fresh.set_normalize_window(600)
            assert e.value.code == L.ERROR_BUSY
            s.push(pcm)
        assert fresh.normalize_window is None
        fresh.set_normalize_window(300, 50)
        fresh.set_normalize("mean")
        assert (fresh.normalize_window, fresh.normalize_min_window, fresh.normalize_center) == (300, 50, True)
        sr.check(fresh.process(pcm), back, [0, len(back)], "mean", 300, 50, True, "after BUSY")


def test_non_default_torch_stream_is_honoured(mfcc_amd, wav_pcm):
    import torch
    pcm = tn.all_kinds(512 + 170 * 3000, 9, wav_pcm)
    kw = dict(nfft=512, nfilters=32, nceptrums=13)
    with mfcc_amd.MFCC(normalize="meanvar", normalize_window=600, **kw) as m, mfcc_amd.MFCC(**kw) as raw:
        want = m.process(pcm)
        x = raw.process(pcm)
        s = torch.cuda.Stream()
        host = torch.from_numpy(pcm).pin_memory()
        rows_h = torch.from_numpy(x.reshape(-1, 13).copy()).pin_memory()
        with torch.cuda.stream(s):
            d = host.to("cuda", non_blocking=True)                        # produced on s, consumed on s
            y = m.process(d)
            rows = rows_h.to("cuda", non_blocking=True)
            z = m.normalize_rows(rows, per_channel(len(pcm), x.shape[1]), window=600)
        s.synchronize()
        assert same_bits(y.cpu().numpy(), want)
        assert same_bits(z.cpu().numpy(), want.reshape(-1, 13))
