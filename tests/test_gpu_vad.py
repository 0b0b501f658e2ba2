"""Energy VAD and voiced-frame selection (``MFCC(vad="select")``, ``mfcc_hip_vad_dev``, ``mfcc_hip_select_dev``) on the
GPU: the decision of every kernel family's own raw rows against the reference of tests/vad_ref.py under its set-aside
rule, crafted rows through both direct entries (exact masks, ``rows[mask]`` bit for bit), the handle mode against
``full[mask]`` across the ragged host / device / per-utterance / chunked entry points, full-size runs that repeat bit
for bit, and the refusals of the paths a selecting handle does not cover."""
import ctypes as C
import os

import numpy as np
import pytest

import kernel_families as kf
import vad_ref as vr

pytestmark = pytest.mark.gpu

PARAM_SETS = {
    "defaults": dict(vr.DEFAULTS),
    "mean_ctx5": dict(energy_threshold=0.0, energy_mean_scale=1.0, frames_context=5, proportion_threshold=0.6),
    "mean_ctx2_p12": dict(energy_threshold=0.0, energy_mean_scale=1.0, frames_context=2, proportion_threshold=0.12),
    "nothing": dict(energy_threshold=1e6, energy_mean_scale=0.0, frames_context=3, proportion_threshold=0.6),
    "everything": dict(energy_threshold=-1e6, energy_mean_scale=0.0, frames_context=3, proportion_threshold=0.6),
}
KW = dict(nfft=512, nfilters=32, nceptrums=13)


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def same_bits(a, b):
    a, b = np.ascontiguousarray(np_of(a), np.float32), np.ascontiguousarray(np_of(b), np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def np_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def unaligned(torch, a):
    """``a`` on the device, its first element 4 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == t.element_size()
    return t


# ------------------------------------------------------------------- 1. every float kernel family
@pytest.mark.parametrize("fam", kf.FLOAT, ids=[f.id for f in kf.FLOAT])
def test_every_kernel_family_against_the_reference(mfcc_amd, wav_pcm, fam):
    import torch
    wav = np.asarray(wav_pcm, np.int16)
    n = len(wav) if fam.hop > 1 else 20000
    wav = wav[:n]
    holes = wav.copy()
    for a, length in ((n // 7, 4 * fam.nfft), (n // 2, fam.nfft // 2), ((3 * n) // 4, 3 * fam.nfft + 11)):
        holes[a:a + length] = 0                                             # silent frames: -inf / NaN rows
    q = n // 4
    gains = np.concatenate([np.clip(np.rint(wav[:q].astype(np.float64) * g), -32768, 32767).astype(np.int16)
                            for g in (1.0, 0.05, 0.5, 0.01)])               # one utterance, four loudness levels
    noise = kf.signal("noise", n, 11, wav)
    utts = [wav, holes, gains, noise]
    with kf.open_handle(mfcc_amd, fam) as m:
        rows = [m.process(u) for u in utts]                                 # the family's own raw rows
        off = offsets_of([len(r) for r in rows])
        x = np.concatenate(rows)
        assert not np.isfinite(rows[1][:, 0]).all()
        t = torch.from_numpy(x).cuda()
        for name, ps in PARAM_SETS.items():
            got = np_of(m.vad_rows(t, off, column=0, **ps))
            share, voiced = vr.compare(got, x, off.astype(np.int64), 0, "%s %s" % (fam.id, name), **ps)
            print("%s %s: %d frames, voiced share %.3f, set aside %.2g" % (fam.id, name, len(x), voiced, share))
            if name == "nothing":
                assert not got.any()
            if name == "everything":
                assert got.any() and not got.all()                          # all but the silent frames' windows
        # another column of the same rows is another decision
        last = x.shape[1] - 1
        got = np_of(m.vad_rows(t, off, column=last, energy_threshold=0.0, energy_mean_scale=1.0))
        vr.compare(got, x, off.astype(np.int64), last, "%s last column" % fam.id, energy_threshold=0.0,
                   energy_mean_scale=1.0)


# ------------------------------------------------------------------- 2. crafted rows through mfcc_hip_vad_dev
def _crafted_column(rng, R):
    """0 / 10 in runs, alternations and isolated frames, with -inf / NaN sprinkled in: with threshold 1, scale 0.5 the
    threshold lies in [1, 6] whatever the mean is, so every value is far from it and the mask is exact."""
    e = np.zeros(R, np.float32)
    i = 0
    while i < R:
        kind, length = int(rng.integers(0, 4)), int(rng.integers(1, 700))
        seg = e[i:i + length]
        if kind == 0:
            seg[:] = 10.0
        elif kind == 1:
            seg[::2] = 10.0                                                  # alternating frames
        elif kind == 2:
            seg[rng.random(len(seg)) < 0.3] = 10.0
        i += length
    e[rng.choice(R, R // 40, replace=False)] = -np.inf
    e[rng.choice(R, R // 60, replace=False)] = np.nan
    return e


def _crafted_lengths(ctx, tile):
    lens = [0, 1, 2, ctx, ctx + 1, 2 * ctx + 1, 63, 64, 65, 255, 256, 257]
    for t in (tile, 2 * tile, 4096):                                         # the decision's tiles and the mean's
        lens += [t - 1, t, t + 1]
    return [v for v in lens if v >= 0] + [0, 5000]


@pytest.mark.parametrize("ctx", [0, 1, 5, 64])
@pytest.mark.parametrize("width", [1, 13, 40, 64])
def test_vad_dev_on_crafted_rows(mfcc_amd, width, ctx):
    import torch
    rng = np.random.default_rng(width * 1000 + ctx)
    col = width // 2
    with mfcc_amd.MFCC(**KW) as m:
        for form in ("table", "uniform"):
            lens = _crafted_lengths(ctx, 1024) if form == "table" else [1025] * 7
            rng.shuffle(lens)
            off = (3 + offsets_of(lens)).astype(np.uint64)                  # the first segment starts at row 3
            R = int(off[-1]) + 4
            x = rng.standard_normal((R, width)).astype(np.float32) * 100
            x[:, col] = _crafted_column(rng, R)
            for s in range(1, len(off)):                                     # patterns that flip across tile edges
                a = int(off[s - 1])
                for edge in range(1024, int(off[s]) - a, 1024):
                    x[a + edge - 2:a + edge + 2, col] = [10.0, 0.0, 10.0, 0.0]
            t = unaligned(torch, x)
            for ps in (dict(energy_threshold=5.0, energy_mean_scale=0.0), dict(energy_threshold=1.0, energy_mean_scale=0.5)):
                for p in (0.6, 0.25):
                    ps = dict(ps, frames_context=ctx, proportion_threshold=p)
                    out = torch.full((R,), 7, dtype=torch.uint8, device="cuda")
                    if form == "uniform":                                    # (segments, rows, width), no offsets
                        got3 = m.vad_rows(t[3:3 + 7 * 1025].view(7, 1025, width), column=col, **ps)
                        out[3:3 + 7 * 1025] = got3.reshape(-1)
                    else:
                        assert m.vad_rows(t, off, column=col, out=out, **ps) is out
                    got = np_of(out)
                    a, b = int(off[0]), int(off[-1])
                    assert (got[:a] == 7).all() and (got[b:] == 7).all()    # bytes outside the segments untouched
                    ref, may = vr.vad(x[a:b], off.astype(np.int64) - a, col, **ps)
                    assert not may.any()
                    assert np.array_equal(got[a:b], ref), (form, ps, np.flatnonzero(got[a:b] != ref)[:5])
                    assert 0 < ref.sum() < len(ref)


# ------------------------------------------------------------------- 3. crafted rows through mfcc_hip_select_dev
def _crafted_mask(rng, R):
    m = np.zeros(R, np.uint8)
    i = 0
    while i < R:
        kind, length = int(rng.integers(0, 4)), int(rng.integers(1, 900))
        seg = m[i:i + length]
        if kind == 0:
            seg[:] = 1
        elif kind == 1:
            seg[::2] = 1
        elif kind == 2:
            seg[rng.random(len(seg)) < 0.5] = 200                            # any non-zero byte selects
        i += length
    return m


@pytest.mark.parametrize("width", [1, 13, 39, 120, 192])
def test_select_dev_on_crafted_rows(mfcc_amd, width):
    import torch
    rng = np.random.default_rng(width)
    tile = min(1024, 4088 // width)
    sentinel = np.float32(-12345.5)
    with mfcc_amd.MFCC(**KW) as m:
        for form in ("table", "uniform"):
            lens = [0, 1, 2, 5, tile - 1, tile, tile + 1, 2 * tile + 1, 0, 3000, 1, 777] if form == "table" \
                else [tile + 1] * 9
            rng.shuffle(lens)
            off = (2 + offsets_of(lens)).astype(np.uint64)
            R = int(off[-1]) + 3
            x = rng.standard_normal((R, width)).astype(np.float32)
            x[rng.choice(R, R // 30, replace=False), 0] = np.nan
            x[rng.choice(R, R // 30, replace=False), width - 1] = -np.inf
            mask = _crafted_mask(rng, R)
            a, b = int(off[0]), int(off[-1])
            for s in range(1, len(off)):                                     # patterns that flip across tile edges
                for edge in range(tile, int(off[s]) - int(off[s - 1]), tile):
                    mask[int(off[s - 1]) + edge - 2:int(off[s - 1]) + edge + 2] = [1, 0, 1, 0]
            if form == "table":
                s0, s1 = int(off[3]), int(off[4])
                mask[s0:s1] = 0                                              # a segment with nothing voiced
            t, v = unaligned(torch, x), unaligned(torch, mask)
            want = x[a:b][mask[a:b] != 0]
            want_off = np.array([np.count_nonzero(mask[a:int(o)]) for o in off], np.uint64)
            for shift in (0, 1, 2, 3):                                       # every 4-byte alignment of the output
                buf = torch.full(((b - a) * width + 4,), float(sentinel), device="cuda")
                out = buf[shift:shift + (b - a) * width].view(b - a, width)
                if form == "uniform":
                    n = len(lens)
                    got, oo = m.select_rows(t[a:b].view(n, tile + 1, width), v[a:b].view(n, tile + 1), out=out)
                else:
                    got, oo = m.select_rows(t, v, off, out=out)
                assert got.data_ptr() == out.data_ptr() and len(got) == len(want)
                assert np.array_equal(oo, want_off), (form, oo, want_off)
                assert same_bits(got, want)
                rest = np_of(buf)
                assert (rest[:shift] == sentinel).all() and (rest[shift + len(want) * width:] == sentinel).all()
            got, oo = m.select_rows(t, v, off) if form == "table" else \
                m.select_rows(t[a:b].view(len(lens), tile + 1, width), v[a:b].view(len(lens), tile + 1))
            assert same_bits(got, want) and np.array_equal(oo, want_off)
            # nothing voiced, everything voiced
            zero, ones = torch.zeros(R, dtype=torch.uint8, device="cuda"), torch.ones(R, dtype=torch.uint8, device="cuda")
            got, oo = m.select_rows(t, zero, off)
            assert got.shape == (0, width) and not oo.any()
            got, oo = m.select_rows(t, ones, off)
            assert same_bits(got, x[a:b]) and np.array_equal(oo, off - off[0])


def test_vad_and_select_dev_arguments(mfcc_amd):
    import torch
    from mfcc_amd import _lib as L
    lib = mfcc_amd.load_library()
    with mfcc_amd.MFCC(**KW) as m:
        t = torch.zeros((10, 13), device="cuda")
        v = torch.zeros(10, dtype=torch.uint8, device="cuda")
        o = torch.zeros((10, 13), device="cuda")
        oo = (C.c_size_t * 3)(9, 9, 9)
        p, q, r = C.c_void_p(t.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(o.data_ptr())
        good = (C.c_size_t * 3)(0, 4, 8)
        bad = (C.c_size_t * 3)(0, 6, 4)

        def vad(rows=p, width=13, column=0, off=good, n=2, thr=5.0, scale=0.5, ctx=0, prop=0.6, out=q):
            return lib.mfcc_hip_vad_dev(m._h, rows, width, column, off, n, thr, scale, ctx, prop, out)

        def sel(rows=p, width=13, mask=q, off=good, n=2, out=r, cap=10, offs=oo):
            return lib.mfcc_hip_select_dev(m._h, rows, width, mask, off, n, out, cap, offs)

        assert vad() == L.SUCCESS and sel() == L.SUCCESS and list(oo) == [0, 0, 0]
        for kw in [dict(off=bad), dict(width=0), dict(width=65), dict(column=-1), dict(column=13), dict(ctx=-1), dict(ctx=65),
                   dict(prop=0.0), dict(prop=1.0), dict(prop=float("nan")), dict(scale=-0.5), dict(scale=float("inf")),
                   dict(thr=float("nan")), dict(thr=float("inf")), dict(rows=None), dict(out=None), dict(off=None),
                   dict(rows=C.c_void_p(t.data_ptr() + 2)),
                   dict(rows=C.c_void_p(v.data_ptr())), dict(out=C.c_void_p(t.data_ptr() + 16))]:   # overlapping
            assert vad(**kw) == L.ERROR_INVALID_PARAM, kw
        for kw in [dict(off=bad), dict(width=0), dict(width=193), dict(rows=None), dict(mask=None), dict(out=None),
                   dict(off=None), dict(offs=None), dict(rows=C.c_void_p(t.data_ptr() + 2)),
                   dict(out=C.c_void_p(o.data_ptr() + 2)), dict(out=p), dict(out=C.c_void_p(t.data_ptr() + 52 * 7)),
                   dict(mask=C.c_void_p(o.data_ptr() + 3))]:
            assert sel(**kw) == L.ERROR_INVALID_PARAM, kw
        assert sel(cap=7) == L.ERROR_BUFFER_SMALL and sel(cap=8) == L.SUCCESS
        assert vad(rows=None, off=None, n=0, out=None) == L.SUCCESS          # n_segs = 0: a no-op
        assert sel(rows=None, mask=None, off=None, n=0, out=None, offs=None) == L.SUCCESS
        for args in [(2, 0, 5.0, 0.5, 0, 0.6), (-1, 0, 5.0, 0.5, 0, 0.6), (1, 13, 5.0, 0.5, 0, 0.6), (1, -1, 5.0, 0.5, 0, 0.6),
                     (1, 0, float("nan"), 0.5, 0, 0.6), (1, 0, 5.0, -1.0, 0, 0.6), (1, 0, 5.0, 0.5, 65, 0.6),
                     (1, 0, 5.0, 0.5, 0, 1.0), (0, 0, 5.0, 0.5, 0, 0.0)]:
            assert lib.mfcc_hip_set_vad(m._h, *args) == L.ERROR_INVALID_PARAM, args
        with pytest.raises(ValueError):
            m.vad_rows(t, column=13)
        with pytest.raises(ValueError):
            m.select_rows(t, torch.zeros(9, dtype=torch.uint8, device="cuda"))
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.select_rows(t, v, out=torch.zeros((9, 13), device="cuda"))
        assert e.value.code == L.ERROR_BUFFER_SMALL
        torch.cuda.synchronize()
        assert not o.any() and m.vad is None
    with mfcc_amd.MFCC(output="logmel", **KW) as m:                         # the column is checked against n_mel there
        m.set_vad("select", column=31)
        assert m.vad == "select" and m.vad_column == 31
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.set_vad("select", column=32)
        assert e.value.code == L.ERROR_INVALID_PARAM and m.vad_column == 31


# ------------------------------------------------------------------- 4. the handle mode
CONFIGS = {
    "plain": dict(),
    "meanvar": dict(normalize="meanvar"),
    "sliding": dict(normalize="meanvar", normalize_window=600),
    "deltas": dict(deltas=2),
    "sliding_deltas": dict(normalize="meanvar", normalize_window=600, deltas=2),
}
# threshold 0.5 + the utterance's mean: an utterance of ONE frame has e = mean exactly, and with threshold 0 that frame
# would sit on theta -- undecided by the rule of tests/vad_ref.py, which these inputs must not be
HANDLE_VAD = dict(energy_threshold=0.5, energy_mean_scale=1.0, frames_context=5, proportion_threshold=0.6)


def _corpus(wav_pcm, seed=7):
    rng = np.random.default_rng(seed)
    wav = np.asarray(wav_pcm, np.int16)
    lens = [0, 511, 512, 517, 37, 682, 20000] + [int(v) for v in rng.integers(0, 30000, 170)] + \
        [160000, 96013, 480000, 33333, 70001]
    utts = []
    for i, n in enumerate(lens):
        u = np.resize(wav[(i * 977) % 50000:], n).astype(np.int16) if i % 3 else kf.signal("silences", n, i, wav)
        if i % 9 == 4 and n > 2000:
            u[:1500] = 0                                                     # leading silence: -inf / NaN rows
        utts.append(u)
    utts[6][:] = 0                                                           # frames, none of them voiced
    return utts


@pytest.mark.parametrize("config", list(CONFIGS))
def test_handle_mode_equals_full_rows_under_the_mask(mfcc_amd, wav_pcm, config, monkeypatch):
    import torch
    cfg = CONFIGS[config]
    utts = _corpus(wav_pcm)
    vkw = {"vad_" + k: v for k, v in HANDLE_VAD.items()}
    with mfcc_amd.MFCC(**KW) as raw, mfcc_amd.MFCC(**KW, **cfg) as full, \
            mfcc_amd.MFCC(vad="select", **KW, **cfg, **vkw) as m:
        assert m.vad == "select" and m.num_features == full.num_features
        raw_rows = raw.process_batch(utts)
        full_rows = full.process_batch(utts)
        fo = offsets_of([len(r) for r in raw_rows])
        x = np.concatenate(raw_rows)
        mask = np_of(m.vad_rows(torch.from_numpy(x).cuda(), fo, column=0, **HANDLE_VAD))
        vr.compare(mask, x, fo.astype(np.int64), 0, config, **HANDLE_VAD)
        want = [full_rows[i][mask[int(fo[i]):int(fo[i + 1])] != 0] for i in range(len(utts))]
        host = m.process_batch(utts)
        dev = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        packed, pfo = m.process_packed(torch.from_numpy(np.concatenate(utts)).cuda(),
                                       offsets_of([len(u) for u in utts]))
        one = [m.process(u) for u in utts]
        one_dev = [m.process(torch.from_numpy(u).cuda()) for u in utts[:40]]
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "4")                    # several chunks of whole utterances
        chunked = m.process_batch(utts)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        again = m.process_batch(utts)
        torch.cuda.synchronize()
    total = sum(len(w) for w in want)
    assert 0.2 < total / len(x) < 0.8, total / len(x)
    assert len(raw_rows[6]) > 0 and len(want[6]) == 0                        # an utterance with no voiced frame
    assert sum(len(w) == 0 for w in want) >= 4 and any(0 < len(w) < len(r) for w, r in zip(want, raw_rows))
    assert packed.shape == (total, m.num_features) and int(pfo[-1]) == total
    for i in range(len(utts)):
        assert host[i].shape == (len(want[i]), full.num_features), i
        assert same_bits(host[i], want[i]), i
        assert same_bits(dev[i], want[i]) and same_bits(one[i], want[i]), i
        assert same_bits(chunked[i], want[i]) and same_bits(again[i], want[i]), i
        assert same_bits(packed[int(pfo[i]):int(pfo[i + 1])], want[i]), i
        if i < len(one_dev):
            assert same_bits(one_dev[i], want[i]), i


def test_handle_mode_on_equal_lengths_and_logmel(mfcc_amd, wav_pcm):
    """Equal lengths run as channels of one launch (the uniform form of every pass); a log-mel handle names its band."""
    import torch
    wav = np.asarray(wav_pcm, np.int16)
    utts = [np.ascontiguousarray(wav[i * 3000:i * 3000 + 40000]) for i in range(24)]
    utts[5] = np.zeros(40000, np.int16)
    for kw in (dict(KW), dict(KW, output="logmel")):
        col = 0 if "output" not in kw else 20
        vad = dict(HANDLE_VAD, frames_context=64)
        with mfcc_amd.MFCC(normalize="mean", deltas=1, **kw) as full, mfcc_amd.MFCC(**kw) as raw, \
                mfcc_amd.MFCC(normalize="mean", deltas=1, vad="select", vad_column=col,
                              **{"vad_" + k: v for k, v in vad.items()}, **kw) as m:
            x = raw.process(np.stack(utts))
            f = full.process(np.stack(utts))
            mask = np_of(m.vad_rows(torch.from_numpy(x).cuda(), column=col, **vad))
            vr.compare(mask.reshape(-1), x.reshape(-1, x.shape[-1]), np.arange(25) * x.shape[1], col, "equal", **vad)
            host = m.process_batch(utts)
            dev = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        assert len(host[5]) == 0 and 0 < mask.mean() < 1
        for i in range(24):
            assert same_bits(host[i], f[i][mask[i] != 0]) and same_bits(dev[i], host[i]), i


# ------------------------------------------------------------------- 5. full size, and a second run
def test_config5_full_size_through_the_handle(mfcc_amd):
    """10 000 utterances of five lengths, loud and quiet stretches of noise; every frame against the reference."""
    import torch
    n_utt, n, block = 10_000, 160_000, 8_000
    g = torch.Generator(device="cuda").manual_seed(5)
    flat = torch.empty(n_utt * n, dtype=torch.int16, device="cuda")
    for c0 in range(0, n_utt, 1000):
        amp = torch.where(torch.rand(1000 * n // block, device="cuda", generator=g) < 0.5, 30.0, 3000.0)
        noise = torch.randn((1000 * n // block, block), device="cuda", generator=g) * amp[:, None]
        flat[c0 * n:(c0 + 1000) * n] = noise.clamp_(-32768, 32767).to(torch.int16).reshape(-1)
    del noise, amp
    lens = np.array([n - 997 * (u % 5) for u in range(n_utt)], np.int64)
    starts = np.arange(n_utt, dtype=np.int64) * n
    utts = [flat[int(s):int(s + k)] for s, k in zip(starts, lens)]
    vkw = {"vad_" + k: v for k, v in HANDLE_VAD.items()}
    with mfcc_amd.MFCC(**KW) as raw, mfcc_amd.MFCC(vad="select", normalize="meanvar", deltas=2, **KW, **vkw) as m, \
            mfcc_amd.MFCC(normalize="meanvar", deltas=2, **KW) as full:
        x = raw.process_batch(utts)
        fo = offsets_of([len(r) for r in x])
        total = int(fo[-1])
        assert total > 9_200_000
        dense = torch.as_strided(x[0], (total, 13), (13, 1))
        mask1 = m.vad_rows(dense, fo, **HANDLE_VAD)
        mask2 = m.vad_rows(dense, fo, **HANDLE_VAD)
        assert torch.equal(mask1, mask2)
        c0 = dense[:, 0].cpu().numpy()
        del x, dense
        got1 = m.process_batch(utts)
        sizes1 = [len(r) for r in got1]
        n_sel = sum(sizes1)
        first = torch.as_strided(got1[0], (n_sel, 39), (39, 1)).clone()
        del got1
        got2 = m.process_batch(utts)
        assert [len(r) for r in got2] == sizes1
        assert torch.equal(first.view(torch.int32), torch.as_strided(got2[0], (n_sel, 39), (39, 1)).view(torch.int32))
        mask = mask1.cpu().numpy()
        share, voiced = vr.compare(mask, c0, fo.astype(np.int64), 0, "config 5", **HANDLE_VAD)
        print("config 5: %d frames, voiced share %.4f, set aside %.3g" % (total, voiced, share))
        assert n_sel == int(np.count_nonzero(mask)) and 0.2 < voiced < 0.8
        assert sizes1 == [int(v) for v in np.add.reduceat(mask.astype(np.int64), fo[:-1].astype(np.int64))]
        for u in (0, 1, 4, 4999, 9999):                                      # spot check of the rows themselves
            f = full.process(utts[u])
            mu = torch.from_numpy(mask[int(fo[u]):int(fo[u + 1])] != 0).cuda()
            assert torch.equal(got2[u].view(torch.int32), f[mu].view(torch.int32)), u


def test_config2_rows_through_the_direct_entries(mfcc_amd):
    import torch
    nch, n = 64, 9_600_000
    g = torch.Generator(device="cuda").manual_seed(3)
    pcm = torch.randn((nch, n), device="cuda", generator=g)
    pcm *= torch.where(torch.rand((nch, n // 8000), device="cuda", generator=g) < 0.4, 30.0, 3000.0).repeat_interleave(8000, 1)
    pcm = pcm.clamp_(-32768, 32767).to(torch.int16)
    pcm[:, 1_000_000:1_200_000] = 0                                          # silent frames: -inf / NaN rows
    with mfcc_amd.MFCC(**KW) as m:
        x = m.process(pcm)
        del pcm
        assert x.shape == (64, 56_468, 13)
        for name in ("defaults", "mean_ctx5"):
            ps = PARAM_SETS[name]
            v1, v2 = m.vad_rows(x, **ps), m.vad_rows(x, **ps)
            y1, o1 = m.select_rows(x, v1)
            y2, o2 = m.select_rows(x, v2)
            assert torch.equal(v1, v2) and np.array_equal(o1, o2) and torch.equal(y1.view(torch.int32), y2.view(torch.int32))
            mask = v1.cpu().numpy()
            rows = x.cpu().numpy()
            assert not np.isfinite(rows[:, :, 0]).all()
            share, voiced = vr.compare(mask.reshape(-1), rows.reshape(-1, 13), np.arange(65) * 56_468, 0,
                                       "config 2 " + name, **ps)
            print("config 2 %s: voiced share %.4f, set aside %.3g" % (name, voiced, share))
            assert np.array_equal(o1, np.concatenate([[0], np.cumsum(mask.sum(axis=1, dtype=np.int64))]).astype(np.uint64))
            for c in (0, 31, 63):                                            # spot check of the rows
                assert same_bits(y1[int(o1[c]):int(o1[c + 1])], rows[c][mask[c] != 0]), c
            assert y1.shape == (int(o1[-1]), 13)


# ------------------------------------------------------------------- 6. refusals and state
def test_refusals_busy_and_state(mfcc_amd, wav_pcm, golden_dir, tmp_path):
    import torch
    from mfcc_amd import _lib as L
    pcm = np.ascontiguousarray(wav_pcm[:512 + 170 * 200], np.int16)
    dpcm = torch.from_numpy(pcm).cuda()
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    with mfcc_amd.MFCC(pad_mode="stream", vad="select", vad_energy_threshold=0.0, vad_energy_mean_scale=1.0, **KW) as m:
        assert m.num_features == 13
        out = torch.empty((1, m.num_frames(len(pcm)), 13), device="cuda")
        for call in [lambda: m.process_fixed(pcm), lambda: m.process_fixed(dpcm), lambda: m.stream(),
                     lambda: m.stream(fixed=True),
                     lambda: m.process_batch([pcm, pcm[:3000]], fixed=True),
                     lambda: m.process_batch([dpcm, dpcm[:3000]], fixed=True),
                     lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=False),
                     lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=True),
                     lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=False),
                     lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=True),
                     lambda: m.process(np.stack([pcm, pcm])), lambda: m.process(torch.stack([dpcm, dpcm])),
                     lambda: m.process(dpcm, halo=1),
                     lambda: m.time_launches(dpcm[None, :], out, warmup=1, iters=2)]:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == L.ERROR_UNSUPPORTED
        with pytest.raises(mfcc_amd.MfccHipError, match="process_batch"):
            m.process(np.stack([pcm, pcm]))
        assert not os.path.exists(tmp_path / "a.mfcc") and not os.path.exists(tmp_path / "b.mfcc")
        sel = m.process(pcm)
        assert 0 < len(sel) < m.num_frames(len(pcm))
        # a buffer too small for every frame: the counts of all frames, as with VAD off
        fo = np.zeros(2, np.uint64)
        off = np.array([0, len(pcm)], np.uint64)
        small = np.empty(len(sel) * 13, np.float32)
        rc = m._lib.mfcc_hip_process_ragged_i16(m._h, pcm.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), 1,
                                                small.ctypes.data_as(C.c_void_p), small.size, fo.ctypes.data_as(C.c_void_p))
        assert rc == L.ERROR_BUFFER_SMALL and int(fo[1]) == m.num_frames(len(pcm))
        # off again: the bits of a handle that never selected
        m.set_vad(None)
        assert m.vad is None
        back = m.process(pcm)
        with m.stream() as s:                                               # sessions are allowed again
            s.push(pcm)
    with mfcc_amd.MFCC(pad_mode="stream", **KW) as fresh:
        want = fresh.process(pcm)
        assert same_bits(back, want)
        with fresh.stream() as s:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                fresh.set_vad("select")
            assert e.value.code == L.ERROR_BUSY
            s.push(pcm)
        assert fresh.vad is None
        fresh.set_vad("select", 0, 0.0, 1.0, 2, 0.5)
        assert (fresh.vad, fresh.vad_frames_context, fresh.vad_proportion_threshold) == ("select", 2, 0.5)
        mask = vr.segment(want[:, 0], 0.0, 1.0, 2, 0.5)[0]
        assert same_bits(fresh.process(pcm), want[mask != 0])


def test_non_default_torch_stream_is_honoured(mfcc_amd, wav_pcm):
    import torch
    utts = _corpus(wav_pcm)[:60]
    vkw = {"vad_" + k: v for k, v in HANDLE_VAD.items()}
    with mfcc_amd.MFCC(vad="select", deltas=2, **KW, **vkw) as m, mfcc_amd.MFCC(**KW) as raw:
        want = m.process_batch(utts)
        x = raw.process_batch(utts)
        fo = offsets_of([len(r) for r in x])
        s = torch.cuda.Stream()
        flat_h = torch.from_numpy(np.concatenate(utts)).pin_memory()
        rows_h = torch.from_numpy(np.concatenate(x)).pin_memory()
        with torch.cuda.stream(s):
            flat = flat_h.to("cuda", non_blocking=True)                      # produced on s, consumed on s
            y, yfo = m.process_packed(flat, offsets_of([len(u) for u in utts]))
            rows = rows_h.to("cuda", non_blocking=True)
            mask = m.vad_rows(rows, fo, **HANDLE_VAD)
            z, zfo = m.select_rows(rows, mask, fo)
        s.synchronize()
        assert [int(v) for v in yfo] == [int(v) for v in offsets_of([len(w) for w in want])]
        assert same_bits(y, np.concatenate(want)) and np.array_equal(zfo, yfo)
        assert same_bits(z, np.concatenate(x)[np_of(mask) != 0])
