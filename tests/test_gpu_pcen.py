"""PCEN on the GPU (``MFCC(output="logmel", pcen=...)`` / ``mfcc_hip_set_pcen`` / ``mfcc_hip_pcen_dev``).

* P1  the kernels' direct entry against the float64 definition of tests/pcen_ref.py under its constant C;
* P2  one segment's result is the same bits alone, inside ragged batches, as a channel of a dense call, through every
      entry point, with the host call cut into frame-range chunks, and from ``pcen_rows`` on the handle's raw rows;
* P3  through handles of every log-mel kernel family, the definition applied to the same handle's raw rows;
* P4  composition and order: PCEN, then normalization, then deltas; the VAD decides on the raw rows;
* P5  the refusals, and ``set_pcen(None)`` restores the raw bits.

Shapes are the smallest at which the kernels can go wrong: segments of 0, 1, 2 rows and one row around one and two
tiles of 128, a carry chain of 20 tiles, widths 1 / 13 (19 tiles per workgroup) / 40 / 64, a base pointer that is 4- but
not 16-byte aligned, silent entries, a band silent in frame 0, a wholly silent segment."""
import ctypes as C

import numpy as np
import pytest

import kernel_families as kf
import pcen_ref as pr
from kernel_families import same

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 127, 128, 129, 255, 256, 257, 128 * 20 + 5, 130]        # the last one is wholly silent
FRONT, BACK = 3, 2                                                       # rows outside the segments
KW512 = dict(nfft=512, nfilters=32, nceptrums=13, output="logmel")


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _params(ps):
    return dict(zip(("s", "alpha", "delta", "r", "eps"), ps))


def _rows(W, seed):
    """Log2 energies in [-8, 24] in segments of LENS behind FRONT rows, 3 % silent entries, column 0 of the long
    segment silent in its frame 0, the last segment silent throughout."""
    rng = np.random.default_rng(seed)
    off = FRONT + np.concatenate([[0], np.cumsum(LENS)])
    x = rng.uniform(-8, 24, (int(off[-1]) + BACK, W)).astype(np.float32)
    x[rng.random(x.shape) < 0.03] = -np.inf
    x[off[9], 0] = -np.inf
    x[off[10]:off[11]] = -np.inf
    x[FRONT + 1, W - 1] = np.nan                                         # any non-finite value counts as silence
    return x, off.astype(np.uint64)


def _misaligned(x):
    """``x`` on the device at an address that is 4 but not 16 bytes aligned."""
    import torch
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    t = flat[1:].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------ P1

@pytest.fixture(scope="module")
def raw_handle(mfcc_amd):
    with mfcc_amd.MFCC(**KW512) as m:
        yield m


@pytest.mark.parametrize("W", [1, 13, 40, 64])
def test_p1_direct_entry_meets_the_definition(raw_handle, W):
    import torch
    m = raw_handle
    x, off = _rows(W, seed=W)
    inside = np.zeros(len(x), bool)
    inside[int(off[0]):int(off[-1])] = True
    for ps in pr.PARAM_SETS:
        t = _misaligned(x)
        assert m.pcen_rows(t, off, **_params(ps)) is t
        got = t.cpu().numpy()
        # rows outside the segments: the same bits
        assert same(got[~inside], x[~inside]), (W, ps)
        ref = pr.pcen_f64(x, off, *ps)
        e = pr.check(got, ref, ps[2], ps[3], rows=inside, what="W %d %r" % (W, ps))
        print("P1 W %d %r: worst %.3g of %.3g" % (W, ps, e, pr.C))
        assert np.all(got[int(off[10]):int(off[11])] == 0.0)             # the silent segment
        # the same bits at a 16-byte aligned address, and on a second run
        a = torch.from_numpy(x).cuda()
        assert a.data_ptr() % 16 == 0
        assert same(m.pcen_rows(a, off, **_params(ps)), got)
        assert same(m.pcen_rows(_misaligned(x), off, **_params(ps)), got)


def test_p1_segment_bits_do_not_depend_on_the_batch(raw_handle):
    """Every segment of the ragged call alone (the uniform form of the tile plan), and all of them as equal-length
    channels of a 3-D tensor."""
    import torch
    m = raw_handle
    x, off = _rows(40, seed=7)
    got = m.pcen_rows(torch.from_numpy(x).cuda(), off).cpu().numpy()
    for k in range(len(LENS)):
        a, b = int(off[k]), int(off[k + 1])
        if b > a:
            alone = m.pcen_rows(torch.from_numpy(x[a:b].copy()).cuda()).cpu().numpy()
            assert same(alone, got[a:b]), LENS[k]
    a = int(off[9])
    dense = np.stack([x[a:a + 300], x[a + 5:a + 305], x[a:a + 300]])
    d = m.pcen_rows(torch.from_numpy(dense).cuda()).cpu().numpy()
    assert same(d[0], got[a:a + 300]) and same(d[2], d[0]) and not same(d[1], d[0])
    # no segments: a no-op
    e = torch.from_numpy(x).cuda()
    m.pcen_rows(e, np.array([5], np.uint64))
    assert same(e, x)


# ------------------------------------------------------------------------------------------------ P2

def test_p2_one_segment_same_bits_everywhere(mfcc_amd, wav_pcm, monkeypatch):
    import torch
    fam = kf.FLOAT[0]
    x = kf.silent_stream(fam, 300, 3)                                    # three tiles, -inf rows
    y = kf.signal("speech", 512 + 170 * 140, 4, wav_pcm)
    z = kf.signal("noise", len(x), 5, wav_pcm)
    with mfcc_amd.MFCC(**KW512, pcen=True) as m, mfcc_amd.MFCC(**KW512) as raw:
        assert m.pcen == dict(zip(("s", "alpha", "delta", "r", "eps"), (pr.f32(v) for v in pr.DEFAULTS)))
        r = raw.process(x)
        assert np.isinf(r).any()
        one = m.process(x)                                               # the host-buffer entry
        assert one.shape == r.shape == (300, 32) and np.isfinite(one).all()
        pr.check(one, pr.pcen_f64(r), pr.DEFAULTS[2], pr.DEFAULTS[3], what="process")
        assert same(m.process(torch.from_numpy(x).cuda()), one)          # the device entry
        # a channel of a dense call, host and device
        dense = np.stack([z, x, z])
        assert same(m.process(dense)[1], one) and same(m.process(torch.from_numpy(dense).cuda())[1], one)
        # inside ragged batches at several positions
        empty = x[:0]
        for batch, where in (([x, y, z], 0), ([y, empty, x, z[:700]], 2), ([z[:100], y, y, x], 3)):
            assert same(m.process_batch(batch)[where], one), where
            got = m.process_batch([torch.from_numpy(b).cuda() for b in batch])
            assert same(got[where], one), where
        flat = np.concatenate([y, x, z])
        offs = np.cumsum([0, len(y), len(x), len(z)]).astype(np.uint64)
        rows, fo = m.process_packed(torch.from_numpy(flat).cuda(), offs)
        assert same(rows[int(fo[1]):int(fo[2])], one)
        # pcen_rows on the handle's own raw rows
        assert same(raw.pcen_rows(raw.process(torch.from_numpy(x).cuda())), one)
        # the host call cut into frame-range chunks of 1 MB: a long channel is still ONE segment
        long = np.resize(x, 1_300_003)
        whole = m.process(torch.from_numpy(long).cuda()).cpu().numpy()
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        assert same(m.process(long), whole)
        assert same(m.process(np.stack([long, long[::-1]]))[0], whole)
        assert same(m.process(np.stack([z, x, z, x, z]))[3], one)        # whole channels per chunk
        assert same(m.process_batch([long[:700_000], x, long[:600_001]])[1], one)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        assert same(whole[:128], one[:128])                              # and tiles do not look ahead


# ------------------------------------------------------------------------------------------------ P3

ASR = dict(nfft=512, hop=160, win_length=400, nceptrums=13)
FAMILIES = {
    "f512_w12": (dict(nfft=512, nfilters=32, nceptrums=13), "mfcc_fused512_w12_kernel"),
    "f512_16f": (dict(nfft=512, nfilters=16, nceptrums=16), "mfcc_fused512_w12_kernel"),
    "k400_h160": (dict(ASR, nfilters=32), "mfcc_fused512_h160_kernel"),
    "g512_h160": (dict(nfft=512, hop=160, nfilters=32, nceptrums=13), "mfcc_float_generic_kernel"),
    "htk64_mb": (dict(ASR, nfilters=64, mel="htk", fmin=0, fmax=8000), "mfcc_fused512_h160_mb_kernel"),
    "f1024": (dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0), "mfcc_fused1024_w12bf_kernel"),
    "g256": (dict(nfft=256, nfilters=20, nceptrums=13, power_scale=0), "mfcc_float_generic_kernel"),
}


@pytest.mark.parametrize("frames", [37, 300])
@pytest.mark.parametrize("fid", list(FAMILIES))
def test_p3_every_logmel_kernel_family(mfcc_amd, wav_pcm, fid, frames):
    kw, kernel = FAMILIES[fid]
    ps = pr.PARAM_SETS[1]
    with mfcc_amd.MFCC(**kw, output="logmel") as m:
        assert m.kernel_name() == kernel, m.kernel_name()
        n = m.hop * (frames - 1) + m.win_length
        pcm = np.stack([kf.signal("speech", n, 3, wav_pcm), kf.signal("silences", n, 4, wav_pcm)])
        pcm[1, :m.win_length + m.hop] = 0                                # silent from frame 0: C_0 = 0 in every band
        raw = m.process(pcm)
        assert raw.shape[1] == frames and np.isinf(raw[1, 0]).all()
        m.set_pcen(_params(ps))
        got = m.process(pcm)
        assert same(m.process_batch(list(pcm))[1], got[1])
        for c in range(2):
            e = pr.check(got[c], pr.pcen_f64(raw[c], None, *ps), ps[2], ps[3], what="%s channel %d" % (fid, c))
            print("P3 %s %d frames channel %d: worst %.3g of %.3g" % (fid, frames, c, e, pr.C))


# ------------------------------------------------------------------------------------------------ P4

def test_p4_pcen_then_normalization_then_deltas(mfcc_amd, wav_pcm):
    import torch
    fam = kf.FLOAT[0]
    xs = [kf.silent_stream(fam, 300, 8), kf.signal("speech", 512 + 170 * 36, 9, wav_pcm)]
    with mfcc_amd.MFCC(**KW512, pcen=True) as p, \
            mfcc_amd.MFCC(**KW512, pcen=True, normalize="meanvar", deltas=2) as m, \
            mfcc_amd.MFCC(**KW512, pcen=True, normalize="mean", normalize_window=50, normalize_center=False,
                          normalize_min_window=1, deltas=1) as s:
        for x in xs:
            d = torch.from_numpy(x).cuda()
            rows = p.process(d)
            want = p.deltas_rows(p.normalize_rows(rows.clone(), mode="meanvar"), order=2, window=2)
            assert same(m.process(d), want) and same(m.process(x), want)
            want = p.deltas_rows(p.normalize_rows(rows, mode="mean", window=50, min_window=1, center=False), order=1)
            assert same(s.process(d), want) and same(s.process(x), want)
        got = m.process_batch(xs)
        for x, g in zip(xs, got):
            assert same(g, m.process(x))


def test_p4_vad_decides_on_the_raw_rows(mfcc_amd, wav_pcm):
    import torch
    xs = [kf.signal("silences", 512 + 170 * 299, 12, wav_pcm), kf.signal("speech", 512 + 170 * 150, 13, wav_pcm)]
    vad = dict(vad="select", vad_column=3, vad_energy_threshold=0.0, vad_energy_mean_scale=1.0, vad_frames_context=2)
    differs = []
    with mfcc_amd.MFCC(**KW512, **vad) as v, mfcc_amd.MFCC(**KW512, pcen=True, **vad) as vp, \
            mfcc_amd.MFCC(**KW512, pcen=True) as p, mfcc_amd.MFCC(**KW512) as raw:
        for x in xs:
            kept, all_raw, all_pcen = v.process(x), raw.process(x), p.process(x)
            got = vp.process(x)
            assert 0 < len(kept) < len(all_raw) and len(got) == len(kept)
            # the frames kept are those the decision on the RAW rows keeps, as PCEN rows of the WHOLE utterance
            mask = raw.vad_rows(torch.from_numpy(all_raw).cuda(), column=3, energy_threshold=0.0, energy_mean_scale=1.0,
                                frames_context=2).cpu().numpy().astype(bool)
            assert same(kept, all_raw[mask])
            assert same(got, all_pcen[mask])
            wrong = raw.vad_rows(torch.from_numpy(all_pcen).cuda(), column=3, energy_threshold=0.0, energy_mean_scale=1.0,
                                 frames_context=2).cpu().numpy().astype(bool)
            differs.append(not np.array_equal(wrong, mask))
        assert any(differs)                                              # a decision on the PCEN rows would differ
        both = vp.process_batch(xs)
        assert same(both[0], vp.process(xs[0])) and same(both[1], vp.process(xs[1]))


# ------------------------------------------------------------------------------------------------ P5

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_p5_refusals(mfcc_amd, wav_pcm, tmp_path):
    import torch
    from mfcc_amd import _lib as L
    lib = mfcc_amd.load_library()
    x = np.ascontiguousarray(wav_pcm[:4000])
    # a cepstra handle has no log2 energies
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as c:
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            c.set_pcen(True)
        assert e.value.code == L.ERROR_UNSUPPORTED and c.pcen is None
        c.set_pcen(None)                                                 # off is always accepted
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            c.stream_bank(2, pcen=True)
        assert e.value.code == L.ERROR_UNSUPPORTED
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pcen=True)
    assert e.value.code == L.ERROR_UNSUPPORTED
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=32, pad_mode="stream", output="logmel", pcen=True) as m:
        d = torch.from_numpy(x).cuda()
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.process(d, halo=1)
        assert e.value.code == L.ERROR_UNSUPPORTED
        for call in (lambda: m.process_fixed(x), lambda: m.process_fixed(d), lambda: m.process_batch([x], fixed=True),
                     lambda: m.stream(), lambda: m.stream_bank(2), lambda: m.stream_bank(2, deltas=1),
                     lambda: m.stream_bank(2, pcen=True),
                     lambda: m.convert(str(tmp_path / "a.wav"), str(tmp_path / "a.mfcc"), fixed=False),
                     lambda: m.convert_many([str(tmp_path / "a.wav")], [str(tmp_path / "a.mfcc")], fixed=False)):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == L.ERROR_UNSUPPORTED
        # bad parameter blocks
        ok = L.Pcen()
        assert lib.mfcc_hip_pcen_defaults(C.byref(ok)) == 0
        rows = torch.zeros((8, 13), device="cuda")
        off = np.array([0, 8], np.uint64)
        for field, v in (("s", 0.0), ("s", 1.5), ("alpha", -0.1), ("delta", -1.0), ("r", 0.0), ("eps", 0.0),
                         ("eps", float("nan")), ("struct_size", 40)):
            bad = L.Pcen.from_buffer_copy(ok)
            setattr(bad, field, v)
            assert lib.mfcc_hip_set_pcen(m._h, C.byref(bad)) == L.ERROR_INVALID_PARAM, field
            assert lib.mfcc_hip_pcen_dev(m._h, C.c_void_p(rows.data_ptr()), 13, _ptr(off), 1, C.byref(bad)) == \
                L.ERROR_INVALID_PARAM, field
        assert lib.mfcc_hip_pcen_dev(m._h, C.c_void_p(rows.data_ptr()), 13, _ptr(off), 1, None) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_pcen_dev(m._h, C.c_void_p(rows.data_ptr()), 65, _ptr(off), 1, C.byref(ok)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_pcen_dev(m._h, C.c_void_p(rows.data_ptr()), 0, _ptr(off), 1, C.byref(ok)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_pcen_dev(m._h, C.c_void_p(rows.data_ptr() + 2), 13, _ptr(off), 1, C.byref(ok)) == \
            L.ERROR_INVALID_PARAM
        dec = np.array([8, 0], np.uint64)
        assert lib.mfcc_hip_pcen_dev(m._h, C.c_void_p(rows.data_ptr()), 13, _ptr(dec), 1, C.byref(ok)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_pcen_dev(m._h, None, 13, None, 0, C.byref(ok)) == 0          # no segments: a no-op
        torch.cuda.synchronize()
        assert float(rows.abs().sum()) == 0.0
        with pytest.raises(ValueError):
            m.pcen_rows(rows, off, s=2)


def test_p5_busy_with_a_live_session_and_off_restores_the_raw_bits(mfcc_amd, wav_pcm):
    import torch
    from mfcc_amd import _lib as L
    x = kf.silent_stream(kf.FLOAT[0], 140, 21)
    batch = [x, x[:3000], x[:0]]
    with mfcc_amd.MFCC(**KW512) as m:
        raw = m.process(x)
        raw_dev = m.process(torch.from_numpy(x).cuda()).cpu().numpy()
        raw_batch = m.process_batch(batch)
        with m.stream() as s:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.set_pcen(True)
            assert e.value.code == L.ERROR_BUSY and m.pcen is None
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.set_pcen(None)
            assert e.value.code == L.ERROR_BUSY
            first = s.push(x[:2000])
        assert same(first, raw[:len(first)])
        m.set_pcen(True, r=0.25)
        assert m.pcen["r"] == 0.25 and not same(m.process(x), raw)
        m.set_pcen(None)
        assert m.pcen is None
        assert same(m.process(x), raw) and same(m.process(torch.from_numpy(x).cuda()), raw_dev)
        for a, b in zip(m.process_batch(batch), raw_batch):
            assert same(a, b)
        with m.stream() as s:                                            # sessions are open to it again
            assert same(s.push(x[:2000]), first)
        # time_launches times the pass too: it runs, with PCEN on and off
        d = torch.from_numpy(np.stack([x, x])).cuda()
        out = torch.empty((2, 140, 32), device="cuda")
        m.set_pcen(True)
        assert m.time_launches(d, out, warmup=1, iters=2) > 0
        assert same(out[0], m.process(x))
