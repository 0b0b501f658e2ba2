"""The filterbank post-passes (``MFCC.set_filterbank(W, ..., normalize=, normalize_window=, deltas=, pcen=)`` /
``mfcc_hip_set_filterbank_post``): utterance and sliding CMVN, deltas and PCEN behind the one-shot filterbank calls, on
rows of up to 128 bands -- the wide kernels of mfcc_amd/csrc/post_wide.hip at 65 .. 128, the narrow ones at 64.

* 1  per-segment normalization under ``normalize_ref.check`` against the raw rows of the same handle, on segments around
     the stats tile ``T = 8192 // W``; at 64 bands bit-equal to ``normalize_rows``;
* 2  sliding normalization and PCEN: bit-equal to the column-slice oracle (the raw rows cut into slices of at most 64
     columns, each through ``normalize_rows(window=...)`` / ``pcen_rows``), and under the float64 references;
* 3  deltas: bit-equal to ``deltas_ref.emulate32`` and to the column-slice oracle through ``deltas_rows``, on segments
     around the delta tile, into views at every float offset inside sentinel rows;
* 4  the chain (PCEN + causal meanvar 40 + 2 x 2 deltas): every entry point, every chunking and every input stage give
     the same bits;
* 5  more tiles than workgroups for the wide delta and stats kernels;
* 6  refusals and state."""
import ctypes as C

import numpy as np
import pytest

import deltas_ref as dr
import fbank_ref as fr
import kernel_families as kf
import normalize_ref as nr
import normalize_sliding_ref as ns
import pcen_ref as pr
from kernel_families import same

pytestmark = pytest.mark.gpu
FUSED, GENERIC = "mfcc_fbank512_kernel", "mfcc_fbank_generic_kernel"
CFGS = {"512_170_512": (512, 170, 512), "512_160_400": (512, 160, 400), "256_80_200": (256, 80, 200)}
KERNEL = {"512_170_512": FUSED, "512_160_400": FUSED, "256_80_200": GENERIC}
BANDS = [64, 65, 80, 128]
EMPTY = 63                                                         # the empty band of the 128-band matrix: a -inf column
PCEN = dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6)
CHAIN = dict(pcen=PCEN, normalize="meanvar", normalize_window=40, normalize_min_window=1, normalize_center=False, deltas=2,
             delta_window=2)
UNSUPPORTED, INVALID, BUSY = -105, -101, -104                      # include/mfcc_hip.h
NARROW_LDS, WIDE_LDS = 4096, 13312                                # mfcc_amd/csrc/post_plan.hpp: floats of the delta kernels' LDS


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    from mfcc_amd import _lib as L
    assert (L.ERROR_UNSUPPORTED, L.ERROR_INVALID_PARAM, L.ERROR_BUSY) == (UNSUPPORTED, INVALID, BUSY)
    return mfcc_amd


def matrix(bands, nfft):
    """HTK in log2; at 128 bands a dense random matrix with one empty band, floor 0: a -inf column"""
    if bands == 128:
        W = fr.dense_random(128, nfft)
        W[EMPTY] = 0.0
        return W
    return fr.htk_weights(bands, nfft)


def open_fb(mfcc_amd, cid, bands, **over):
    nfft, hop, flen = CFGS[cid]
    kw = dict(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    if nfft != 512:
        kw["power_scale"] = 0
    if flen != nfft:
        kw["win_length"] = flen
    kw.update(over)
    m = mfcc_amd.MFCC(**kw)
    try:
        m.W = matrix(bands, nfft)
        m.set_filterbank(m.W)
        assert m.filterbank_kernel_name() == KERNEL[cid] and m.num_bands == m.num_filterbank_columns == bands
    except BaseException:
        m.close()
        raise
    return m


def corpus(cid, frames, wav_pcm, seed=0):
    """(flat CUDA int16, sample offsets) of utterances with these frame counts (0: an utterance too short for a frame)"""
    import torch
    _, hop, flen = CFGS[cid]
    kinds = ["speech", "noise", "silences", "uniform"]
    xs = [kf.signal(kinds[u % 4], flen + hop * (n - 1) if n else flen // 2, seed + u, wav_pcm) for u, n in enumerate(frames)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
    return torch.from_numpy(np.concatenate(xs + [np.zeros(8, np.int16)])).cuda()[:int(off[-1])], off, xs


def packed(m, flat, off, frames=None, **kw):
    import torch
    rows, fo = m.filterbank_packed(flat, off, **kw)
    torch.cuda.synchronize()
    if frames is not None:
        assert np.array_equal(np.diff(fo.astype(np.int64)), frames)
    return rows, fo


def slices(m, rows, fo, pcen=None, norm=None, deltas=None, width=64):
    """The column-slice oracle: the raw rows (a CUDA tensor, segments fo) cut into slices of at most ``width`` columns, each
    through the direct entries in the chain's order, put back as [s | D | DD] of the full width."""
    import torch
    W = rows.shape[1]
    order = deltas[0] if deltas else 0
    if not len(rows):
        return rows.new_zeros((0, W * (1 + order)))
    parts = [[] for _ in range(1 + order)]
    for a in range(0, W, width):
        s = rows[:, a:a + width].clone()                          # PCEN works in place: never on the caller's rows
        w = int(s.shape[1])
        if pcen:
            m.pcen_rows(s, fo, **pcen)
        if norm:
            s = m.normalize_rows(s, fo, **norm)
        if deltas:
            e = m.deltas_rows(s, fo, order=deltas[0], window=deltas[1])
            for k in range(1 + order):
                parts[k].append(e[:, k * w:(k + 1) * w])
        else:
            parts[0].append(s)
    out = torch.cat([torch.cat(p, dim=1) for p in parts], dim=1)
    torch.cuda.synchronize()
    return out


def delta_tile(W, order, window):
    per = ((NARROW_LDS if W <= 64 else WIDE_LDS) - 8) // W
    return (per - 2 * window) // 3 if order == 1 else (per - 6 * window) // 5


# ------------------------------------------------------------------------------------------------ 1

@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("cid", list(CFGS))
def test_1_per_segment_normalization(mfcc_amd, wav_pcm, cid, bands):
    T = 8192 // bands
    frames = [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3]      # a partial tile; more tiles than the G stripes of finalize
    flat, off, _ = corpus(cid, frames, wav_pcm, seed=bands)
    with open_fb(mfcc_amd, cid, bands) as m:
        raw, fo = packed(m, flat, off, frames)
        raw_np = raw.cpu().numpy()
        if bands == 128:
            assert np.isneginf(raw_np[:, EMPTY]).all()
        for mode in ("mean", "meanvar"):
            m.set_filterbank(m.W, normalize=mode)
            assert m.num_filterbank_columns == bands
            got, fo2 = packed(m, flat, off, frames)
            assert np.array_equal(fo, fo2)
            worst = nr.check(got.cpu().numpy(), raw_np, fo, mode, "%s %d %s" % (cid, bands, mode))   # non-finite: bit for bit
            print("per-segment %s %d bands %s: worst |got - ref| / bound %.3g" % (cid, bands, mode, worst))
            if bands == 64:                                        # the same kernel at the same width
                assert same(got, m.normalize_rows(raw.clone(), fo, mode=mode))
            m.set_filterbank(m.W)
            assert same(packed(m, flat, off)[0], raw)              # ... and none again


# ------------------------------------------------------------------------------------------------ 2

SLIDING = [(40, True, 1), (40, False, 1), (600, True, 100), (600, False, 100), (600, False, 1)]


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("cid", list(CFGS))
def test_2_sliding_normalization(mfcc_amd, wav_pcm, cid, bands):
    # shorter than either window; longer than a run (32 / 150 rows) and than a tile of 256 // W runs
    frames = [17, 0, 39, 41, 700, 1300]
    flat, off, _ = corpus(cid, frames, wav_pcm, seed=100 + bands)
    with open_fb(mfcc_amd, cid, bands) as m:
        raw, fo = packed(m, flat, off, frames)
        raw_np = raw.cpu().numpy()
        for i, (window, center, min_window) in enumerate(SLIDING):
            mode = ("meanvar", "mean")[i % 2]
            m.set_filterbank(m.W, normalize=mode, normalize_window=window, normalize_min_window=min_window, normalize_center=center)
            got = packed(m, flat, off, frames)[0]
            what = "%s %d %s N=%d center=%d M=%d" % (cid, bands, mode, window, center, min_window)
            assert same(got, slices(m, raw, fo, norm=dict(mode=mode, window=window, min_window=min_window, center=center))), what
            if i in (1, 3):                                        # the float64 reference once per window
                ns.check(got.cpu().numpy(), raw_np, fo, mode, window, min_window, center, what)


@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("cid", list(CFGS))
def test_2_pcen(mfcc_amd, wav_pcm, cid, bands):
    import torch
    _, hop, flen = CFGS[cid]
    frames = [127, 128, 129, 3 * 128 + 5, 0, 200]
    flat, off, _ = corpus(cid, frames, wav_pcm, seed=200 + bands)
    flat[int(off[5]):] = 0                                         # the last utterance: silence
    with open_fb(mfcc_amd, cid, bands) as m:
        raw, fo = packed(m, flat, off, frames)
        assert torch.isneginf(raw[int(fo[5]):]).all()              # E = 0 in every band: log2 with floor 0
        m.set_filterbank(m.W, pcen=PCEN)
        got = packed(m, flat, off, frames)[0]
        assert same(got, slices(m, raw, fo, pcen=PCEN))
        ref = pr.pcen_f64(raw.cpu().numpy(), fo, **PCEN)
        worst = pr.check(got.cpu().numpy(), ref, PCEN["delta"], PCEN["r"], what="%s %d" % (cid, bands))
        print("pcen %s %d bands: worst ratio %.3g of allowed %.3g" % (cid, bands, worst, pr.C))
        assert (got[int(fo[5]):] == got[int(fo[5])]).all()         # silence: (0 + delta)^r - delta^r in every frame and band


# ------------------------------------------------------------------------------------------------ 3

@pytest.mark.parametrize("order,window", [(1, 1), (1, 8), (2, 2), (2, 8)])
@pytest.mark.parametrize("bands", BANDS)
def test_3_deltas(mfcc_amd, wav_pcm, bands, order, window):
    import torch
    cid = list(CFGS)[(bands + order + window) % 3]
    g = delta_tile(bands, order, window)
    assert g >= (8 if bands > 64 else 3)
    frames = [1, window, g - 1, g, g + 1, 3 * g + 2, 0, 2]         # neighbours: a clamp must not read across an edge
    flat, off, _ = corpus(cid, frames, wav_pcm, seed=300 + bands)
    with open_fb(mfcc_amd, cid, bands) as m:
        raw, fo = packed(m, flat, off, frames)
        m.set_filterbank(m.W, deltas=order, delta_window=window)
        WO = bands * (1 + order)
        assert m.num_filterbank_columns == WO
        got = packed(m, flat, off, frames)[0]
        assert tuple(got.shape) == (sum(frames), WO)
        assert same(got, slices(m, raw, fo, deltas=(order, window)))
        assert same(got, dr.emulate32(raw.cpu().numpy(), [int(v) for v in fo], order, window)), (cid, bands, order, window)
        # a result at every float offset from a 16-byte boundary, inside sentinel rows
        R = sum(frames)
        for k in range(4):
            big = torch.full(((R + 4) * WO + 8,), 12345.0, device="cuda")
            a = 2 * WO + k
            assert (big.data_ptr() + 4 * a) % 16 == 4 * ((2 * WO + k) % 4)
            view = big[a:a + R * WO].view(R, WO)
            out = packed(m, flat, off, frames, out=view)[0]
            assert out.data_ptr() == view.data_ptr() and same(view, got), k
            assert (big[:a] == 12345.0).all() and (big[a + R * WO:] == 12345.0).all(), k


# ------------------------------------------------------------------------------------------------ 4

def chain_oracle(m, raw, fo):
    return slices(m, raw, fo, pcen=PCEN, norm=dict(mode="meanvar", window=40, min_window=1, center=False), deltas=(2, 2))


@pytest.mark.parametrize("bands", [80, 128])
@pytest.mark.parametrize("cid", list(CFGS))
def test_4_the_chain_from_every_entry_point(mfcc_amd, wav_pcm, cid, bands, monkeypatch):
    import torch
    _, hop, flen = CFGS[cid]
    nf, n = 300, flen + hop * 299
    chans = np.stack([kf.signal(k, n, 7 + u, wav_pcm) for u, k in enumerate(["speech", "silences", "noise"])])
    buf = torch.zeros((3, n + 5), dtype=torch.int16, device="cuda")            # an odd stride
    buf[:, :n] = torch.from_numpy(chans).cuda()
    with open_fb(mfcc_amd, cid, bands) as m:
        raw = m.filterbank(buf[:, :n]).reshape(3 * nf, bands)
        fo = np.arange(4, dtype=np.uint64) * nf
        want = chain_oracle(m, raw, fo).view(3, nf, 3 * bands)
        m.set_filterbank(m.W, **CHAIN)
        assert m.num_filterbank_columns == 3 * bands
        assert same(m.filterbank(buf[:, :n]), want)                                      # dense, 3 channels
        assert same(m.filterbank(buf[1, :n]), want[1])                                   # dense, 1 channel
        rows, fo2 = packed(m, buf[:, :n].contiguous().reshape(-1), np.arange(4) * n, [nf] * 3)       # equal lengths
        assert same(rows.view(3, nf, -1), want)
        # unequal lengths and an empty utterance: pack and gather
        cuts = [n, 0, flen + hop * 99, flen // 2, flen + hop * 160]
        flat = torch.cat([buf[u % 3, :c] for u, c in enumerate(cuts)])
        frames = [nf, 0, 100, 0, 161]
        rows, fo3 = packed(m, flat, np.concatenate([[0], np.cumsum(cuts)]), frames)
        assert same(rows[:nf], want[0])
        for u in (2, 4):
            a, b = int(fo3[u]), int(fo3[u + 1])
            m.set_filterbank(m.W)
            r1 = m.filterbank(buf[u % 3, :cuts[u]])
            one = chain_oracle(m, r1, np.array([0, len(r1)], dtype=np.uint64))
            m.set_filterbank(m.W, **CHAIN)
            assert same(rows[a:b], one) and same(m.filterbank(buf[u % 3, :cuts[u]]), one), u
        host = m.filterbank(chans)                                                       # the host-buffer call
        assert isinstance(host, np.ndarray) and same(host, want)
        # 1 MB chunks: several whole channels per chunk, and frame ranges of one long channel
        many = np.ascontiguousarray(np.tile(chans, (8, 1)))                              # 24 channels of about 96 KB
        long = kf.signal("silences", 700_001, 47, wav_pcm)
        dev_many, dev_long = m.filterbank(torch.from_numpy(many).cuda()), m.filterbank(torch.from_numpy(long).cuda())
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        host_many, host_long = m.filterbank(many), m.filterbank(long)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        assert same(host_many, dev_many), "whole-channel chunks differ from the device call"
        assert same(host_long, dev_long), "frame-range chunks differ from the device call"
        assert same(dev_many[:3], want) and same(dev_many[21:], want)


@pytest.mark.parametrize("over", [dict(sample_format="ulaw"), dict(input_rate=8000), dict(center=True)], ids=lambda d: list(d)[0])
def test_4_the_chain_behind_every_input_stage(mfcc_amd, wav_pcm, over):
    import torch
    cid, bands = "512_160_400", 80
    if "sample_format" in over:
        x = np.random.default_rng(5).integers(0, 256, (2, 40_000)).astype(np.uint8)
    else:
        x = np.stack([kf.signal(k, 40_000, 9 + u, wav_pcm) for u, k in enumerate(["speech", "noise"])])
    with open_fb(mfcc_amd, cid, bands, **over) as m:
        xd = torch.from_numpy(x).cuda()
        raw = m.filterbank(xd)
        nf = raw.shape[1]
        assert nf == m.num_frames(40_000) > 128
        want = chain_oracle(m, raw.reshape(2 * nf, bands), np.arange(3, dtype=np.uint64) * nf).view(2, nf, 3 * bands)
        m.set_filterbank(m.W, **CHAIN)
        assert same(m.filterbank(xd), want) and same(m.filterbank(x), want)
        rows, fo = packed(m, xd.reshape(-1), [0, 40_000, 80_000], [nf, nf])
        assert same(rows.view(2, nf, -1), want)


# ------------------------------------------------------------------------------------------------ 5

def _steady(mfcc_amd, rows_per_tile, post):
    """Channels x rows that give every workgroup of the wide kernels' grid (eight per CU, post_plan.hpp) a third tile;
    compared with calls on three of the channels alone, which have fewer tiles than workgroups"""
    import torch
    cid, bands, tiles_per_ch = "512_160_400", 128, 64
    _, hop, flen = CFGS[cid]
    groups = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    nch = -(-3 * groups // tiles_per_ch)
    nf = tiles_per_ch * rows_per_tile
    x = torch.randint(-20000, 20000, (nch, flen + hop * (nf - 1)), dtype=torch.int16, device="cuda",
                      generator=torch.Generator("cuda").manual_seed(1))
    m = mfcc_amd.MFCC(nfft=512, hop=hop, win_length=flen, nfilters=8, nceptrums=8)
    with m:
        m.set_filterbank(fr.dense_random(bands, 512), **post)                            # no empty band: no NaN to compare
        got = m.filterbank(x)
        assert got.shape[1] == nf and nch * tiles_per_ch >= 3 * groups
        for u in (0, nch // 2, nch - 1):
            assert torch.equal(m.filterbank(x[u]), got[u]), u
            assert torch.isfinite(got[u]).all()


def test_5_more_tiles_than_workgroups_wide_deltas(mfcc_amd):
    _steady(mfcc_amd, delta_tile(128, 2, 8), dict(deltas=2, delta_window=8))


def test_5_more_tiles_than_workgroups_wide_stats(mfcc_amd):
    _steady(mfcc_amd, 8192 // 128, dict(normalize="meanvar"))


# ------------------------------------------------------------------------------------------------ 6

def _post(L, **kw):
    q = L.FilterbankPost(struct_size=C.sizeof(L.FilterbankPost), normalize_min_window=1, normalize_center=1, delta_window=2)
    assert L.load().mfcc_hip_pcen_defaults(C.byref(q.pcen)) == 0
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_6_every_bad_field_is_refused_and_changes_nothing(mfcc_amd, wav_pcm):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    x = torch.from_numpy(kf.signal("speech", 400 + 160 * 59, 3, wav_pcm)).cuda()
    with open_fb(mfcc_amd, "512_160_400", 80) as m:
        m.set_filterbank(m.W, normalize="mean", deltas=1)
        before = m.filterbank(x)
        assert tuple(before.shape) == (60, 160)
        bad = [dict(struct_size=0), dict(struct_size=C.sizeof(L.FilterbankPost) - 4), dict(struct_size=C.sizeof(L.FilterbankPost) + 4),
               dict(normalize=-1), dict(normalize=3), dict(normalize_window=-1), dict(normalize_window=16385),
               dict(normalize_window=40, normalize_min_window=0), dict(normalize_window=40, normalize_min_window=41),
               dict(normalize_center=2), dict(normalize_center=-1), dict(delta_order=-1), dict(delta_order=3), dict(delta_window=0),
               dict(delta_window=9), dict(delta_order=2, delta_window=9), dict(pcen_on=2), dict(pcen_on=-1)]
        for kw in bad:
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(_post(L, **kw))) == INVALID, kw
        for i in range(4):
            q = _post(L)
            q.reserved[i] = 1
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(q)) == INVALID, i
        for field, v in (("s", 0.0), ("s", 1.5), ("alpha", -0.1), ("delta", -1.0), ("r", 0.0), ("eps", 0.0), ("s", float("nan"))):
            q = _post(L, pcen_on=1)
            setattr(q.pcen, field, v)
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(q)) == INVALID, (field, v)
            q.pcen_on = 0                                              # not looked at without pcen_on
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(q)) == 0
            m.set_filterbank(m.W, normalize="mean", deltas=1)
        q = _post(L, pcen_on=1)
        q.pcen.struct_size = 0
        assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(q)) == INVALID
        assert m.num_filterbank_columns == 160 and same(m.filterbank(x), before)
        assert lib.mfcc_hip_set_filterbank_post(m._h, None) == 0 and m.num_filterbank_columns == 80


def test_6_refusals_and_state(mfcc_amd, wav_pcm):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    cid = "512_160_400"
    x = torch.from_numpy(kf.signal("speech", 400 + 160 * 199, 3, wav_pcm)).cuda()
    with mfcc_amd.MFCC(nfft=512, hop=160, win_length=400, nfilters=8, nceptrums=8) as m:              # no matrix
        assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(_post(L, normalize=1))) == UNSUPPORTED
        assert lib.mfcc_hip_set_filterbank_post(m._h, None) == UNSUPPORTED
        assert m.num_filterbank_columns == 0
    with open_fb(mfcc_amd, cid, 80) as m:
        W = m.W
        for scale in ("ln", "log10", "energy"):                                              # PCEN reads log2 energies
            m.set_filterbank(W, scale)
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(_post(L, pcen_on=1))) == UNSUPPORTED
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(_post(L, normalize=2, delta_order=1))) == 0
            assert m.num_filterbank_columns == 160
        m.set_filterbank(W)
        raw, raw_halo = m.filterbank(x), m.filterbank(x, halo=1)
        own, spec = m.process(x), m.power_spectrum(x)
        m.set_filterbank(W, **CHAIN)
        with pytest.raises(mfcc_amd.MfccHipError) as e:                                      # a shard of a longer stream
            m.filterbank(x, halo=1)
        assert e.value.code == UNSUPPORTED
        assert same(m.process(x), own) and same(m.power_spectrum(x), spec)                   # the handle's own calls: unchanged
        with pytest.raises(mfcc_amd.MfccHipError) as e:                                      # a bank takes its settings at creation
            m.stream_bank(2, filterbank=True)
        assert e.value.code == UNSUPPORTED
        with m.stream_bank(2):                                                               # the handle's own rows: as ever
            pass
        m.set_filterbank(W)                                                                  # resets the settings
        assert m.num_filterbank_columns == 80 and same(m.filterbank(x), raw) and same(m.filterbank(x, halo=1), raw_halo)
        with m.stream_bank(2, filterbank=True) as bank:
            assert lib.mfcc_hip_set_filterbank_post(m._h, C.byref(_post(L, normalize=1))) == BUSY
            assert lib.mfcc_hip_set_filterbank_post(m._h, None) == BUSY
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.set_filterbank(W, normalize="mean")
            assert e.value.code == BUSY
            assert m.num_filterbank_columns == 80 and same(m.filterbank(x), raw)             # unchanged
            assert bank.num_features == 80
        m.set_filterbank(W, normalize="meanvar", deltas=2)                                   # the bank is gone
        assert m.num_filterbank_columns == 240
        m.set_filterbank(None)
        assert m.num_bands == 0 and m.num_filterbank_columns == 0
        m.set_filterbank(W)
        assert m.num_filterbank_columns == 80 and same(m.filterbank(x), raw)                 # None cleared them
    # the handle's own settings still do not reach a filterbank call
    busy = dict(nfilters=40, nceptrums=13, output="logmel", mel="htk", fmin=20.0, normalize="meanvar", deltas=2, pcen=True)
    with open_fb(mfcc_amd, cid, 80, **busy) as m:
        assert m.num_features == 120 and same(m.filterbank(x), raw)
        own = m.process(x)
        m.set_filterbank(m.W, deltas=1)
        assert same(m.process(x), own) and m.num_features == 120
    # the direct entries keep their width
    with open_fb(mfcc_amd, cid, 80) as m:
        rows = torch.zeros((50, 65), device="cuda")
        for call in (lambda: m.normalize_rows(rows), lambda: m.normalize_rows(rows, window=40), lambda: m.pcen_rows(rows),
                     lambda: m.deltas_rows(rows)):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == INVALID
