"""The filterbank stream bank (``MFCC.stream_bank(n, filterbank=True)`` / ``mfcc_hip_bank_create_filterbank``): live lines
whose rows are the handle's filterbank rows, up to 128 bands, with causal CMVN, deltas and PCEN of their own.

Everything here is bit for bit, and the oracle is the library's own one-shot path:

* 1  a plain bank: any pushes followed by a flush equal ``m.filterbank(whole signal)`` -- both fused shapes and the
     generic kernel, the fp32 and the MFMA form of the fused kernel, a ln matrix with a floor, both pad modes, host and
     device pushes;
* 2  the routes: 2500 lines in lockstep (more records than workgroups), a mixed push (the gather), a straggler, a result
     inside sentinel rows, a refused push;
* 3  online: the one-shot rows cut into column slices of at most 64, each slice through ``pcen_rows`` /
     ``normalize_rows(window=N, min_window=1, center=False)`` / ``deltas_rows``, put back as ``[s | D | DD]``; at 64 bands
     the whole width too, which pins the oracle without the per-column assumption;
* 4  PCEN across a tile edge, over three tiles, on a silent stream;
* 5  lifecycle and refusals;
* 6  a mu-law handle, and a resampler in front of the bank."""
import ctypes as C
import types

import numpy as np
import pytest

import fbank_ref as fr
import kernel_families as kf
import online_ref as on
from kernel_families import same

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]
FUSED, GENERIC = "mfcc_fbank512_kernel", "mfcc_fbank_generic_kernel"
CFGS = {"512_170_512": (512, 170, 512), "512_160_400": (512, 160, 400), "256_80_200": (256, 80, 200)}
KERNEL = {"512_170_512": FUSED, "512_160_400": FUSED, "256_80_200": GENERIC}
PCEN = dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6)
UNSUPPORTED, INVALID, BUSY, SMALL = -105, -101, -104, -106         # include/mfcc_hip.h


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    from mfcc_amd import _lib as L
    assert (L.ERROR_UNSUPPORTED, L.ERROR_INVALID_PARAM, L.ERROR_BUSY, L.ERROR_BUFFER_SMALL) == (UNSUPPORTED, INVALID, BUSY, SMALL)
    return mfcc_amd


def matrix(name, nfft):
    """(weights, scale, floor)"""
    if name.startswith("htk"):                                               # htkN_log2: the fp32 form
        return fr.htk_weights(int(name[3:].split("_")[0]), nfft), "log2", 0.0
    if name == "dense127_energy":                                            # the MFMA form at the fused shapes
        W = fr.dense_random(127, nfft)
        W[63] = 0.0                                                          # an empty band inside
        return W, "energy", 0.0
    assert name == "ln23_floor"
    return fr.htk_weights(23, nfft), "ln", 1e-3


def framing(cfg):
    """what online_ref's helpers read of a family: the hop and the frame length"""
    return types.SimpleNamespace(hop=cfg[1], nfft=cfg[2])


def open_fb(mfcc_amd, cid, mat, pad="notebook", **over):
    nfft, hop, flen = CFGS[cid]
    kw = dict(nfft=nfft, hop=hop, nfilters=8, nceptrums=8, pad_mode=pad)
    if nfft != 512:
        kw["power_scale"] = 0
    if flen != nfft:
        kw["win_length"] = flen
    kw.update(over)
    m = mfcc_amd.MFCC(**kw)
    try:
        if mat is not None:
            W, scale, floor = matrix(mat, nfft)
            m.set_filterbank(W, scale, floor)
            if "impl" not in over:
                assert m.filterbank_kernel_name() == KERNEL[cid]
                if mat == "dense127_energy":
                    assert fr.form_of(W, KERNEL[cid]) == ("bf16" if KERNEL[cid] == FUSED else "f32")
                else:
                    assert fr.form_of(W, KERNEL[cid]) == "f32"
    except BaseException:
        m.close()
        raise
    return m


def streams(fam, pad, wav_pcm, frames=(33, 21, 40, 27, 36), kinds=("speech", "silences", "const_min", "noise", "uniform")):
    return [kf.signal(k, on.length(fam, n, pad), 3 + u, wav_pcm) for u, (k, n) in enumerate(zip(kinds, frames))]


def rows_of(got, tails, like):
    return [on.cat(got[u] + [tails[u]], like[u]) for u in range(len(like))]


# ------------------------------------------------------------------------------------------------ 1

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mat", ["htk80_log2", "dense127_energy", "ln23_floor"])
@pytest.mark.parametrize("cid", list(CFGS))
def test_1_plain_bank_equals_the_one_shot_filterbank(mfcc_amd, wav_pcm, cid, mat, pad):
    fam = framing(CFGS[cid])
    xs = streams(fam, pad, wav_pcm)
    rounds = on.schedule([len(x) for x in xs], seed=CFGS[cid][0] + CFGS[cid][1], choices=on.sizes(fam))
    with open_fb(mfcc_amd, cid, mat, pad) as m:
        one = [m.filterbank(x) for x in xs]
        assert [len(o) for o in one] == [33, 21, 40, 27, 36] and one[0].shape[1] == m.num_bands
        with m.stream_bank(len(xs), filterbank=True) as bank:
            assert bank.filterbank and not bank.online and bank.lag == 0 and bank.num_features == m.num_bands
            for name, push in (("host", on.push_host), ("device", on.push_dev)):
                got = push(bank, xs, rounds)
                tails = bank.flush()
                assert [len(t) for t in tails] == [int(pad == "stream")] * len(xs)
                assert not bank.pending.any()
                for u, r in enumerate(rows_of(got, tails, one)):
                    assert same(r, one[u]), (cid, mat, pad, name, u)
        if mat == "dense127_energy":
            assert all((o[:, 63] == 0).all() and not np.signbit(o[:, 63]).any() for o in one)      # the empty band: +0.0


# ------------------------------------------------------------------------------------------------ 2

def test_2_lockstep_lines_beyond_the_grid(mfcc_amd):
    import torch
    n, (nfft, hop, flen) = 2500, CFGS["512_160_400"]
    x = torch.from_numpy(np.random.default_rng(1).integers(-20000, 20000, (n, flen + 3 * hop)).astype(np.int16)).cuda()
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2") as m:
        one = m.filterbank(x)                                                # (n, 4, 80)
        assert tuple(one.shape) == (n, 4, 80)
        with m.stream_bank(n, filterbank=True) as bank:
            a = 0
            for k, c in enumerate([flen, hop, hop, hop]):
                flat = x[:, a:a + c].contiguous().reshape(-1)
                out, fo = bank.push_packed(flat, np.arange(n + 1, dtype=np.uint64) * c)
                assert np.array_equal(fo, np.arange(n + 1))
                assert same(out.view(n, 80), one[:, k]), k
                a += c
            assert np.array_equal(bank.pending, [flen - hop] * n)


@pytest.mark.parametrize("cfg", ["plain", "meanvar40_dd2"])
def test_2_mixed_push_straggler_and_sentinels(mfcc_amd, wav_pcm, cfg):
    import torch
    cid = "512_160_400"
    fam = framing(CFGS[cid])
    hop, flen = fam.hop, fam.nfft
    cfg = {} if cfg == "plain" else on.MEANVAR40_DD2
    lag = on.lag_of(cfg)
    # one push: stream 0 completes no frame, stream 1 forty, the others one; then stream 2 alone; then the rest of all
    first = [flen - 1, flen + 39 * hop, flen, flen + 7, flen + hop - 1]
    xs = [kf.signal(k, n + 9 * hop + 13 * u, 20 + u, wav_pcm) for u, (k, n) in
          enumerate(zip(["noise", "speech", "silences", "uniform", "const_min"], first))]
    with open_fb(mfcc_amd, cid, "htk80_log2") as m:
        one = [_online_oracle(m, m.filterbank(x), cfg) for x in xs]
        with m.stream_bank(5, filterbank=True, **cfg) as bank:
            W = bank.num_features
            assert W == 80 * (1 + cfg.get("deltas", 0))
            got = [[] for _ in xs]

            def push(chunks):
                """through push_packed into a view inside sentinel rows"""
                lens = [len(c) for c in chunks]
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
                flat = torch.from_numpy(np.concatenate(chunks + [np.zeros(4, np.int16)])).cuda()[:int(off[-1])]
                nf = int(bank.num_frames(lens)[-1])
                big = torch.full((nf + 5, W), 12345.0, device="cuda")
                out, fo = bank.push_packed(flat, off, out=big[2:2 + nf])
                torch.cuda.synchronize()
                assert int(fo[-1]) == nf and (big[:2] == 12345.0).all() and (big[2 + nf:] == 12345.0).all()
                o = out.cpu().numpy()
                for u in range(len(xs)):
                    got[u].append(o[int(fo[u]):int(fo[u + 1])])
                return [int(fo[u + 1] - fo[u]) for u in range(len(xs))]

            model = on.Model(fam, 5, lag)
            chunks = [x[:k] for x, k in zip(xs, first)]
            assert push(chunks) == model.push(first) == [max(0, f - lag) for f in (0, 40, 1, 1, 1)]
            pos = list(first)
            alone = [0, 0, 5 * hop, 0, 0]                                    # the straggler: five frames of stream 2 alone
            assert push([x[p:p + k] for x, p, k in zip(xs, pos, alone)]) == model.push(alone) == [0, 0, 5 - lag + min(lag, 1), 0, 0]
            pos[2] += 5 * hop
            push([x[p:] for x, p in zip(xs, pos)])
            assert list(bank.held) == [lag] * 5
            tails = bank.flush()
            for u, r in enumerate(rows_of(got, tails, one)):
                assert same(r, one[u]), u


def test_2_refused_push_consumes_nothing(mfcc_amd, wav_pcm):
    lib = mfcc_amd.load_library()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731
    xs = [np.ascontiguousarray(wav_pcm[3000 * u:3000 * u + 4000]) for u in range(3)]
    with open_fb(mfcc_amd, "512_170_512", "htk80_log2") as m, m.stream_bank(3, filterbank=True) as bank:
        one = [m.filterbank(x) for x in xs]
        first = bank.push([x[:1400] for x in xs])                            # 6 frames each
        flat = np.concatenate([x[1400:] for x in xs])
        offsets = (np.arange(4) * 2600).astype(np.uint64)
        out = np.empty((44, 80), np.float32)                                 # 45 rows are due: 15 per stream
        fo = np.full(4, 77, np.uint64)
        assert lib.mfcc_hip_bank_push(bank._b, ptr(flat), ptr(offsets), ptr(out), out.size, ptr(fo)) == SMALL
        assert list(fo) == [0, 15, 30, 45]
        assert list(bank.pending) == [1400 - 6 * 170] * 3
        rows = bank.push([x[1400:] for x in xs])
        tails = bank.flush()
        for u in range(3):
            assert same(on.cat([first[u], rows[u], tails[u]], one[u]), one[u]), u


# ------------------------------------------------------------------------------------------------ 3

def _online_oracle(m, rows, cfg, pcen=None, width=64):
    """The one-shot rows (frames, W) cut into column slices of at most ``width``, each slice through the direct entries,
    put back as [s | D | DD] of the full width."""
    import torch
    order = cfg.get("deltas", 0)
    W = rows.shape[1]
    if not len(rows):
        return np.zeros((0, W * (1 + order)), np.float32)
    parts = [[] for _ in range(1 + order)]
    for a in range(0, W, width):
        s = torch.from_numpy(np.ascontiguousarray(rows[:, a:a + width])).cuda()
        w = int(s.shape[1])
        if pcen:
            m.pcen_rows(s, **pcen)
        if cfg.get("normalize"):
            s = m.normalize_rows(s, mode=cfg["normalize"], window=cfg["normalize_window"], min_window=1, center=False)
        if order:
            e = m.deltas_rows(s, order=order, window=cfg["delta_window"])
            for k in range(1 + order):
                parts[k].append(e[:, k * w:(k + 1) * w])
        else:
            parts[0].append(s)
    return torch.cat([torch.cat(p, dim=1) for p in parts], dim=1).cpu().numpy()


MEANVAR40 = dict(normalize="meanvar", normalize_window=40)
ONLINE = {
    # id: (shape, bands, the bank's settings)
    "64_meanvar40_dd2": ("512_160_400", 64, on.MEANVAR40_DD2),
    "65_d1x8": ("512_160_400", 65, on.RAW_D8),
    "80_meanvar40_dd2": ("512_160_400", 80, on.MEANVAR40_DD2),
    "80_meanvar40": ("512_170_512", 80, MEANVAR40),
    "128_meanvar40_dd2x8": ("512_160_400", 128, dict(MEANVAR40, deltas=2, delta_window=8)),
    "128_dd2x8": ("256_80_200", 128, dict(deltas=2, delta_window=8)),
    "128_mean600": ("512_170_512", 128, dict(normalize="mean", normalize_window=600)),
    "65_meanvar40_d1x8": ("256_80_200", 65, dict(MEANVAR40, deltas=1, delta_window=8)),
}


@pytest.mark.parametrize("oid", list(ONLINE))
def test_3_online_bank_equals_the_direct_entries_by_columns(mfcc_amd, wav_pcm, oid):
    cid, bands, cfg = ONLINE[oid]
    fam = framing(CFGS[cid])
    pad = "stream" if bands in (65, 128) else "notebook"
    lag = on.lag_of(cfg)
    xs = streams(fam, pad, wav_pcm, frames=(150, 3, 143, 1, 156, 0), kinds=("speech", "noise", "silences", "uniform", "noise", "noise"))
    choices = on.sizes(fam) * 3 + [40 * fam.hop + 1, 23 * fam.hop]
    rounds = on.schedule([len(x) for x in xs], seed=bands + lag, choices=choices)
    with open_fb(mfcc_amd, cid, "htk%d_log2" % bands, pad) as m:
        raw = [m.filterbank(x) for x in xs]
        one = [_online_oracle(m, r, cfg) for r in raw]
        if bands == 64:                                                      # the whole width: no per-column assumption
            whole = [_online_oracle(m, r, cfg, width=64) for r in raw]
            halves = [_online_oracle(m, r, cfg, width=32) for r in raw]
            assert all(same(a, b) for a, b in zip(whole, halves))
        with m.stream_bank(len(xs), filterbank=True, **cfg) as bank:
            assert bank.online and bank.lag == lag and bank.num_features == bands * (1 + cfg.get("deltas", 0))
            model = on.Model(fam, len(xs), lag)
            for name, push in (("host", on.push_host), ("device", on.push_dev)):
                got = push(bank, xs, rounds)
                for cut in rounds:
                    model.push([b - a for a, b in cut])
                assert list(bank.held) == model.held
                tails = bank.flush()
                model.held = [0] * len(xs)
                model.queued = [0] * len(xs)
                assert not bank.pending.any() and not bank.held.any()
                for u, r in enumerate(rows_of(got, tails, one)):
                    assert same(r, one[u]), (oid, name, u)


def test_3_flush_and_reset_of_subsets(mfcc_amd, wav_pcm):
    cid, cfg = "512_160_400", dict(MEANVAR40, deltas=2, delta_window=8)
    fam = framing(CFGS[cid])
    hop, flen = fam.hop, fam.nfft
    xs = [kf.signal("noise", on.length(fam, 120, "stream"), 50 + u, wav_pcm) for u in range(4)]
    ys = [kf.signal("uniform", on.length(fam, 90, "stream"), 60 + u, wav_pcm) for u in range(4)]
    first = [flen + 70 * hop, flen + 30 * hop + 7, flen + 2 * hop, flen + hop]
    empty = xs[0][:0]
    with open_fb(mfcc_amd, cid, "htk128_log2", "stream") as m:
        orc = lambda x: _online_oracle(m, m.filterbank(x), cfg)              # noqa: E731
        one_x, one_y = [orc(x) for x in xs], [orc(y) for y in ys]
        one_part = [orc(xs[1][:first[1]]), orc(xs[3][:first[3]])]
        with m.stream_bank(4, filterbank=True, **cfg) as bank:
            assert bank.lag == 16 and bank.num_features == 384
            a = bank.push([x[:k] for x, k in zip(xs, first)])
            assert list(bank.held) == [16, 16, 3, 2]
            t = bank.flush([3, 1])                                           # in the order listed
            assert same(on.cat([a[3], t[0]], t[0]), one_part[1]) and same(on.cat([a[1], t[1]], t[1]), one_part[0])
            bank.push([empty, empty, xs[2][first[2]:first[2] + 50 * hop], empty])
            bank.reset([2])                                                  # ... while 0 goes on
            assert list(bank.held) == [16, 0, 0, 0] and bank.pending[2] == 0
            b = bank.push([xs[0][first[0]:], ys[1], ys[2], ys[3]])
            t = bank.flush()
            assert same(on.cat([a[0], b[0], t[0]], a[0]), one_x[0])
            for u in (1, 2, 3):
                assert same(on.cat([b[u], t[u]], b[u]), one_y[u]), u


# ------------------------------------------------------------------------------------------------ 4

@pytest.mark.parametrize("cfg", ["pcen", "pcen_meanvar40_dd2"])
def test_4_pcen_tile_edges_and_silence(mfcc_amd, wav_pcm, cfg):
    cid = "512_160_400"
    fam = framing(CFGS[cid])
    hop, flen = fam.hop, fam.nfft
    cfg = {} if cfg == "pcen" else on.MEANVAR40_DD2
    x = kf.silent_stream(fam, 430, 31)
    silent = np.zeros(on.length(fam, 140, "stream"), np.int16)
    # stream 0: 124 frames, then one frame per push across frames 127 -> 128 -> 129, then the rest; stream 1: 100 frames,
    # then a chunk that spans three tiles (frames 100 .. 419), then the rest; stream 2: silence; stream 3: all at once
    cuts0 = [flen + 123 * hop] + [hop] * 10
    cuts1 = [flen + 99 * hop, 320 * hop]
    with open_fb(mfcc_amd, cid, "htk80_log2", "stream") as m:
        one = _online_oracle(m, m.filterbank(x), cfg, pcen=PCEN)
        one_silent = _online_oracle(m, m.filterbank(silent), cfg, pcen=PCEN)
        with m.stream_bank(4, filterbank=True, pcen=PCEN, **cfg) as bank:
            assert bank.online and bank.lag == on.lag_of(cfg)
            got, pos = [[], [], [], []], [0, 0, 0, 0]
            for k in range(12):
                take = [cuts0[k] if k < len(cuts0) else len(x) - pos[0], cuts1[k] if k < len(cuts1) else len(x) - pos[1],
                        len(silent) if k == 3 else 0, len(x) if k == 0 else 0]
                chunks = [s[p:p + t] for s, p, t in zip([x, x, silent, x], pos, take)]
                pos = [p + len(c) for p, c in zip(pos, chunks)]
                for u, r in enumerate(bank.push(chunks)):
                    got[u].append(r)
                if 1 <= k <= 10:
                    assert len(got[0][-1]) == 1
            assert pos == [len(x), len(x), len(silent), len(x)]
            tails = bank.flush()
            for u, want in enumerate([one, one, one_silent, one]):
                assert same(on.cat(got[u] + [tails[u]], want), want), u


@pytest.mark.parametrize("mat", ["dense127_energy", "ln23_floor"])
def test_4_pcen_wants_a_log2_matrix(mfcc_amd, mat):
    with open_fb(mfcc_amd, "512_160_400", mat) as m:
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.stream_bank(2, filterbank=True, pcen=PCEN)
        assert e.value.code == UNSUPPORTED
        with m.stream_bank(2, filterbank=True, normalize="mean", normalize_window=5) as bank:        # ... without it: fine
            assert bank.num_features == m.num_bands


# ------------------------------------------------------------------------------------------------ 5

def test_5_refusals(mfcc_amd):
    from mfcc_amd import _lib as L
    lib = mfcc_amd.load_library()
    with open_fb(mfcc_amd, "512_160_400", None) as m:                        # no matrix
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.stream_bank(2, filterbank=True)
        assert e.value.code == UNSUPPORTED
        with m.stream_bank(2):                                               # the handle's own rows: as ever
            pass
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2", input_rate=8000) as m:
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.stream_bank(2, filterbank=True)
        assert e.value.code == UNSUPPORTED
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2") as m:
        ok = L.Pcen()
        assert lib.mfcc_hip_pcen_defaults(C.byref(ok)) == 0
        bad = L.Pcen.from_buffer_copy(ok)
        bad.s = 0.0
        b = C.c_void_p()
        create = lambda *a: lib.mfcc_hip_bank_create_filterbank(m._h, *a, C.byref(b))          # noqa: E731
        assert create(2, C.byref(bad), 0, 0, 0, 2) == INVALID
        assert create(0, None, 0, 0, 0, 2) == INVALID
        assert create(2, None, 3, 5, 0, 2) == INVALID and create(2, None, -1, 5, 0, 2) == INVALID
        assert create(2, None, 1, 0, 0, 2) == INVALID and create(2, None, 2, L.MAX_NORMALIZE_WINDOW + 1, 0, 2) == INVALID
        assert create(2, None, 0, 0, 3, 2) == INVALID and create(2, None, 0, 0, -1, 2) == INVALID
        assert create(2, None, 0, 0, 1, 0) == INVALID and create(2, None, 0, 0, 2, 9) == INVALID
        assert not b.value
        assert create(2, None, 0, 0, 0, 1) == 0 and b.value                  # NONE ignores the window: a plain bank
        assert lib.mfcc_hip_bank_row_width(b) == 80 and lib.mfcc_hip_bank_lag(b) == 0 and lib.mfcc_hip_bank_size(b) == 2
        lib.mfcc_hip_bank_destroy(b)
        with pytest.raises(ValueError):
            m.stream_bank(2, fixed=True, filterbank=True)


def test_5_the_matrix_is_the_banks_while_it_lives(mfcc_amd, wav_pcm):
    x = kf.signal("speech", 6000, 1, wav_pcm)
    W2 = fr.htk_weights(40, 512)
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2") as m:
        before = m.filterbank(x)
        with m.stream_bank(2) as mfcc_bank:                                  # only an MFCC bank alive: set_filterbank works
            m.set_filterbank(W2, "ln", 0.5)
            assert m.num_bands == 40
            m.set_filterbank(*matrix("htk80_log2", 512))
            assert same(m.filterbank(x), before)
            with m.stream_bank(2, filterbank=True) as bank:
                for args in ((W2, "ln", 0.5), (None,)):
                    with pytest.raises(mfcc_amd.MfccHipError) as e:
                        m.set_filterbank(*args)
                    assert e.value.code == BUSY
                assert m.num_bands == 80 and same(m.filterbank(x), before)   # the matrix is untouched
                rows = bank.push([x, x[:0]])[0]
                assert same(rows, before)
                with pytest.raises(mfcc_amd.MfccHipError) as e:
                    m.set_normalize("mean")                                  # it counts as a session like any bank
                assert e.value.code == BUSY
            assert len(mfcc_bank.push([x, x])[0]) == len(before)
            m.set_filterbank(W2, "ln", 0.5)                                  # the bank is gone
            assert m.num_bands == 40


def test_5_either_destroy_order_and_the_handles_own_settings(mfcc_amd, wav_pcm):
    x = kf.signal("noise", 8000, 2, wav_pcm)
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2", "stream") as m:
        one = m.filterbank(x)
    # a handle with post settings of its own: an MFCC bank is refused, a filterbank bank gives the filterbank rows
    m = open_fb(mfcc_amd, "512_160_400", "htk80_log2", "stream", normalize="meanvar", deltas=2, output="logmel")
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        m.stream_bank(2)
    assert e.value.code == UNSUPPORTED
    bank = m.stream_bank(2, filterbank=True)
    other = m.stream_bank(1, filterbank=True, deltas=1)
    a = bank.push([x[:3000], x[:100]])
    m.close()                                                                # the handle first
    b = bank.push([x[3000:], x[:0]])
    t = bank.flush([0])
    assert same(on.cat([a[0], b[0], t[0]], one), one)
    bank.close()
    other.close()                                                            # the last one frees the handle
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2") as m2:               # ... and the bank first
        bank = m2.stream_bank(2, filterbank=True)
        bank.close()
        m2.set_filterbank(None)


# ------------------------------------------------------------------------------------------------ 6

def test_6_mulaw_handle(mfcc_amd):
    fam = framing(CFGS["512_160_400"])
    rng = np.random.default_rng(8)
    raw = [rng.integers(0, 256, on.length(fam, n, "stream"), dtype=np.uint8) for n in (30, 17, 1)]
    rounds = on.schedule([len(x) for x in raw], seed=4, choices=on.sizes(fam))
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2", "stream") as m16:
        one = [m16.filterbank(mfcc_amd.decode(x, "ulaw")) for x in raw]
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2", "stream", sample_format="ulaw") as m, \
            m.stream_bank(3, filterbank=True) as bank:
        got = on.push_host(bank, raw, rounds)
        tails = bank.flush()
        for u, r in enumerate(rows_of(got, tails, one)):
            assert same(r, one[u]), u


def test_6_resampler_in_front_of_the_bank(mfcc_amd):
    import torch
    lines, total = 4, 12000
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (lines, total), dtype=np.uint8)
    cfg = dict(MEANVAR40, deltas=1, delta_window=2)
    with open_fb(mfcc_amd, "512_160_400", "htk80_log2") as m:
        whole = [mfcc_amd.resample(mfcc_amd.decode(raw[u], "ulaw"), 8000, 16000) for u in range(lines)]
        one = [m.filterbank(w) for w in whole]
        one_online = [_online_oracle(m, o, cfg) for o in one]
        with m.resampler(lines, 8000, "ulaw") as rs, m.stream_bank(lines, filterbank=True) as bank, \
                m.stream_bank(lines, filterbank=True, **cfg) as online:
            rows, rows_online = [[] for _ in range(lines)], [[] for _ in range(lines)]

            def take(out, oo):                                               # composed on the device
                for dst, bk in ((rows, bank), (rows_online, online)):
                    r, fo = bk.push_packed(out, oo)
                    for u in range(lines):
                        dst[u].append(r[int(fo[u]):int(fo[u + 1])])

            pos = 0
            for n in (1000, 37, 2963, 4000, 4000):
                flat = torch.from_numpy(np.ascontiguousarray(raw[:, pos:pos + n]).reshape(-1)).cuda()
                take(*rs.push_packed(flat, np.arange(lines + 1, dtype=np.uint64) * n))
                pos += n
            assert pos == total
            take(*rs.flush_packed())
            torch.cuda.synchronize()
            tails = online.flush()
            assert [len(t) for t in bank.flush()] == [0] * lines             # the notebook framing: no tail row
            for u in range(lines):
                assert same(torch.cat(rows[u]), one[u]), u
                assert same(np.concatenate([torch.cat(rows_online[u]).cpu().numpy(), tails[u]]), one_online[u]), u
