"""PCEN as state of the online stream bank (``MFCC.stream_bank(n, pcen=...)`` / ``mfcc_hip_bank_create_online_pcen``).

Any pushes followed by a flush give every stream, bit for bit, the rows of the one-shot call on its whole signal by a
handle with the same PCEN parameters, the purely causal window (min_window 1) and the same deltas:

* B1  seeded schedules through ``push`` and ``push_packed``, both framings, PCEN alone and with meanvar 40 + delta-delta;
* B2  one frame per push across the frames 127 -> 128 -> 129 of a tile edge, a chunk that spans three tiles;
* B3  flush / reset of subsets and stragglers, a reset in the middle of a tile;
* B4  a small buffer and a refused push consume nothing;
* B5  a plain bank and an online bank without PCEN next to it are unchanged; p = NULL is the online bank.

Streams of 0, 1 and 3 frames, one silent from its first frame (C_0 = 0), one with silent stretches; 300 and 420 frames
cross two and three tile edges at chunk positions the schedules draw."""
import ctypes as C

import numpy as np
import pytest

import kernel_families as kf
import online_ref as on
import pcen_ref as pr
from kernel_families import open_handle, same

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]
PCEN = dict(s=0.04, alpha=0.8, delta=10.0, r=0.25, eps=1e-6)
CFGS = {"pcen": {}, "pcen_meanvar40_dd2": on.MEANVAR40_DD2}
LOGMEL = dict(output="logmel")


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _streams(fam, pad, wav_pcm):
    silent_start = kf.signal("noise", on.length(fam, 140, pad), 5, wav_pcm)
    silent_start[:fam.nfft + 2 * fam.hop] = 0                            # frames 0..2 silent: C_0 = 0 in every band
    return [kf.signal("speech", on.length(fam, 300, pad), 3, wav_pcm),
            silent_start,
            kf.signal("noise", on.length(fam, 1, pad), 6, wav_pcm),
            kf.signal("uniform", on.length(fam, 3, pad), 7, wav_pcm),
            np.zeros(0, np.int16),
            kf.silent_stream(fam, 420, 8)]


def _one_shot(mfcc_amd, fam, pad, cfg, xs, pcen=PCEN):
    with open_handle(mfcc_amd, fam, pad, **LOGMEL, pcen=pcen, **on.one_shot_kwargs(cfg)) as m1:
        return [m1.process(x) for x in xs]


# ------------------------------------------------------------------------------------------------ B1

@pytest.mark.parametrize("cfg", list(CFGS), ids=list(CFGS))
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fid", ["f512", "g256"])
def test_b1_any_schedule_equals_the_one_shot_call(mfcc_amd, wav_pcm, fid, pad, cfg):
    fam = on.BY_ID[fid]
    cfg = CFGS[cfg]
    xs = _streams(fam, pad, wav_pcm)
    choices = on.sizes(fam) * 4 + [40 * fam.hop + 1, 127 * fam.hop, 129 * fam.hop + 3, 260 * fam.hop + fam.nfft]
    rounds = on.schedule([len(x) for x in xs], seed=fam.nfft + fam.hop, choices=choices)
    one = _one_shot(mfcc_amd, fam, pad, cfg, xs)
    assert len(one[0]) == 300 and len(one[5]) in (420, 421) and all(np.isfinite(o[:, :fam.nfilters]).all() for o in one if len(o))
    with open_handle(mfcc_amd, fam, pad, **LOGMEL) as m, m.stream_bank(len(xs), pcen=PCEN, **cfg) as bank:
        assert bank.lag == on.lag_of(cfg) and bank.num_features == one[0].shape[1] and bank.online
        assert bank.pcen == {k: pr.f32(v) for k, v in PCEN.items()}
        for name, push in (("host", on.push_host), ("device", on.push_dev)):
            got = push(bank, xs, rounds)
            tails = bank.flush()
            assert not bank.pending.any() and not bank.held.any()
            for u in range(len(xs)):
                assert same(on.cat(got[u] + [tails[u]], one[u]), one[u]), (fid, pad, name, u)


def test_b1_rows_meet_the_definition(mfcc_amd, wav_pcm):
    """Without the one-shot PCEN kernels: the bank's rows against the float64 definition on the raw rows."""
    fam = on.BY_ID["f512"]
    xs = _streams(fam, "stream", wav_pcm)
    rounds = on.schedule([len(x) for x in xs], seed=5, choices=on.sizes(fam))
    ps = tuple(PCEN[k] for k in ("s", "alpha", "delta", "r", "eps"))
    with open_handle(mfcc_amd, fam, "stream", **LOGMEL) as m, m.stream_bank(len(xs), pcen=PCEN) as bank:
        raw = [m.process(x) for x in xs]
        got = on.push_host(bank, xs, rounds)
        tails = bank.flush()
        for u, r in enumerate(raw):
            rows = on.cat(got[u] + [tails[u]], r)
            assert rows.shape == r.shape
            if len(r):
                pr.check(rows, pr.pcen_f64(r, None, *ps), ps[2], ps[3], what="stream %d" % u)


# ------------------------------------------------------------------------------------------------ B2

@pytest.mark.parametrize("cfg", list(CFGS), ids=list(CFGS))
def test_b2_tile_edges(mfcc_amd, wav_pcm, cfg):
    fam = on.BY_ID["f512"]
    cfg = CFGS[cfg]
    hop, nfft = fam.hop, fam.nfft
    x = kf.silent_stream(fam, 500, 31)
    one = _one_shot(mfcc_amd, fam, "stream", cfg, [x])[0]
    # stream 0: 124 frames, then one frame per push up to frame 133, then the rest; stream 1: 100 frames, then a chunk
    # that spans three tiles (frames 100..419), then the rest; stream 2: everything at once
    cuts0 = [nfft + 123 * hop] + [hop] * 10
    cuts1 = [nfft + 99 * hop, 320 * hop]
    with open_handle(mfcc_amd, fam, "stream", **LOGMEL) as m, m.stream_bank(3, pcen=PCEN, **cfg) as bank:
        got = [[], [], []]
        pos = [0, 0, 0]
        for k in range(12):
            take = [cuts0[k] if k < len(cuts0) else len(x) - pos[0], cuts1[k] if k < len(cuts1) else len(x) - pos[1],
                    len(x) if k == 0 else 0]
            chunks = [x[p:p + t] for p, t in zip(pos, take)]
            pos = [p + len(c) for p, c in zip(pos, chunks)]
            for u, r in enumerate(bank.push(chunks)):
                got[u].append(r)
            if 1 <= k <= 10:
                assert len(got[0][-1]) == 1
        assert pos == [len(x)] * 3
        tails = bank.flush()
        for u in range(3):
            assert same(on.cat(got[u] + [tails[u]], one), one), u


# ------------------------------------------------------------------------------------------------ B3

@pytest.mark.parametrize("pad", PADS)
def test_b3_flush_and_reset_of_subsets(mfcc_amd, wav_pcm, pad):
    fam = on.BY_ID["f512"]
    cfg = on.MEANVAR40_DD2
    hop, nfft = fam.hop, fam.nfft
    xs = [kf.signal("noise", on.length(fam, 200, pad), 50 + u, wav_pcm) for u in range(4)]
    ys = [kf.signal("uniform", on.length(fam, 140, pad), 60 + u, wav_pcm) for u in range(4)]
    one_x, one_y = _one_shot(mfcc_amd, fam, pad, cfg, xs), _one_shot(mfcc_amd, fam, pad, cfg, ys)
    first = [nfft + 129 * hop, nfft + 30 * hop + 7, nfft + 2 * hop, nfft + hop]
    one_part = _one_shot(mfcc_amd, fam, pad, cfg, [xs[1][:first[1]], xs[3][:first[3]]])
    empty = xs[0][:0]
    with open_handle(mfcc_amd, fam, pad, **LOGMEL) as m, m.stream_bank(4, pcen=PCEN, **cfg) as bank:
        a = bank.push([x[:k] for x, k in zip(xs, first)])
        # streams 3 and 1 end here (in the order listed); 0 and 2 carry on, 1 and 3 start new signals
        t = bank.flush([3, 1])
        assert same(on.cat([a[3], t[0]], t[0]), one_part[1]) and same(on.cat([a[1], t[1]], t[1]), one_part[0])
        b = bank.push([xs[0][first[0]:], ys[1], xs[2][first[2]:], ys[3]])
        t = bank.flush()
        assert same(on.cat([a[0], b[0], t[0]], a[0]), one_x[0])
        assert same(on.cat([a[2], b[2], t[2]], a[2]), one_x[2])
        assert same(on.cat([b[1], t[1]], b[1]), one_y[1])
        assert same(on.cat([b[3], t[3]], b[3]), one_y[3])
        # a reset in the middle of a tile: the carry, the local smoother and the frame count go
        bank.push([empty, empty, xs[2][:nfft + 150 * hop], xs[3][:100]])
        bank.reset([2])
        assert bank.held[2] == 0 and bank.pending[2] == 0 and bank.pending[3] == 100
        c = bank.push([empty, empty, ys[2], empty])
        t = bank.flush([2])
        assert same(on.cat([c[2], t[0]], c[2]), one_y[2])
        bank.reset()
        # a straggler: stream 0 gets samples in every push, stream 1 only now and then
        got, p1 = [[], []], 0
        for k, a0 in enumerate(range(0, len(xs[0]), 4000)):
            late = xs[1][p1:p1 + 12000] if k % 3 == 2 else empty
            p1 += len(late)
            for u, r in enumerate(bank.push([xs[0][a0:a0 + 4000], late, empty, empty])[:2]):
                got[u].append(r)
        got[1].append(bank.push([empty, xs[1][p1:], empty, empty])[1])
        t = bank.flush([0, 1])
        assert same(on.cat(got[0] + [t[0]], one_x[0]), one_x[0]) and same(on.cat(got[1] + [t[1]], one_x[1]), one_x[1])


# ------------------------------------------------------------------------------------------------ B4

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("cfg", list(CFGS), ids=list(CFGS))
def test_b4_small_buffer_and_refused_push_consume_nothing(mfcc_amd, wav_pcm, cfg):
    lib = mfcc_amd.load_library()
    fam = on.BY_ID["f512"]
    cfg = CFGS[cfg]
    lag = on.lag_of(cfg)
    xs = [np.ascontiguousarray(wav_pcm[3000 * u:3000 * u + 4000]) for u in range(3)]
    one = _one_shot(mfcc_amd, fam, "notebook", cfg, xs)
    with open_handle(mfcc_amd, fam, **LOGMEL) as m, m.stream_bank(3, pcen=PCEN, **cfg) as bank:
        first = bank.push([x[:1400] for x in xs])                                # 6 frames each
        assert [len(r) for r in first] == [6 - lag] * 3 and list(bank.held) == [lag] * 3
        flat = np.concatenate([x[1400:] for x in xs])
        offsets = (np.arange(4) * 2600).astype(np.uint64)
        W = bank.num_features
        out = np.empty((44, W), np.float32)                                      # 45 rows are due: 15 per stream
        fo = np.full(4, 77, np.uint64)
        assert lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(offsets), _ptr(out), out.size, _ptr(fo)) == -106
        assert list(fo) == [0, 15, 30, 45]
        bad = offsets.copy()
        bad[2] = bad[1] - 1                                                      # decreasing offsets: refused
        assert lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(bad), _ptr(out), out.size, _ptr(fo)) == -101
        assert list(bank.held) == [lag] * 3 and list(bank.pending) == [1400 - 6 * fam.hop] * 3
        rows = bank.push([x[1400:] for x in xs])                                 # the same push, with room
        tails = bank.flush()
        for u in range(3):
            assert same(on.cat([first[u], rows[u], tails[u]], one[u]), one[u]), u


# ------------------------------------------------------------------------------------------------ B5

@pytest.mark.parametrize("pad", PADS)
def test_b5_other_banks_next_to_a_pcen_bank(mfcc_amd, wav_pcm, pad):
    lib = mfcc_amd.load_library()
    fam = on.BY_ID["f512"]
    xs = [kf.signal(k, on.length(fam, 150 + 3 * u, pad), 11 + u, wav_pcm) for u, k in enumerate(["speech", "noise"])]
    rounds = on.schedule([len(x) for x in xs], seed=3, choices=on.sizes(fam) + [131 * fam.hop])
    one_pcen = _one_shot(mfcc_amd, fam, pad, {}, xs)
    with open_handle(mfcc_amd, fam, pad, **LOGMEL, **on.one_shot_kwargs(on.MEAN5)) as m1:
        one_mean = [m1.process(x) for x in xs]
    with open_handle(mfcc_amd, fam, pad, **LOGMEL) as m:
        one = [m.process(x) for x in xs]
        b = C.c_void_p()
        # p = NULL is mfcc_hip_bank_create_online
        assert lib.mfcc_hip_bank_create_online_pcen(m._h, 2, None, 1, 5, 0, 2, C.byref(b)) == 0 and b.value
        with m.stream_bank(2) as plain, m.stream_bank(2, pcen=PCEN) as pcen, m.stream_bank(2, **on.MEAN5) as mean:
            assert plain.pcen is None and not plain.online and pcen.online and pcen.lag == 0
            got_p, got_n, got_m, got_c = [[], []], [[], []], [[], []], [[], []]
            fo = np.zeros(3, np.uint64)
            for cut in rounds:                                         # the four banks take turns on one handle
                chunks = [x[a:b_] for x, (a, b_) in zip(xs, cut)]
                for got, bank in ((got_p, plain), (got_n, pcen), (got_m, mean)):
                    for u, r in enumerate(bank.push(chunks)):
                        got[u].append(r)
                flat = np.concatenate(chunks)
                offs = np.array([0, len(chunks[0]), len(flat)], np.uint64)
                out = np.empty((len(flat) // fam.hop + 2, 32), np.float32)
                assert lib.mfcc_hip_bank_push(b, _ptr(flat), _ptr(offs), _ptr(out), out.size, _ptr(fo)) == 0
                for u in range(2):
                    got_c[u].append(out[int(fo[u]):int(fo[u + 1])].copy())
            nf = C.c_size_t(0)
            out = np.empty((2, 32), np.float32)
            assert lib.mfcc_hip_bank_flush(b, None, 0, _ptr(out), out.size, C.byref(nf)) == 0
            tp, tn, tm = plain.flush(), pcen.flush(), mean.flush()
            for u in range(2):
                assert same(on.cat(got_p[u] + [tp[u]], one[u]), one[u]), u
                assert same(on.cat(got_n[u] + [tn[u]], one_pcen[u]), one_pcen[u]), u
                assert same(on.cat(got_m[u] + [tm[u]], one_mean[u]), one_mean[u]), u
                assert same(on.cat(got_c[u] + [out[u:u + 1][:nf.value // 2]], one_mean[u]), one_mean[u]), u
        lib.mfcc_hip_bank_destroy(b)
        # refusals of the new entry
        from mfcc_amd import _lib as L
        ok = L.Pcen()
        assert lib.mfcc_hip_pcen_defaults(C.byref(ok)) == 0
        bad = L.Pcen.from_buffer_copy(ok)
        bad.s = 0.0
        b2 = C.c_void_p()
        assert lib.mfcc_hip_bank_create_online_pcen(m._h, 2, C.byref(bad), 0, 0, 0, 2, C.byref(b2)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_bank_create_online_pcen(m._h, 0, C.byref(ok), 0, 0, 0, 2, C.byref(b2)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_bank_create_online_pcen(m._h, 2, C.byref(ok), 3, 5, 0, 2, C.byref(b2)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_bank_create_online_pcen(m._h, 2, C.byref(ok), 0, 0, 3, 2, C.byref(b2)) == L.ERROR_INVALID_PARAM
        assert not b2.value
        with pytest.raises(ValueError):
            m.stream_bank(2, fixed=True, pcen=True)
        with pytest.raises(ValueError):
            m.stream_bank(2, pcen=dict(s=0))
        with m.stream_bank(2, pcen=True):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.set_pcen(True)                                # the bank counts as a session
            assert e.value.code == L.ERROR_BUSY
        m.set_pcen(True)
