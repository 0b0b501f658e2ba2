"""The online stream bank (``MFCC.stream_bank(n, normalize=..., normalize_window=N, deltas=K, delta_window=Nd)`` /
``mfcc_hip_bank_create_online``): causal CMVN and lagged deltas as device state of a bank.

Any pushes followed by a flush give every stream, bit for bit (-inf / NaN patterns included), the rows of the one-shot
call on its whole signal by a handle with the same settings (purely causal window, min_window 1):

* O1  seeded schedules, both entries, both framings, five kernel families, four settings;
* O2  the same rows against the float64 references, without the one-shot kernels;
* O3  2500 lines in lockstep: more records than workgroups, ``held`` and ``num_frames`` against the plan;
* O4  flush / reset of subsets, ragged flush offsets, one frame per push against one push;
* O5  the contract's edges.

Shapes are the smallest at which the kernels can go wrong: streams of 0, 1 and 3 frames (shorter than the lag, clamped
on both sides), windows without a finite value, a variance of exactly 0 (the stale-sums restart), a ring that wraps
twice with runs that start before the first new row (N = 600), W = 64 (four runs per workgroup)."""
import ctypes as C

import numpy as np
import pytest

import deltas_ref
import kernel_families as kf
import normalize_sliding_ref as nsr
import online_ref as on
from kernel_families import open_handle, same

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]
FAMS = ["f512", "f1024", "g256", "g128_h1", "g1024_64"]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _over(fid):
    return dict(output="logmel") if fid == "g1024_64" else {}


def _streams(fam, pad, wav_pcm, frames, const_frames):
    """Ordinary streams of unequal length, one of 1 frame, one of 3, one that never gets samples, one with silences
    (-inf rows), noise followed by constant -32768."""
    a, b = frames
    return [kf.signal("speech", on.length(fam, a, pad), 3, wav_pcm),
            kf.signal("noise", on.length(fam, b, pad), 5, wav_pcm),
            kf.signal("noise", on.length(fam, 1, pad), 6, wav_pcm),
            kf.signal("uniform", on.length(fam, 3, pad), 7, wav_pcm),
            np.zeros(0, np.int16),
            kf.silent_stream(fam, a + 7, 8),
            on.noise_then_const(fam, 20, const_frames, pad, 9)]


def _check_schedule(mfcc_amd, fam, pad, cfg, xs, rounds, over, tag):
    with open_handle(mfcc_amd, fam, pad, **over, **on.one_shot_kwargs(cfg)) as m1:
        one = [m1.process(x) for x in xs]
    assert any(not np.isfinite(o).all() for o in one), "no -inf / NaN row among the inputs"
    with open_handle(mfcc_amd, fam, pad, **over) as m, m.stream_bank(len(xs), **cfg) as bank:
        assert bank.lag == on.lag_of(cfg) and bank.num_features == one[0].shape[1]
        for name, push in (("host", on.push_host), ("device", on.push_dev)):
            got = push(bank, xs, rounds)
            assert int(bank.held.max()) <= bank.lag
            tails = bank.flush()
            assert not bank.pending.any() and not bank.held.any()
            for u in range(len(xs)):
                assert same(on.cat(got[u] + [tails[u]], one[u]), one[u]), (tag, name, u)


# ------------------------------------------------------------------------------------------------ O1

@pytest.mark.parametrize("cfg", list(on.SETTINGS), ids=list(on.SETTINGS))
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fid", FAMS)
def test_o1_any_schedule_equals_the_one_shot_call(mfcc_amd, wav_pcm, fid, pad, cfg):
    fam = on.BY_ID[fid]
    # N + S = 72 rows of ring at N = 40: the constant part is longer than that
    xs = _streams(fam, pad, wav_pcm, frames=(90, 131), const_frames=100)
    rounds = on.schedule([len(x) for x in xs], seed=fam.nfft + fam.hop, choices=on.sizes(fam))
    _check_schedule(mfcc_amd, fam, pad, on.SETTINGS[cfg], xs, rounds, _over(fid), (fid, pad, cfg))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fid", ["f512", "g128_h1"])
def test_o1_long_window_ring_wraps_and_runs_start_before_the_push(mfcc_amd, wav_pcm, fid, pad):
    """N = 600: S = 150, the ring holds 750 rows and wraps twice in 1700 frames; almost every push starts inside a run.
    Chunks from nothing to more frames than the ring holds (one push then writes only its last 750 rows to it)."""
    fam = on.BY_ID[fid]
    hop, nfft = fam.hop, fam.nfft
    xs = [kf.signal("noise", on.length(fam, 1700, pad), 21, wav_pcm),
          kf.silent_stream(fam, 1711, 22),
          on.noise_then_const(fam, 100, 1650, pad, 23)]              # constant for more than N + S = 750 frames
    choices = on.sizes(fam) + [40 * hop + 1, 149 * hop, 151 * hop + 3, 300 * hop + nfft, 800 * hop + 5] * 2
    rounds = on.schedule([len(x) for x in xs], seed=nfft, choices=choices)
    _check_schedule(mfcc_amd, fam, pad, on.MEANVAR600_DD2, xs, rounds, {}, (fid, pad, "meanvar600_dd2"))


# ------------------------------------------------------------------------------------------------ O2

@pytest.mark.parametrize("pad", PADS)
def test_o2_rows_against_the_float64_references(mfcc_amd, wav_pcm, pad):
    fam = on.BY_ID["f512"]
    cfg = on.MEANVAR40_DD2
    xs = [kf.signal("speech", on.length(fam, 150, pad), 3, wav_pcm), kf.silent_stream(fam, 140, 4),
          on.noise_then_const(fam, 20, 100, pad, 5)]
    rounds = on.schedule([len(x) for x in xs], seed=9, choices=on.sizes(fam))
    with open_handle(mfcc_amd, fam, pad) as m, m.stream_bank(len(xs), **cfg) as bank:
        raw = [m.process(x) for x in xs]
        got = on.push_host(bank, xs, rounds)
        tails = bank.flush()
        for u, r in enumerate(raw):
            rows = on.cat(got[u] + [tails[u]], r)
            T, W = r.shape
            assert rows.shape == (T, 3 * W)
            static = np.ascontiguousarray(rows[:, :W])
            worst = nsr.check(static, r, [0, T], mode="meanvar", window=40, min_window=1, center=False,
                              what="%s stream %d" % (pad, u))
            assert worst <= 1.0
            assert deltas_ref.check_stage(rows, static, [0, T], order=2, window=2, what="%s stream %d" % (pad, u)) <= 1.0


# ------------------------------------------------------------------------------------------------ O3

def test_o3_lockstep_lines_beyond_the_grid(mfcc_amd, wav_pcm):
    """2500 lines, the first push a frame, then six of one hop each: every line alike in each push, one delta record
    per line (more than 8 per CU), 19 CMVN runs per workgroup."""
    import torch
    fam = on.BY_ID["f512"]
    cfg = on.MEANVAR40_DD2
    n_streams, n_push = 2500, 7
    n = fam.nfft + (n_push - 1) * fam.hop
    x = np.stack([kf.signal("noise", n, 7000 + u, wav_pcm) for u in range(n_streams)])
    xd = torch.from_numpy(x).cuda()
    with open_handle(mfcc_amd, fam, "stream", **on.one_shot_kwargs(cfg)) as m1:
        one = m1.process(xd).cpu().numpy()
    model = on.Model(fam, n_streams, on.lag_of(cfg))
    with open_handle(mfcc_amd, fam, "stream") as m, m.stream_bank(n_streams, **cfg) as bank:
        assert n_streams > 8 * torch.cuda.get_device_properties(0).multi_processor_count
        outs, a = [], 0
        for k in range(n_push):
            w = fam.nfft if k == 0 else fam.hop
            part = xd[:, a:a + w].contiguous().reshape(-1)
            a += w
            want = model.push([w] * n_streams)
            fo = bank.num_frames([w] * n_streams)
            assert np.array_equal(np.diff(fo.astype(np.int64)), want), k
            out, fo2 = bank.push_packed(part, np.arange(n_streams + 1, dtype=np.uint64) * w)
            assert np.array_equal(fo2, fo) and np.array_equal(bank.held, model.held), k
            outs.append(out.reshape(n_streams, want[0], out.shape[1]))
        assert [o.shape[1] for o in outs] == [0, 0, 0, 0, 1, 1, 1]
        got = torch.cat(outs, dim=1).cpu().numpy()
        tails = bank.flush()
        assert all(len(t) == 5 for t in tails)                                   # held 4 and the tail frame
        got = np.concatenate([got, np.stack(tails)], axis=1)
        assert same(got, one)


# ------------------------------------------------------------------------------------------------ O4

@pytest.mark.parametrize("pad", PADS)
def test_o4_flush_and_reset_of_subsets(mfcc_amd, wav_pcm, pad):
    fam = on.BY_ID["f512"]
    cfg = on.MEANVAR40_DD2
    hop, nfft = fam.hop, fam.nfft
    tail = 1 if pad == "stream" else 0
    xs = [kf.signal("noise", on.length(fam, 60, pad), 50 + u, wav_pcm) for u in range(4)]
    ys = [kf.signal("uniform", on.length(fam, 9, pad), 60 + u, wav_pcm) for u in range(4)]
    with open_handle(mfcc_amd, fam, pad, **on.one_shot_kwargs(cfg)) as m1:
        one_x, one_y = [m1.process(x) for x in xs], [m1.process(y) for y in ys]
        first = [nfft + 20 * hop, nfft + 30 * hop + 7, nfft + 2 * hop, nfft + hop]
        one_short = m1.process(xs[3][:first[3]])                                 # 2 frames (3 with the tail)
        one_part = m1.process(xs[1][:first[1]])
    lib = mfcc_amd.load_library()
    with open_handle(mfcc_amd, fam, pad) as m, m.stream_bank(4, **cfg) as bank:
        a = bank.push([x[:k] for x, k in zip(xs, first)])
        assert list(bank.held) == [4, 4, 3, 2] and [len(r) for r in a] == [17, 27, 0, 0]
        # the ragged offsets, in the order listed: stream 3 holds 2 rows, stream 1 holds 4
        s = np.array([3, 1], np.uint64)
        out = np.empty((12, bank.num_features), np.float32)
        fo = np.full(3, 77, np.uint64)
        small = lib.mfcc_hip_bank_flush_ragged(bank._b, s.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p),
                                               5 * bank.num_features, fo.ctypes.data_as(C.c_void_p))
        assert small == -106 and list(fo) == [0, 2 + tail, 6 + 2 * tail] and list(bank.held) == [4, 4, 3, 2]
        rc = lib.mfcc_hip_bank_flush_ragged(bank._b, s.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p),
                                            out.size, fo.ctypes.data_as(C.c_void_p))
        assert rc == 0 and list(fo) == [0, 2 + tail, 6 + 2 * tail]
        assert same(out[:int(fo[1])], one_short)
        assert same(on.cat([a[1], out[int(fo[1]):int(fo[2])]], a[1]), one_part)
        assert list(bank.held) == [4, 0, 3, 0] and bank.pending[1] == 0 and bank.pending[3] == 0
        # 1 and 3 start new signals; 0 and 2 carry on, bit for bit
        b = bank.push([xs[0][first[0]:], ys[1], xs[2][first[2]:], ys[3]])
        t = bank.flush()
        assert same(on.cat([a[0], b[0], t[0]], a[0]), one_x[0])
        assert same(on.cat([a[2], b[2], t[2]], a[2]), one_x[2])
        assert same(on.cat([b[1], t[1]], b[1]), one_y[1])
        assert same(on.cat([b[3], t[3]], b[3]), one_y[3])
        # reset: the window, the held rows and the frame count go
        empty = xs[0][:0]
        bank.push([empty, empty, xs[2][:nfft + 50 * hop], xs[3][:100]])
        assert bank.held[2] == 4
        bank.reset([2])
        assert bank.held[2] == 0 and bank.pending[2] == 0 and bank.pending[3] == 100
        c = bank.push([empty, empty, ys[2], empty])
        t = bank.flush([2])
        assert same(on.cat([c[2], t[0]], c[2]), one_y[2])
        bank.reset()
        # one frame per push against one single push
        x = xs[0]
        cuts = [(0, nfft)] + [(k, min(k + hop, len(x))) for k in range(nfft, len(x), hop)]
        got = on.push_host(bank, [x, x[:0], x[:0], x[:0]], [[c, (0, 0), (0, 0), (0, 0)] for c in cuts])
        assert max(len(r) for r in got[0]) == 1
        t = bank.flush([0])
        single = bank.push([x, empty, empty, empty])
        t2 = bank.flush([0])
        assert same(on.cat(got[0] + [t[0]], one_x[0]), one_x[0])
        assert same(on.cat([single[0], t2[0]], one_x[0]), one_x[0])


# ------------------------------------------------------------------------------------------------ O5

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_o5_refused_handles_and_settings(mfcc_amd):
    lib = mfcc_amd.load_library()
    for kw in (dict(normalize="mean"), dict(deltas=1), dict(vad="select")):
        with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, **kw) as m:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.stream_bank(2, deltas=1)
            assert e.value.code == -105, kw
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        with pytest.raises(ValueError):
            m.stream_bank(2, fixed=True, deltas=1)
        b = C.c_void_p()
        for args in ((1, 0, 0, 2), (2, 16385, 0, 2), (3, 5, 0, 2), (0, 0, 3, 2), (0, 0, 1, 0), (0, 0, 1, 9), (0, 0, -1, 2)):
            assert lib.mfcc_hip_bank_create_online(m._h, 2, *args, C.byref(b)) == -101 and not b.value, args
        assert lib.mfcc_hip_bank_create_online(m._h, 0, 1, 5, 0, 2, C.byref(b)) == -101
        with m.stream_bank(2, deltas=1):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.set_deltas(1)                                # the bank counts as a session
            assert e.value.code == -104
        m.set_deltas(1)


def test_o5_small_buffer_consumes_nothing_and_flush_wants_the_ragged_form(mfcc_amd, wav_pcm):
    lib = mfcc_amd.load_library()
    fam = on.BY_ID["f512"]
    cfg = on.MEANVAR40_DD2
    xs = [np.ascontiguousarray(wav_pcm[3000 * u:3000 * u + 4000]) for u in range(3)]
    with open_handle(mfcc_amd, fam, **on.one_shot_kwargs(cfg)) as m1:
        one = [m1.process(x) for x in xs]
    with open_handle(mfcc_amd, fam) as m, m.stream_bank(3, **cfg) as bank:
        first = bank.push([x[:1400] for x in xs])                                # 6 frames, 2 returned, 4 held
        assert [len(r) for r in first] == [2, 2, 2] and list(bank.held) == [4, 4, 4]
        flat = np.concatenate([x[1400:] for x in xs])
        offsets = (np.arange(4) * 2600).astype(np.uint64)
        W = bank.num_features
        assert W == 39
        out = np.empty((44, W), np.float32)                                      # 45 rows are due: 15 per stream
        fo = np.full(4, 77, np.uint64)
        rc = lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(offsets), _ptr(out), out.size, _ptr(fo))
        assert rc == -106 and list(fo) == [0, 15, 30, 45]
        assert lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(offsets), _ptr(out), 45 * 13, _ptr(fo)) == -106
        assert list(bank.held) == [4, 4, 4] and list(bank.pending) == [1400 - 6 * fam.hop] * 3
        nf = C.c_size_t(0)
        assert lib.mfcc_hip_bank_flush(bank._b, None, 0, _ptr(out), out.size, C.byref(nf)) == -105
        assert list(bank.held) == [4, 4, 4]
        rows = bank.push([x[1400:] for x in xs])                                 # the same push, with room
        tails = bank.flush()
        for u in range(3):
            assert same(on.cat([first[u], rows[u], tails[u]], one[u]), one[u]), u


@pytest.mark.parametrize("pad", PADS)
def test_o5_plain_banks_next_to_an_online_one(mfcc_amd, wav_pcm, pad):
    """A plain bank on the same handle is unaffected; an online bank without settings (NONE, order 0) is the plain
    bank bit for bit; a bank without a lag still takes mfcc_hip_bank_flush."""
    lib = mfcc_amd.load_library()
    fam = on.BY_ID["f512"]
    xs = [kf.signal(k, on.length(fam, 40 + 3 * u, pad), 11 + u, wav_pcm) for u, k in enumerate(["speech", "noise"])]
    rounds = on.schedule([len(x) for x in xs], seed=3, choices=on.sizes(fam))
    with open_handle(mfcc_amd, fam, pad, **on.one_shot_kwargs(on.MEAN5)) as m1:
        one_mean = [m1.process(x) for x in xs]
    with open_handle(mfcc_amd, fam, pad) as m:
        one = [m.process(x) for x in xs]
        with m.stream_bank(2) as plain, m.stream_bank(2, **on.MEANVAR40_DD2) as online, \
                m.stream_bank(2, normalize_window=7) as none, m.stream_bank(2, **on.MEAN5) as mean:
            assert none.online and none.lag == 0 and none.num_features == 13 and plain.lag == 0
            got_p, got_n, got_m = [[], []], [[], []], [[], []]
            for cut in rounds:                                         # the four banks take turns on one handle
                chunks = [x[a:b] for x, (a, b) in zip(xs, cut)]
                online.push(chunks)
                for got, bank in ((got_p, plain), (got_n, none), (got_m, mean)):
                    for u, r in enumerate(bank.push(chunks)):
                        got[u].append(r)
            nf = C.c_size_t(0)
            out = np.empty((2, 13), np.float32)
            assert lib.mfcc_hip_bank_flush(mean._b, None, 0, _ptr(out), out.size, C.byref(nf)) == 0
            assert nf.value == (2 if pad == "stream" else 0)
            tp, tn = plain.flush(), none.flush()
            for u in range(2):
                assert same(on.cat(got_p[u] + [tp[u]], one[u]), one[u]), u
                assert same(on.cat(got_n[u] + [tn[u]], one[u]), one[u]), u
                assert same(on.cat(got_m[u] + [out[u:u + 1][:nf.value // 2]], one_mean[u]), one_mean[u]), u
