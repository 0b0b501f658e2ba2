"""The stream bank (``MFCC.stream_bank`` / ``mfcc_hip_bank_*``): N online sessions advanced by one launch.

Every stream of a bank gets, bit for bit (-inf / NaN patterns included), the rows of the one-shot call on its whole
signal and, round by round, the rows a session of its own returns -- whatever each stream is fed per push:

* B1  any schedule, every kernel family, both framings, host and device entry;
* B2  2500 lines in lockstep: more streams than workgroups, rows written straight into the caller's tensor;
* B3  flush / reset of a subset, short streams, bad stream lists;
* B4  log-mel rows;
* B5  the contract's edges (small buffer, bad offsets, refused handles, BUSY, destroy order, a session next to it);
* B6  agreement with ``MfccStream`` per push.

Shapes are the smallest at which the bank's copy kernels can go wrong: chunk lengths around 0, 8 samples (one 16-byte
vector), the hop and the frame, carries that overlap their source, more records than the grid has workgroups."""
import ctypes as C

import numpy as np
import pytest

import kernel_families as kf
from kernel_families import ALL, IDS, open_handle, run, same

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]
BY_ID = {f.id: f for f in ALL}
EXTRA = (0, 1, 5, 15, 2)                       # B1: stream u has 16 * 3 + EXTRA[u] frames


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _length(fam, n_frames, pad):
    """Samples that give ``n_frames`` frames in framing ``pad`` (and half a hop more for STREAM)."""
    if pad == "notebook":
        return fam.hop * (n_frames - 1) + fam.nfft
    return fam.hop * (n_frames - 2) + fam.nfft + fam.hop // 2


def _sizes(fam):
    hop, nfft = fam.hop, fam.nfft
    return [0, 1, 2, 7, 8, 9, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, 3 * nfft + 5]


def _schedule(fam, lengths, seed):
    """Rounds of one chunk length per stream, each drawn on its own, until every stream is spent."""
    rng = np.random.default_rng(seed)
    pos = [0] * len(lengths)
    rounds = []
    while any(p < n for p, n in zip(pos, lengths)):
        cut = []
        for u, n in enumerate(lengths):
            c = min(int(rng.choice(_sizes(fam))), n - pos[u])
            cut.append((pos[u], pos[u] + c))
            pos[u] += c
        rounds.append(cut)
    return rounds


def _cat(rows, like):
    rows = [np.asarray(r) for r in rows]
    return np.concatenate(rows) if rows else like[:0]


def _push_host(bank, xs, rounds):
    got = [[] for _ in xs]
    for cut in rounds:
        for u, r in enumerate(bank.push([x[a:b] for x, (a, b) in zip(xs, cut)])):
            got[u].append(r)
    return got


def _push_dev(bank, xs, rounds):
    """Every round's chunks lie in ONE device tensor uploaded beforehand; all pushes are issued on a side stream with
    nothing between them, each into a tensor of the caller's, and only then is anything waited for or read."""
    import torch
    flats, offs = [], []
    for cut in rounds:
        chunks = [x[a:b] for x, (a, b) in zip(xs, cut)]
        offs.append(np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64))
        flats.append(np.concatenate(chunks))
    starts = np.concatenate([[0], np.cumsum([len(f) for f in flats])])
    big = torch.from_numpy(np.concatenate(flats + [np.zeros(8, np.int16)])).cuda()
    odt = torch.int16 if bank.fixed else torch.float32
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(side):
        for k, off in enumerate(offs):
            flat = big[int(starts[k]):int(starts[k + 1])]
            nf = int(bank.num_frames(np.diff(off.astype(np.int64)))[-1])
            out = torch.empty((nf, bank._row()), device="cuda", dtype=odt)
            res, fo = bank.push_packed(flat, off, out=out)
            assert res is out
            outs.append((out, fo))
    side.synchronize()
    got = [[] for _ in xs]
    for out, fo in outs:
        o = out.cpu().numpy()
        for u in range(len(xs)):
            got[u].append(o[int(fo[u]):int(fo[u + 1])])
    return got


# ------------------------------------------------------------------------------------------------ B1

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_b1_any_schedule_equals_the_one_shot_call(mfcc_amd, wav_pcm, fam, pad):
    kinds = kf.KINDS[:len(EXTRA)]
    lengths = [_length(fam, 48 + e, pad) for e in EXTRA]
    xs = [kf.signal(k, n, 31 * u + fam.nfft, wav_pcm) for u, (k, n) in enumerate(zip(kinds, lengths))]
    with open_handle(mfcc_amd, fam, pad) as m:
        one = [run(m, fam, x) for x in xs]
        assert [len(o) for o in one] == [48 + e for e in EXTRA]
        rounds = _schedule(fam, lengths, seed=fam.nfft + fam.hop)
        with m.stream_bank(len(xs), fixed=fam.fixed) as bank:
            for name, push in (("host", _push_host), ("device", _push_dev)):
                got = push(bank, xs, rounds)
                tails = bank.flush()
                assert not bank.pending.any()
                for u in range(len(xs)):
                    assert same(_cat(got[u] + [tails[u]], one[u]), one[u]), (fam.id, pad, name, u)
            # nfft - 1 samples (pending = nfft - 1), one more (the first frame; the carry overlaps its source whenever
            # hop < nfft - hop + 1), then a hop of one-sample pushes (the second frame), every stream alike
            n = fam.nfft + fam.hop
            cuts = [(0, fam.nfft - 1), (fam.nfft - 1, fam.nfft)] + [(i, i + 1) for i in range(fam.nfft, n)]
            got = _push_host(bank, [x[:n] for x in xs], [[c] * len(xs) for c in cuts])
            assert (bank.pending == fam.nfft - fam.hop).all()
            tails = bank.flush()
            for u, x in enumerate(xs):
                ref = run(m, fam, x[:n])
                assert len(ref) == (3 if pad == "stream" else 2)
                assert same(_cat(got[u] + [tails[u]], ref), ref), (fam.id, pad, "fixed schedule", u)


# ------------------------------------------------------------------------------------------------ B2

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fid", ["f512", "x512"])
def test_b2_lockstep_lines_beyond_the_grid(mfcc_amd, wav_pcm, fid, pad):
    """2500 lines of nfft + 2 hop + 3 samples (an odd number: the halves are 428 and 427 samples, every line alike in
    each push).  The first push only accumulates, the second completes three frames per line."""
    import torch
    fam = BY_ID[fid]
    n_streams, n = 2500, fam.nfft + 2 * fam.hop + 3
    x = np.stack([kf.signal("noise", n, 7000 + u, wav_pcm) for u in range(n_streams)])
    xd = torch.from_numpy(x).cuda()
    half = (n + 1) // 2
    with open_handle(mfcc_amd, fam, pad) as m, m.stream_bank(n_streams, fixed=fam.fixed) as bank:
        assert n_streams > 8 * torch.cuda.get_device_properties(0).multi_processor_count
        one = run(m, fam, xd)
        outs = []
        for part in (xd[:, :half], xd[:, half:]):
            w = part.shape[1]
            out, fo = bank.push_packed(part.contiguous().reshape(-1), np.arange(n_streams + 1, dtype=np.uint64) * w)
            assert len(np.unique(np.diff(fo.astype(np.int64)))) == 1              # uniform frame offsets
            outs.append(out.reshape(n_streams, int(fo[1]), out.shape[1]))
        assert outs[0].shape[1] == 0 and outs[1].shape[1] == 3
        assert (bank.pending == n - 3 * fam.hop).all()
        got = outs[1].cpu().numpy()
        if pad == "stream":
            got = np.concatenate([got, np.stack(bank.flush())], axis=1)
        assert same(got, one), (fid, pad)


# ------------------------------------------------------------------------------------------------ B3

@pytest.mark.parametrize("pad", PADS)
def test_b3_subsets_short_streams_and_bad_lists(mfcc_amd, wav_pcm, pad):
    fam = BY_ID["x512"]
    nfft, hop = fam.nfft, fam.hop
    tail = 1 if pad == "stream" else 0
    xs = [kf.signal("noise", 2400, 50 + u, wav_pcm) for u in range(4)]
    ys = [kf.signal("uniform", 1500, 60 + u, wav_pcm) for u in range(4)]
    with open_handle(mfcc_amd, fam, pad) as m, m.stream_bank(4, fixed=True) as bank:
        first = [700, 650, 1100, 333]
        a = bank.push([x[:k] for x, k in zip(xs, first)])
        t = bank.flush([3, 1])                                   # in the order listed
        assert [len(r) for r in t] == [tail, tail]
        assert same(_cat([a[3], t[0]], a[3]), run(m, fam, xs[3][:333]))
        assert same(_cat([a[1], t[1]], a[1]), run(m, fam, xs[1][:650]))
        pend = bank.pending
        assert pend[1] == 0 and pend[3] == 0 and pend[0] == 700 - hop * 2 and pend[2] == 1100 - hop * 4
        # 1 and 3 start new signals; 0 and 2 carry on
        b = bank.push([xs[0][700:], ys[1], xs[2][1100:], ys[3]])
        t = bank.flush()
        assert same(_cat([a[0], b[0], t[0]], a[0]), run(m, fam, xs[0]))
        assert same(_cat([a[2], b[2], t[2]], a[2]), run(m, fam, xs[2]))
        assert same(_cat([b[1], t[1]], b[1]), run(m, fam, ys[1]))
        assert same(_cat([b[3], t[3]], b[3]), run(m, fam, ys[3]))
        # reset mid-frame: pending samples and the history sample go (700 samples: one carry, a history that is not 0)
        empty = xs[0][:0]
        assert len(bank.push([empty, empty, xs[2][:700], xs[3][:100]])[2]) == 2
        bank.reset([2])
        pend = bank.pending
        assert pend[2] == 0 and pend[3] == 100
        c = bank.push([empty, empty, ys[2], xs[3][100:900]])
        t = bank.flush([2, 3])
        assert same(_cat([c[2], t[0]], c[2]), run(m, fam, ys[2]))
        assert same(_cat([c[3], t[1]], c[3]), run(m, fam, xs[3][:900]))
        # streams shorter than a frame: the driver's single zero-padded frame
        short = [0, 1, 100, nfft - 1]
        s = bank.push([x[:k] for x, k in zip(xs, short)])
        assert [len(r) for r in s] == [0, 0, 0, 0] and list(bank.pending) == short
        t = bank.flush()
        for u, k in enumerate(short):
            assert len(t[u]) == tail and same(t[u], run(m, fam, xs[u][:k])), (pad, k)
        # a bad list is refused whole
        bank.push([x[:200] for x in xs])
        for bad in ([1, 1], [0, 4], [2, 3, 2]):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                bank.flush(bad)
            assert e.value.code == -101
            with pytest.raises(mfcc_amd.MfccHipError):
                bank.reset(bad)
            assert list(bank.pending) == [200] * 4
        d = bank.push([x[200:] for x in xs])
        t = bank.flush()
        for u in range(4):
            assert same(_cat([d[u], t[u]], d[u]), run(m, fam, xs[u]))


# ------------------------------------------------------------------------------------------------ B4

@pytest.mark.parametrize("pad", PADS)
def test_b4_logmel_rows(mfcc_amd, pad):
    fam = BY_ID["f512"]
    xs = [kf.silent_stream(fam, 40 + 3 * u, 90 + u) for u in range(3)]
    with open_handle(mfcc_amd, fam, pad, output="logmel") as m, m.stream_bank(3) as bank:
        one = [m.process(x) for x in xs]
        assert one[0].shape[1] == fam.nfilters and any(np.isneginf(o).any() for o in one)
        for push in (_push_host, _push_dev):
            got = push(bank, xs, _schedule(fam, [len(x) for x in xs], seed=5))
            tails = bank.flush()
            for u in range(3):
                assert got[u][0].shape[1] == fam.nfilters
                assert same(_cat(got[u] + [tails[u]], one[u]), one[u]), (pad, u)


# ------------------------------------------------------------------------------------------------ B5

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_b5_refused_pushes_leave_the_bank_as_it_was(mfcc_amd, wav_pcm):
    lib = mfcc_amd.load_library()
    fam = BY_ID["f512"]
    xs = [np.ascontiguousarray(wav_pcm[3000 * u:3000 * u + 2000]) for u in range(3)]
    with open_handle(mfcc_amd, fam) as m, m.stream_bank(3) as bank:
        bank.push([x[:300] for x in xs])
        flat = np.concatenate([x[300:] for x in xs])
        offsets = (np.arange(4) * 1700).astype(np.uint64)
        out = np.empty((5, 13), np.float32)
        fo = np.full(4, 77, np.uint64)
        rc = lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(offsets), _ptr(out), out.size, _ptr(fo))
        assert rc == -106 and list(fo) == [0, 9, 18, 27]                     # BUFFER_SMALL, the counts are there
        assert list(bank.pending) == [300] * 3
        dec = np.array([0, 1700, 1600, 3400], np.uint64)
        big = np.empty((27, 13), np.float32)
        assert lib.mfcc_hip_bank_push(bank._b, _ptr(flat), _ptr(dec), _ptr(big), big.size, _ptr(fo)) == -101
        assert lib.mfcc_hip_bank_push_dev(bank._b, None, _ptr(dec), None, 0, _ptr(fo)) == -101
        assert list(bank.pending) == [300] * 3
        rows = bank.push([x[300:] for x in xs])
        for u in range(3):
            assert same(rows[u], m.process(xs[u])), u


def test_b5_handles_a_bank_refuses_and_busy_setters(mfcc_amd):
    for kw in (dict(normalize="mean"), dict(deltas=1), dict(vad="select")):
        with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, **kw) as m:
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.stream_bank(2)
            assert e.value.code == -105, kw
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, output="logmel") as m:
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.stream_bank(2, fixed=True)
        assert e.value.code == -105
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        with m.stream_bank(2):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.set_deltas(1)
            assert e.value.code == -104
        m.set_deltas(1)                                        # free again once the bank is gone


def test_b5_destroy_order_and_a_session_next_to_the_bank(mfcc_amd, wav_pcm):
    x, y = np.ascontiguousarray(wav_pcm[:3000]), np.ascontiguousarray(wav_pcm[9000:12000])
    m = mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream")
    one_x, one_y, one_half = m.process(x), m.process(y), m.process(y[:1500])
    bank = m.stream_bank(2)
    with m.stream() as s:
        got_b, got_s = [[], []], []
        for k in range(6):                                     # the session and the bank take turns on one handle
            r = bank.push([x[500 * k:500 * (k + 1)], y[250 * k:250 * (k + 1)]])
            got_s.append(s.push(y[500 * k:500 * (k + 1)]))
            got_b[0].append(r[0])
            got_b[1].append(r[1])
        got_s.append(s.flush())
        assert same(np.concatenate(got_s), one_y)
    m.close()                                                  # the handle first: the bank keeps it alive
    t = bank.flush()
    assert same(np.concatenate(got_b[0] + [t[0]]), one_x)
    assert same(np.concatenate(got_b[1] + [t[1]]), one_half)
    bank.close()
    bank.close()


# ------------------------------------------------------------------------------------------------ B6

def test_b6_the_bank_is_n_sessions(mfcc_amd, wav_pcm):
    fam = BY_ID["f512"]
    xs = [kf.signal(k, 9000 + 300 * u, 11 + u, wav_pcm) for u, k in enumerate(["speech", "noise", "silences"])]
    rounds = _schedule(fam, [len(x) for x in xs], seed=77)
    with open_handle(mfcc_amd, fam, "stream") as m, m.stream_bank(3) as bank:
        sessions = [m.stream() for _ in xs]
        try:
            for k, cut in enumerate(rounds):
                rows = bank.push([x[a:b] for x, (a, b) in zip(xs, cut)])
                for u, (a, b) in enumerate(cut):
                    assert same(rows[u], sessions[u].push(xs[u][a:b])), (k, u)
                assert list(bank.pending) == [s.pending for s in sessions]
            tails = bank.flush()
            for u, s in enumerate(sessions):
                assert same(tails[u], s.flush()), u
        finally:
            for s in sessions:
                s.close()
