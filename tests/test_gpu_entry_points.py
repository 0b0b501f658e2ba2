"""Every kernel family (tests/kernel_families.py) through every way into the kernels.

R is ONE ``process`` / ``process_fixed`` call on a device tensor of the whole input.  R meets the family's contract
(E1: the float64 oracle's per-coefficient error bound, or the RTL oracle bit for bit), and every other entry point
reproduces R bit for bit, -inf / NaN patterns included:

* E2  a shard with a one-sample history halo (``halo=1``) at frame k;
* E3  ``mfcc_amd.dist`` frame shards of 2-, 3- and 8-way plans;
* E4  the host-buffer copy pipeline (chunks of whole channels, frame ranges of a long channel with a halo and a cut
      ``n_samples``, ragged host batches, a caller-pinned buffer), with 1 MB chunks so that small inputs walk every path;
* E5  a streaming session (``halo = 1`` and ``force_frames`` on every launch) under many push patterns and a reset;
* E6  ragged batches: host arrays, device tensors and one flat device buffer, against per-utterance calls;
* E7  frame-shift independence: the same samples at another frame index (other tile, other neighbours) give the same
      row.

Geometry comes from each family's nfft / hop only."""
import numpy as np
import pytest

import kernel_families as kf
from kernel_families import ALL, IDS, as_np, open_handle, run, same

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _length(fam, n_frames, pad):
    """Samples that give ``n_frames`` frames in framing ``pad`` (and a part of a hop more for STREAM)."""
    if pad == "notebook":
        return fam.hop * (n_frames - 1) + fam.nfft
    return fam.hop * (n_frames - 2) + fam.nfft + fam.hop // 2


# ------------------------------------------------------------------------------------------------ E1

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e1_one_call_on_strided_channels_meets_the_oracle(mfcc_amd, wav_pcm, fam, pad):
    """Six kinds of channel at an odd channel stride from an odd base offset; frame counts 16 k + {0, 1, 15}."""
    import torch
    nch = len(kf.KINDS)
    worst = 0.0
    with open_handle(mfcc_amd, fam, pad) as m:
        for i, (k, r) in enumerate(((5, 0), (4, 1), (3, 15))):
            nfr = 16 * k + r
            n = _length(fam, nfr, pad)
            pcm = kf.channels(n, 100 * i + fam.nfft, wav_pcm)
            off = 2 * i + 1
            stride = n + 2 * i + 3
            stride += 1 - stride % 2
            flat = np.zeros(off + stride * nch + 8, np.int16)
            for c in range(nch):
                flat[off + c * stride: off + c * stride + n] = pcm[c]
            view = torch.as_strided(_dev(flat), (nch, n), (stride, 1), storage_offset=off)
            got = run(m, fam, view)
            assert tuple(got.shape) == (nch, nfr, fam.nceptrums) and m.num_frames(n) == nfr
            assert same(got, run(m, fam, _dev(pcm))), (fam.id, nfr)        # the same rows as a dense copy
            worst = max(worst, kf.check_oracle(fam, got, pcm, pad, what="%s %d frames" % (pad, nfr)))
    print("E1 %s %s: worst error / bound %.3f" % (fam.id, pad, worst))


# ------------------------------------------------------------------------------------------------ E2

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e2_a_halo_shard_is_the_rows_from_its_frame_on(mfcc_amd, wav_pcm, fam, pad):
    hop, nfft = fam.hop, fam.nfft
    nfr = 16 * 5 + 7
    n = _length(fam, nfr, pad) + 11
    pcm = kf.channels(n, 7 + fam.nfft, wav_pcm, kinds=("speech", "uniform", "silences"))
    x = _dev(pcm)
    with open_handle(mfcc_amd, fam, pad) as m:
        R = as_np(run(m, fam, x))
        nf = R.shape[1]
        for k in (1, 5, 16, 33, nf - 3):
            part = run(m, fam, x[:, hop * k - 1:], halo=1)                # a strided view: channel stride n
            assert same(part, R[:, k:]), (fam.id, pad, k)
            if k == 5:
                kf.check_oracle(fam, part, pcm[:, hop * k - 1:], pad, halo=1, what="halo shard at frame 5")
            # a shard that ends inside the stream: its rows up to there (STREAM adds a padded tail frame of its own)
            k2 = min(nf - 1, k + 17)
            mid = as_np(run(m, fam, x[:, hop * k - 1: hop * (k2 - 1) + nfft].contiguous(), halo=1))
            assert same(mid[:, :k2 - k], R[:, k:k2]), (fam.id, pad, k, k2)


# ------------------------------------------------------------------------------------------------ E3

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e3_dist_frame_shards_concatenate_to_the_one_call(mfcc_amd, wav_pcm, fam, pad):
    from mfcc_amd import dist as md
    nfr = 16 * 6 + 5
    pcm = kf.signal("speech", _length(fam, nfr, pad) + fam.hop // 3 + 1, 31, wav_pcm)
    with open_handle(mfcc_amd, fam, pad) as m:
        R = as_np(run(m, fam, _dev(pcm)))
        nf = m.num_frames(len(pcm))
        compute = md.mfcc_compute(m, fixed=fam.fixed)
        for world in (2, 3, 8):
            for geo in (dict(nfft=m.nfft, hop=m.hop), {}):              # explicit, and the handle's own by default
                parts = []
                for rank in range(world):
                    shard, loc = md.process_frames_sharded(compute, pcm, rank, world, fam.nceptrums, n_frames=nf, **geo)
                    assert loc.shape == (shard.n_frames, fam.nceptrums)
                    parts.append(loc)
                assert same(np.concatenate(parts), R), (fam.id, pad, world, geo)


# ------------------------------------------------------------------------------------------------ E4

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e4_host_copy_pipeline_equals_the_device_call(mfcc_amd, fam, pad, monkeypatch):
    """1 MB chunks (524 288 samples): frame ranges of one odd-length channel (>= 3 chunks) and of three long channels,
    several channels per chunk, a caller-pinned buffer, a ragged host batch."""
    import torch
    monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
    rng = np.random.default_rng(fam.nfft + len(pad))
    noise = lambda *shape: (rng.standard_normal(shape) * 3000).clip(-32768, 32767).astype(np.int16)   # noqa: E731
    with open_handle(mfcc_amd, fam, pad) as m:
        for nch, n in ((1, 3 * 524_288 + 4_099), (3, 600_001), (40, 20_001)):
            x = noise(nch, n)
            x[:, n // 3: n // 3 + 4 * fam.nfft] = 0                       # silent frames inside a chunk
            host = run(m, fam, x)
            dev = as_np(run(m, fam, _dev(x)))
            assert host.shape == dev.shape == (nch, m.num_frames(n), fam.nceptrums)
            assert same(host, dev), (fam.id, pad, nch, n)
            xp = torch.from_numpy(x).pin_memory()                        # already registered: neither fail nor unpin
            assert same(run(m, fam, xp.numpy()), dev), (fam.id, pad, nch, n, "pinned")
            del xp
        lens = [int(v) for v in rng.integers(0, 700_000, 9)] + [0, 1, fam.nfft, 3 * 524_288 + 1, 17, 200_003]
        utts = [noise(v) for v in lens]
        many = m.process_batch(utts, fixed=fam.fixed)
        assert len(many) == len(utts)
        for i, u in enumerate(utts):
            one = as_np(run(m, fam, _dev(u))) if len(u) else run(m, fam, u)
            assert same(many[i], one), (fam.id, pad, i, len(u))


# ------------------------------------------------------------------------------------------------ E5

def _pushes(n, kind, fam, rng):
    pos = 0
    while pos < n:
        if kind == "driver":                                  # the host driver's pattern: nfft, then hop per round
            c = fam.nfft if pos == 0 else fam.hop
        elif kind == "hop-1":
            c = max(1, fam.hop - 1)                           # hop 1: one sample per push, not none
        elif kind == "hop+1":
            c = fam.hop + 1
        elif kind == "random":
            c = int(rng.integers(1, 4097))
        elif kind == "single":
            c = n
        else:
            raise ValueError(kind)
        yield pos, min(n, pos + c)
        pos += c


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e5_streaming_session_equals_the_one_call(mfcc_amd, wav_pcm, fam, pad):
    pcm = kf.signal("silences", _length(fam, 16 * 4 + 3, pad) + 5 + 4 * fam.nfft, 55, wav_pcm)
    other = kf.signal("speech", _length(fam, 40, pad), 56, wav_pcm)
    rng = np.random.default_rng(fam.nfft)
    with open_handle(mfcc_amd, fam, pad) as m:
        R = as_np(run(m, fam, _dev(pcm)))
        R2 = as_np(run(m, fam, _dev(other)))
        with m.stream(fixed=fam.fixed) as s:
            for kind in ("driver", "hop-1", "hop+1", "random", "single"):
                rows = [s.push(pcm[a:b]) for a, b in _pushes(len(pcm), kind, fam, rng)]
                rows.append(s.flush())
                assert same(np.concatenate(rows), R), (fam.id, pad, kind)
                assert s.pending == 0
            # one sample per push over the first 2 nfft samples (the RTL's own rate), then the rest at once
            rows = [s.push(pcm[i:i + 1]) for i in range(2 * fam.nfft)]
            assert sum(len(r) for r in rows) == (2 * fam.nfft - fam.nfft) // fam.hop + 1
            rows += [s.push(pcm[2 * fam.nfft:]), s.flush()]
            assert same(np.concatenate(rows), R), (fam.id, pad, "one sample per push")
            # a reset mid-stream drops the frame in progress and the history: the next stream starts afresh
            s.push(pcm[:fam.nfft + fam.hop // 2])
            s.reset()
            assert s.pending == 0
            rows = [s.push(other[a:b]) for a, b in _pushes(len(other), "hop+1", fam, rng)] + [s.flush()]
            assert same(np.concatenate(rows), R2), (fam.id, pad, "after reset")


# ------------------------------------------------------------------------------------------------ E6

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e6_ragged_batches_equal_per_utterance_calls(mfcc_amd, wav_pcm, fam, pad):
    import torch
    hop, nfft = fam.hop, fam.nfft
    rng = np.random.default_rng(fam.nfft + 3)
    lens = [0, 1, nfft - 1, nfft, nfft + 1, nfft + hop - 1, nfft + hop, 16 * hop + nfft]
    lens += [nfft + hop * int(f) + int(e) for f, e in zip(rng.integers(0, 60, 6), rng.integers(0, hop, 6))]
    lens.insert(9, hop * 2000 + nfft + 3)                              # >= 2000 frames, not at either end
    kinds = ["speech", "noise", "uniform", "square", "silences"]
    utts = [kf.signal(kinds[i % len(kinds)], v, 200 + i, wav_pcm) for i, v in enumerate(lens)]
    with open_handle(mfcc_amd, fam, pad) as m:
        one = [run(m, fam, u) for u in utts]
        assert [len(o) for o in one] == [m.num_frames(v) for v in lens]
        host = m.process_batch(utts, fixed=fam.fixed)
        dev = m.process_batch([_dev(u) for u in utts], fixed=fam.fixed)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        packed, fo = m.process_packed(_dev(np.concatenate(utts)), offs, fixed=fam.fixed)
        eq, _ = m.process_packed(_dev(np.concatenate([utts[8]] * 3)), [0, lens[8], 2 * lens[8], 3 * lens[8]],
                                 fixed=fam.fixed)                      # equal lengths: the multi-channel form
        torch.cuda.synchronize()
    assert len(host) == len(dev) == len(utts)
    for i, o in enumerate(one):
        assert same(host[i], o), (fam.id, pad, "host", i, lens[i])
        assert same(dev[i], o), (fam.id, pad, "device", i, lens[i])
        assert same(packed[int(fo[i]):int(fo[i + 1])], o), (fam.id, pad, "packed", i, lens[i])
    assert same(eq, np.concatenate([one[8]] * 3))


# ------------------------------------------------------------------------------------------------ E7

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", ALL, ids=IDS)
def test_e7_a_row_does_not_depend_on_its_frame_index(mfcc_amd, wav_pcm, fam, pad):
    """k hops of other samples in front (every residue of a 16-frame tile, and 17, 33): frame f becomes frame f + k with
    the same samples and history, so rows a[1:] and b[k + 1:] must be the same bits, -inf / NaN patterns included."""
    hop = fam.hop
    x = kf.silent_stream(fam, 16 * 8 + 5, 77)
    pre = kf.signal("noise", hop * 33, 78, wav_pcm)
    with open_handle(mfcc_amd, fam, pad) as m:
        a = as_np(run(m, fam, _dev(x)))
        if not fam.fixed:
            assert np.isneginf(a[:, 0]).sum() >= 3                    # the silent frames are there
        for k in list(range(16)) + [17, 33]:
            b = as_np(run(m, fam, _dev(np.concatenate([pre[:k * hop], x]))))
            assert len(b) == len(a) + k
            assert same(a[1:], b[k + 1:]), (fam.id, pad, k)
    kf.check_oracle(fam, a, x, pad, what="silent stretches")
