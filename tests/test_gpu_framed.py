"""Frame lengths below nfft on the GPU (``MFCC(win_length=...)``, mfcc_hip_create_framed): the fused 512 / hop 160
kernel and the generic kernel against the float64 reference of tests/framed_ref.py with the per-coefficient bound of
oracle/error_bound.py; tile and buffer edges of the new kernel; every float entry point against the dense device call
of the same handle, bit for bit; the post-passes; the fixed path's refusals; plain handles unchanged.

The range the fused kernel accepts beyond 400 / 13 -- frame lengths 160 .. 511, 1 .. 32 cepstra, the lifter -- is
computed at its ends, not only selected.  The steady state of the tile loop is tests/test_gpu_steady_state.py's.

Small shapes only: 37 to 48 frames per channel for the reference checks, at most a few tiles elsewhere."""
import numpy as np
import pytest

import framed_ref as fr
import kernel_families as kf
from kernel_families import as_np, same

pytestmark = pytest.mark.gpu

NEW = "mfcc_fused512_h160_kernel"
GENERIC = "mfcc_float_generic_kernel"
# the arithmetic of each kernel, read from its source (oracle/error_bound.py: MODELS): the new kernel contracts the mel
# bank on bf16 x 2-split operands and runs the DCT in fp32, like the four-wave form it repeats; the generic one is fp32
MODEL = {NEW: "bf16x2/fp32", GENERIC: "fp32/fp32"}
ASR = dict(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=13)

# id -> (MFCC arguments, kernel)
SHAPES = {
    "k400": (dict(ASR), NEW),
    "g400": (dict(ASR, impl="generic"), GENERIC),
    "k400_16f": (dict(ASR, nfilters=16), NEW),
    "k400_48k": (dict(ASR, samplerate=48000), NEW),                      # a filter on bin 0: the exact-DC instantiation
    "g200": (dict(nfft=256, hop=80, win_length=200, nfilters=20, nceptrums=13, power_scale=0), GENERIC),
    "g800": (dict(nfft=1024, hop=320, win_length=800, nfilters=40, nceptrums=13, power_scale=0), GENERIC),
}


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _length(nfr, pad, L=400, hop=160):
    """samples that give ``nfr`` frames: exactly the last frame's end (notebook), half a hop into the tail frame or, for
    one frame, short of a frame (stream)"""
    if pad == "notebook":
        return hop * (nfr - 1) + L
    return L - 7 if nfr == 1 else hop * (nfr - 2) + L + hop // 2


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _open(mfcc_amd, kw, kernel, **over):
    m = mfcc_amd.MFCC(**dict(kw, **over))
    name = m.kernel_name()
    if name != kernel:
        m.close()
        raise AssertionError("handle runs %s, not %s" % (name, kernel))
    return m


def _ref_kw(kw):
    ps = kw.get("power_scale", 512.0)
    return dict(L=kw["win_length"], hop=kw["hop"], nfft=kw["nfft"], n_mel=kw["nfilters"],
                sample_rate=int(kw.get("samplerate", 16000)), power_scale=float(ps) if ps else float(kw["nfft"]),
                n_cep=kw["nceptrums"], lifter=float(kw.get("lifter", 0.0)))


def _check(got, pcm, kw, kernel, pad="notebook", halo=0, what="", output="cepstra", all_bounded=False):
    """every coefficient of every frame of every channel against framed_ref; no frame is set aside (``all_bounded``:
    and the reference must bound every frame, or pin its -inf / NaN pattern)"""
    got, pcm = as_np(got), np.asarray(pcm)
    if pcm.ndim == 1:
        got, pcm = got[None], pcm[None]
    worst = 0.0
    for c in range(len(pcm)):
        ref, bound = fr.reference_and_bound(pcm[c], MODEL[kernel], pad_mode=pad, halo=halo, output=output, **_ref_kw(kw))
        if all_bounded:
            assert not np.isposinf(bound).any(), "%s channel %d: the reference leaves frames unbounded" % (what, c)
        worst = max(worst, fr.check(got[c], ref, bound, "%s channel %d" % (what, c)))
    return worst


# ------------------------------------------------------------------------------------------------ both kernels

@pytest.mark.parametrize("shape", list(SHAPES))
def test_both_kernels_meet_the_framed_reference(mfcc_amd, wav_pcm, shape):
    """The six kinds of channel at seed 3, 48 frames each, every coefficient of every frame."""
    kw, kernel = SHAPES[shape]
    L, hop = kw["win_length"], kw["hop"]
    n = 47 * hop + L + 5
    pcm = kf.channels(n, 3, wav_pcm)
    with _open(mfcc_amd, kw, kernel) as m:
        assert m.win_length == L and m.num_frames(n) == 48
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 48, kw["nceptrums"])
        worst = _check(got, pcm, kw, kernel, what=shape, all_bounded=True)
    print("%s: worst error / bound %.3f" % (shape, worst))


@pytest.mark.parametrize("shape", ["k400", "g400", "k400_48k", "k400_16f"])
def test_log_mel_rows_meet_the_framed_reference(mfcc_amd, wav_pcm, shape):
    kw, kernel = SHAPES[shape]
    n = 47 * 160 + 400 + 5
    pcm = kf.channels(n, 3, wav_pcm)
    with _open(mfcc_amd, kw, kernel, output="logmel") as m:
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 48, kw["nfilters"])
        _check(got, pcm, kw, kernel, what=shape + " logmel", output="logmel")


# ------------------------------------------------------------------------------------------------ edges, new kernel

@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("halo", [0, 1])
def test_tile_and_buffer_edges_of_the_new_kernel(mfcc_amd, wav_pcm, pad, halo):
    """Frame counts around a tile, 1 and 6 channels, odd and even channel strides; the tensor ends with the last
    channel's last sample, so the last frame's samples L .. 511 lie past the end of the buffer."""
    import torch
    L, hop = 400, 160
    with _open(mfcc_amd, ASR, NEW, pad_mode=pad) as m:
        for nfr in (1, 15, 16, 17, 33):
            n = _length(nfr, pad)
            assert m.num_frames(n) == nfr
            for nch in (1, 6):
                pcm = kf.channels(n + halo, 10 * nfr + nch, wav_pcm)[:nch]
                dense = as_np(m.process(_dev(pcm), halo=halo))
                assert dense.shape == (nch, nfr, 13)
                _check(dense, pcm, ASR, NEW, pad, halo, "%d frames, %d channels" % (nfr, nch))
                for extra in (1, 2, 3):                                  # strides n + halo + extra: odd and even
                    stride = n + halo + extra
                    flat = np.zeros(stride * (nch - 1) + n + halo, np.int16)
                    for c in range(nch):
                        flat[c * stride: c * stride + n + halo] = pcm[c]
                    view = torch.as_strided(_dev(flat), (nch, n + halo), (stride, 1))
                    assert same(m.process(view, halo=halo), dense), (nfr, nch, stride)


@pytest.mark.parametrize("pad", ["notebook", "stream"])
def test_lengths_around_one_frame(mfcc_amd, wav_pcm, pad):
    L, hop = 400, 160
    with _open(mfcc_amd, ASR, NEW, pad_mode=pad) as m, _open(mfcc_amd, dict(ASR, impl="generic"), GENERIC, pad_mode=pad) as g:
        for n in (L - 1, L, L + hop - 1, L + hop):
            pcm = kf.channels(n, n, wav_pcm, kinds=("speech", "uniform", "noise"))
            nf = fr.num_frames(n, L, hop, pad)
            assert m.num_frames(n) == g.num_frames(n) == nf
            for h, kernel in ((m, NEW), (g, GENERIC)):
                got = h.process(_dev(pcm))
                assert tuple(got.shape) == (3, nf, 13)
                if nf:
                    _check(got, pcm, ASR, kernel, pad, what="n = %d" % n)


def test_a_frame_does_not_depend_on_its_tile(mfcc_amd, wav_pcm):
    """k hops of other samples in front: frame f becomes frame f + k, other tile, other neighbours, the same bits; a
    silent frame's -inf stays in its own row."""
    hop, L = 160, 400
    x = kf.signal("noise", hop * 40 + L, 77, wav_pcm)
    x[hop * 10: hop * 10 + 3 * L] = 0
    pre = kf.signal("uniform", hop * 17, 78, wav_pcm)
    with _open(mfcc_amd, ASR, NEW) as m:
        a = as_np(m.process(_dev(x)))
        silent = np.isneginf(a[:, 0])
        assert silent.sum() >= 3 and np.isfinite(a[~silent]).all()
        for k in (1, 5, 15, 16, 17):
            b = as_np(m.process(_dev(np.concatenate([pre[:k * hop], x]))))
            assert same(a[1:], b[k + 1:]), k


# ------------------------------------------------------------------------------------------------ the accepted range

LENGTHS = [160, 161, 255, 511]                     # the ends of mfcc_fused160::supported, one off, and an odd middle


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("L", LENGTHS)
def test_frame_lengths_of_the_accepted_range(mfcc_amd, wav_pcm, L, pad):
    """The six kinds at 37 frames, every coefficient of every frame bounded; then 1, 16 and 17 frames in a tensor that
    ends with the last channel's last sample, so slots L .. 511 of the last frame lie past the end of the buffer (352
    samples at L = 160)."""
    kw = dict(ASR, win_length=L)
    with _open(mfcc_amd, kw, NEW, pad_mode=pad) as m:
        assert m.win_length == L
        worst = 0.0
        for nfr in (37, 1, 16, 17):
            n = _length(nfr, pad, L)
            assert m.num_frames(n) == nfr
            pcm = kf.channels(n, 7, wav_pcm)
            got = m.process(_dev(pcm))                                   # contiguous: nothing behind the last sample
            assert tuple(got.shape) == (len(kf.KINDS), nfr, 13)
            worst = max(worst, _check(got, pcm, kw, NEW, pad, what="L %d, %s, %d frames" % (L, pad, nfr),
                                      all_bounded=True))
    print("L %d, %s: worst error / bound %.3f" % (L, pad, worst))


@pytest.mark.parametrize("n_cep,lifter", [(1, 0.0), (16, 0.0), (17, 0.0), (32, 0.0), (13, 22.0), (32, 22.0)])
def test_cepstra_counts_and_the_lifter(mfcc_amd, wav_pcm, n_cep, lifter):
    kw = dict(ASR, nceptrums=n_cep, lifter=lifter)
    n = _length(37, "notebook")
    pcm = kf.channels(n, 7, wav_pcm)
    with _open(mfcc_amd, kw, NEW) as m:
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 37, n_cep)
        worst = _check(got, pcm, kw, NEW, what="%d cepstra, lifter %g" % (n_cep, lifter), all_bounded=True)
    print("%d cepstra, lifter %g: worst error / bound %.3f" % (n_cep, lifter, worst))


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("L", [160, 511])
def test_sessions_and_banks_at_the_ends_of_the_frame_lengths(mfcc_amd, wav_pcm, L, pad):
    """A session fed in uneven chunks and flushed, and a raw bank of 4, equal the dense call bit for bit.  L = hop: a
    line never holds a whole hop of history behind the frames it has produced."""
    kw = dict(ASR, win_length=L)
    n = 36 * 160 + L + 7
    pcm = kf.channels(n, 11, wav_pcm, kinds=("speech", "noise", "silences", "uniform"))
    with _open(mfcc_amd, kw, NEW, pad_mode=pad) as m:
        R = as_np(m.process(_dev(pcm)))
        assert R.shape == (4, m.num_frames(n), 13)
        _check(R, pcm, kw, NEW, pad, what="L %d, %s" % (L, pad))
        with m.stream() as s:
            rows = [s.push(c) for c in _chunks(pcm[0], (1, 159, 160, 161, 1000))]
            assert s.pending < L
            rows.append(s.flush())
            assert same(np.concatenate(rows), R[0]), (L, pad, "session")
        sizes = [(1, 159, 160, 161, 1000), (0, 700, 0, 33), (2048,), (399, 0, 1, 160)]
        with m.stream_bank(4) as b:
            rows = _feed(b, pcm, sizes, L)
            for u in range(4):
                assert same(rows[u], R[u]), (L, pad, "bank", u)


# ------------------------------------------------------------------------------------------------ entry points

def _chunks(x, sizes):
    pos, out = 0, []
    i = 0
    while pos < len(x):
        c = sizes[i % len(sizes)]
        out.append(x[pos:pos + c])
        pos += c
        i += 1
    return out


def _feed(bank, pcm, sizes, L):
    """stream u gets pcm[u] in chunks of sizes[u] (some of them 0), one chunk per push, nothing once it has run out;
    then a flush.  Returns the rows of every stream."""
    parts = [_chunks(pcm[u], sizes[u]) for u in range(len(pcm))]
    rows = [[] for _ in parts]
    while any(parts):
        for u, r in enumerate(bank.push([p.pop(0) if p else np.zeros(0, np.int16) for p in parts])):
            rows[u].append(r)
        assert int(bank.pending.max()) < L
    for u, r in enumerate(bank.flush()):
        rows[u].append(r)
    return [np.concatenate(r) for r in rows]


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("shape", ["k400", "g400", "g200"])
def test_every_float_entry_point_equals_the_dense_device_call(mfcc_amd, wav_pcm, shape, pad):
    import torch
    kw, kernel = SHAPES[shape]
    L, hop = kw["win_length"], kw["hop"]
    n = 36 * hop + L + 7
    pcm = kf.channels(n, 11, wav_pcm, kinds=("speech", "noise", "silences", "uniform"))
    with _open(mfcc_amd, kw, kernel, pad_mode=pad) as m:
        R = as_np(m.process(_dev(pcm)))
        nf = m.num_frames(n)
        assert R.shape == (4, nf, 13)
        # host dense
        assert same(m.process(pcm), R)
        # ragged: 0 frames, 1 frame, and a quiet utterance directly in front of a full-scale one
        quiet = (kf.signal("noise", 3 * hop + L, 5, wav_pcm) // 300).astype(np.int16)
        loud = kf.signal("square", 5 * hop + L + 3, 6, wav_pcm)
        utts = [pcm[0], np.zeros(0, np.int16), pcm[1][:L + hop - 1 if pad == "notebook" else L - 3], quiet, loud,
                pcm[2][:17 * hop + L], pcm[3]]
        one = [as_np(m.process(_dev(u))) if len(u) else m.process(u) for u in utts]
        assert len(one[1]) == (0 if pad == "notebook" else 1) and len(one[2]) == 1
        host = m.process_batch(utts)
        dev = m.process_batch([_dev(u) for u in utts])
        lens = [len(u) for u in utts]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        packed, fo = m.process_packed(_dev(np.concatenate(utts)), offs)
        eq, _ = m.process_packed(_dev(pcm.reshape(-1)), np.arange(5, dtype=np.uint64) * n)     # equal lengths
        torch.cuda.synchronize()
        for i, o in enumerate(one):
            assert same(host[i], o), (shape, pad, "host", i)
            assert same(dev[i], o), (shape, pad, "device", i)
            assert same(packed[int(fo[i]):int(fo[i + 1])], o), (shape, pad, "packed", i)
        assert same(eq, R.reshape(-1, 13))
        # time_launches runs the same launch into a caller's buffer
        out = torch.empty((4, nf, 13), device="cuda", dtype=torch.float32)
        assert m.time_launches(_dev(pcm), out, warmup=1, iters=2) > 0.0
        assert same(out, R)
        # a session fed in chunks, then flushed
        with m.stream() as s:
            rows = [s.push(c) for c in _chunks(pcm[0], (1, 159, 160, 161, 1000))]
            assert s.pending < L
            rows.append(s.flush())
            assert same(np.concatenate(rows), R[0]), (shape, pad, "session")
        # a raw bank of 4 with uneven chunks, some of them empty
        sizes = [(1, 159, 160, 161, 1000), (0, 700, 0, 33), (2048,), (399, 0, 1, 160)]
        with m.stream_bank(4) as b:
            rows = _feed(b, pcm, sizes, L)
            for u in range(4):
                assert same(rows[u], R[u]), (shape, pad, "bank", u)
    # an online bank equals the dense call of a handle with the same causal settings
    online = dict(normalize="meanvar", normalize_window=600, deltas=2)
    with _open(mfcc_amd, kw, kernel, pad_mode=pad, normalize_min_window=1, normalize_center=False, **online) as mo:
        Ro = as_np(mo.process(_dev(pcm)))
    with _open(mfcc_amd, kw, kernel, pad_mode=pad) as m, m.stream_bank(4, **online) as b:
        rows = _feed(b, pcm, sizes, L)
        for u in range(4):
            assert same(rows[u], Ro[u]), (shape, pad, "online bank", u)


@pytest.mark.parametrize("pad", ["notebook", "stream"])
def test_dist_frame_shards_of_a_framed_handle_concatenate_to_the_one_call(mfcc_amd, wav_pcm, pad):
    """``mfcc_amd.dist`` plans its spans with the handle's frame length: explicitly, and by default from the adapter."""
    from mfcc_amd import dist as md
    pcm = kf.signal("speech", _length(16 * 3 + 5, pad) + 53, 31, wav_pcm)
    for kw, kernel in (SHAPES["k400"], SHAPES["g200"]):
        with _open(mfcc_amd, kw, kernel, pad_mode=pad) as m:
            R = as_np(m.process(_dev(pcm)))
            nf = m.num_frames(len(pcm))
            compute = md.mfcc_compute(m)
            assert compute.frame_length == kw["win_length"]
            for world in (2, 3):
                for geo in (dict(nfft=m.nfft, hop=m.hop, frame_length=m.win_length), {}):
                    parts = [md.process_frames_sharded(compute, pcm, rank, world, 13, n_frames=nf, **geo)[1]
                             for rank in range(world)]
                    assert same(np.concatenate(parts), R), (kernel, pad, world, geo)
            with pytest.raises(ValueError):                              # spans planned for another frame length
                md.process_frames_sharded(compute, pcm, 0, 2, 13, n_frames=nf, frame_length=m.nfft)


def test_a_quiet_utterance_in_front_of_a_loud_one_keeps_its_rows(mfcc_amd, wav_pcm):
    """The quiet utterance's last frame reads the loud one's samples in slots L .. 511: they meet a zero window."""
    hop, L = 160, 400
    quiet = np.clip(kf.signal("noise", 20 * hop + L, 5, wav_pcm) // 1000, -3, 3).astype(np.int16)
    loud = kf.signal("square", 20 * hop + L + 3, 6, wav_pcm)
    for kw, kernel in (SHAPES["k400"], SHAPES["g400"]):
        with _open(mfcc_amd, kw, kernel) as m:
            alone = as_np(m.process(_dev(quiet)))
            batch = m.process_batch([_dev(quiet), _dev(loud)])
            assert same(batch[0], alone) and same(batch[1], m.process(_dev(loud)))
            both = as_np(m.process(_dev(np.stack([quiet, loud[:len(quiet)]]))))        # channels back to back
            assert same(both[0], alone)
            _check(alone, quiet, kw, kernel, what="quiet")


def test_convert_writes_the_float_rows(mfcc_amd, golden_dir, tmp_path):
    import os
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    with _open(mfcc_amd, dict(ASR), NEW) as m:
        out = str(tmp_path / "a.mfcc")
        assert m.convert(wav, out, fixed=False) == 1112
        outs = [str(tmp_path / "b.mfcc"), str(tmp_path / "c.mfcc")]
        m.convert_many([wav, wav], outs, fixed=False)
        a = np.fromfile(out, np.int16)
        assert a.size == 1112 * 13 and all(np.array_equal(np.fromfile(o, np.int16), a) for o in outs)
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.convert(wav, out, fixed=True)
        assert e.value.code == mfcc_amd._lib.ERROR_UNSUPPORTED
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            m.convert_many([wav], [out], fixed=True)
        assert e.value.code == mfcc_amd._lib.ERROR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ post-passes

def test_post_passes_on_framed_rows_equal_the_direct_entries(mfcc_amd, wav_pcm):
    hop, L = 160, 400
    utts = [kf.signal(k, hop * f + L + 3, 40 + i, wav_pcm)
            for i, (k, f) in enumerate((("speech", 70), ("silences", 33), ("noise", 16), ("speech", 1)))]
    devs = [_dev(u) for u in utts]
    with _open(mfcc_amd, ASR, NEW) as m:
        raw = m.process_batch(devs)
        fo = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64)
        import torch
        rows = torch.cat(list(raw))
        with _open(mfcc_amd, ASR, NEW, normalize="meanvar") as mn:
            assert same(torch.cat(list(mn.process_batch(devs))), m.normalize_rows(rows.clone(), fo, mode="meanvar"))
        with _open(mfcc_amd, ASR, NEW, deltas=2) as md:
            assert same(torch.cat(list(md.process_batch(devs))), m.deltas_rows(rows, fo, order=2))
        with _open(mfcc_amd, ASR, NEW, vad="select") as mv:
            sel = mv.process_batch(devs)
            voiced = m.vad_rows(rows, fo)
            picked, so = m.select_rows(rows, voiced, fo)
            assert [len(s) for s in sel] == np.diff(so.astype(np.int64)).tolist()
            assert same(torch.cat(list(sel)), picked)
            assert 0 < len(picked) <= len(rows)
    with _open(mfcc_amd, ASR, NEW, output="logmel") as ml:
        lm = ml.process_batch(devs)
        assert [tuple(r.shape) for r in lm] == [(len(r), 32) for r in raw]
        for u, r in zip(utts, lm):
            _check(r, u, ASR, NEW, what="logmel", output="logmel")


# ------------------------------------------------------------------------------------------------ refusals

def test_the_fixed_path_refuses_a_framed_handle(mfcc_amd, wav_pcm):
    import torch
    U = mfcc_amd._lib.ERROR_UNSUPPORTED
    x = kf.signal("speech", 4000, 1, wav_pcm)
    offs = np.array([0, 2000, 4000], np.uint64)
    # 512 / 170 / 32: the fixed path's own shape, refused only because of the frame length
    for kw in (dict(nfft=512, hop=170, win_length=400, nfilters=32, nceptrums=13), dict(ASR)):
        with mfcc_amd.MFCC(**kw) as m:
            out = torch.empty((1, 64, 13), device="cuda", dtype=torch.int16)
            calls = [lambda: m.process_fixed(x), lambda: m.process_fixed(_dev(x)), lambda: m.process_fixed(_dev(x), halo=1),
                     lambda: m.process_batch([x, x], fixed=True), lambda: m.process_batch([_dev(x), _dev(x[:3000])], fixed=True),
                     lambda: m.process_packed(_dev(x), offs, fixed=True),
                     lambda: m.time_launches(_dev(x), out, fixed=True), lambda: m.stream(fixed=True),
                     lambda: m.stream_bank(3, fixed=True)]
            for i, call in enumerate(calls):
                with pytest.raises(mfcc_amd.MfccHipError) as e:
                    call()
                assert e.value.code == U, (kw, i)
            assert len(m.process(x)) == m.num_frames(len(x))             # the float path of the same handle works


def test_impl_fused512_on_a_framed_handle_is_the_new_kernel_or_unsupported(mfcc_amd):
    with mfcc_amd.MFCC(**dict(ASR, impl="fused512")) as m:
        assert m.kernel_name() == NEW
    for kw in (dict(ASR, hop=170), dict(ASR, nfilters=20), dict(nfft=256, hop=80, win_length=200, nfilters=16, nceptrums=13)):
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            mfcc_amd.MFCC(**dict(kw, impl="fused512"))
        assert e.value.code == mfcc_amd._lib.ERROR_UNSUPPORTED
    for L in (160, 511):
        with mfcc_amd.MFCC(**dict(ASR, win_length=L)) as m:
            assert m.kernel_name() == NEW and m.win_length == L


# ------------------------------------------------------------------------------------------------ plain handles

def test_plain_handles_are_unchanged(mfcc_amd, wav_pcm):
    x = _dev(kf.channels(170 * 40 + 512 + 3, 9, wav_pcm))
    with mfcc_amd.MFCC(nfft=512, hop=160, nfilters=32, nceptrums=13) as m:
        assert m.kernel_name() == GENERIC and m.win_length == 512
        a = as_np(m.process(x))
    with mfcc_amd.MFCC(nfft=512, hop=160, nfilters=32, nceptrums=13, win_length=512) as m:
        assert m.kernel_name() == GENERIC and same(m.process(x), a)
    with mfcc_amd.MFCC() as m, mfcc_amd.MFCC(win_length=512) as w:
        assert m.kernel_name() == w.kernel_name() and m.win_length == w.win_length == 512
        assert same(m.process(x), w.process(x))
        assert same(m.process_fixed(x), w.process_fixed(x))
