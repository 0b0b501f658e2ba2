"""HTK-style mel banks on the GPU (``MFCC(mel="htk", fmin=..., fmax=...)``, mfcc_hip_create_banked): the fused 512 /
hop 160 kernel for one to four filter blocks and the generic kernel against the float64 reference of
tests/melbank_ref.py with the per-coefficient bound of oracle/error_bound.py; tile and buffer edges of the new kernel;
a frame's independence of its tile; every float entry point against the dense device call of the same handle, bit for
bit; selection and refusals; notebook-bank handles unchanged.

The range the fused kernel accepts beyond 400 / 13 / eight banks -- frame lengths 160 .. 511, 1 .. 16 cepstra, the
lifter, log-mel rows wider than 16, and the set masks of kernel_families.MASK_BANKS, which drive its mel contraction --
is computed, not only selected.  The steady state of the tile loop is tests/test_gpu_steady_state.py's.

Small shapes only: 37 to 48 frames per channel for the reference checks, at most a few tiles elsewhere."""
import numpy as np
import pytest

import kernel_families as kf
import melbank_ref as mr
from kernel_families import as_np, same

pytestmark = pytest.mark.gpu

NEW = "mfcc_fused512_h160_mb_kernel"
H160 = "mfcc_fused512_h160_kernel"
GENERIC = "mfcc_float_generic_kernel"
# the arithmetic of each kernel, read from its source (oracle/error_bound.py: MODELS; eb.model_of does not know the new
# name): the new kernel contracts the mel bank on bf16 x 2-split operands and runs the DCT in fp32, like the hop-160
# form it repeats; the generic one is fp32 throughout
MODEL = {NEW: "bf16x2/fp32", GENERIC: "fp32/fp32"}
ASR = dict(nfft=512, hop=160, win_length=400, nceptrums=13, mel="htk")


def _htk(n_mel, fmin, fmax, rate=16000, **over):
    return dict(ASR, nfilters=n_mel, fmin=fmin, fmax=fmax, samplerate=rate, **over)


# id -> MFCC arguments of an HTK handle at 400 / 160 / 512; each runs on the new kernel and with impl="generic"
BANKS = {
    "htk23": _htk(23, 20, 8000),
    "htk40": _htk(40, 20, 8000),
    "htk64_vggish": _htk(64, 125, 7500),
    "htk64": _htk(64, 0, 8000),
    "htk32": _htk(32, 0, 8000),
    "htk16": _htk(16, 0, 8000),
    "htk40_8k": _htk(40, 0, 4000, 8000),
    "htk23_48k": _htk(23, 20, 24000, 48000),
}
G800 = dict(nfft=1024, hop=320, win_length=800, nfilters=40, nceptrums=13, power_scale=0, mel="htk", fmin=20, fmax=None)
SHAPES = [(b, k) for b in BANKS for k in (NEW, GENERIC)] + [("g800", GENERIC)]


def _shape(bank, kernel):
    kw = dict(G800) if bank == "g800" else dict(BANKS[bank])
    if kernel == GENERIC and bank != "g800":
        kw["impl"] = "generic"
    return kw


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
                n_cep=kw["nceptrums"], low=float(kw["fmin"]), high=kw["fmax"], lifter=float(kw.get("lifter", 0.0)))


_REFS = {}


def _reference(pcm, kw, kernel, pad, halo, output):
    """reference and bound of one channel; computed once per (samples, handle, model) and shared"""
    key = (pcm.tobytes(), tuple(sorted(_ref_kw(kw).items(), key=str)), MODEL[kernel], pad, halo, output)
    if key not in _REFS:
        ref, bound = mr.reference_and_bound(pcm, MODEL[kernel], pad_mode=pad, halo=halo, output=output, **_ref_kw(kw))
        ref.setflags(write=False)
        bound.setflags(write=False)
        _REFS[key] = (ref, bound)
    return _REFS[key]


def _check(got, pcm, kw, kernel, pad="notebook", halo=0, what="", output="cepstra", all_bounded=False):
    """every value of every frame of every channel against melbank_ref; no frame is set aside (``all_bounded``: and the
    reference must bound every frame, or pin its -inf / NaN pattern)"""
    got, pcm = as_np(got), np.asarray(pcm)
    if pcm.ndim == 1:
        got, pcm = got[None], pcm[None]
    worst = 0.0
    for c in range(len(pcm)):
        ref, bound = _reference(pcm[c], kw, kernel, pad, halo, output)
        if all_bounded:
            assert not np.isposinf(bound).any(), "%s channel %d: the reference leaves frames unbounded" % (what, c)
        worst = max(worst, mr.check(got[c], ref, bound, "%s channel %d" % (what, c)))
    return worst


# ------------------------------------------------------------------------------------------------ both kernels

@pytest.mark.parametrize("bank,kernel", SHAPES)
def test_both_kernels_meet_the_banked_reference(mfcc_amd, wav_pcm, bank, kernel):
    """The six kinds of channel at seed 3, 48 frames each, every coefficient of every frame."""
    kw = _shape(bank, kernel)
    L, hop = kw["win_length"], kw["hop"]
    n = 47 * hop + L + 5
    pcm = kf.channels(n, 3, wav_pcm)
    with _open(mfcc_amd, kw, kernel) as m:
        assert (m.mel, m.fmin) == ("htk", float(kw["fmin"])) and m.fmax == float(kw["fmax"] or m.samplerate / 2)
        assert m.win_length == L and m.num_frames(n) == 48
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 48, 13)
        worst = _check(got, pcm, kw, kernel, what=bank, all_bounded=True)
    # exactly the all-zero frames of `silences` are left as a -inf / NaN pattern: 16 of them at 400 / 160
    got = as_np(got)
    open_rows = ~np.isfinite(got).all(axis=2)
    silent = list(kf.KINDS).index("silences")
    assert open_rows.sum() == open_rows[silent].sum() == (11 if bank == "g800" else 16)
    print("%s on %s: worst error / bound %.3f" % (bank, kernel, worst))


@pytest.mark.parametrize("bank,kernel", SHAPES)
def test_log_mel_rows_meet_the_banked_reference(mfcc_amd, wav_pcm, bank, kernel):
    kw = _shape(bank, kernel)
    L, hop = kw["win_length"], kw["hop"]
    n = 47 * hop + L + 5
    pcm = kf.channels(n, 3, wav_pcm)
    with _open(mfcc_amd, kw, kernel, output="logmel") as m:
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 48, kw["nfilters"]) and m.num_features == kw["nfilters"]
        worst = _check(got, pcm, kw, kernel, what=bank + " logmel", output="logmel", all_bounded=True)
    print("%s log-mel on %s: worst error / bound %.3f" % (bank, kernel, worst))


# ------------------------------------------------------------------------------------------------ edges, new kernel

@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("bank", ["htk40", "htk64"])
def test_tile_and_buffer_edges_of_the_new_kernel(mfcc_amd, wav_pcm, bank, pad, halo):
    """Frame counts around a tile, 1 and 6 channels, odd and even channel strides; the tensor ends with the last
    channel's last sample, so the last frame's samples L .. 511 lie past the end of the buffer.  40 filters: a padded
    block; 64: all four."""
    import torch
    kw = BANKS[bank]
    with _open(mfcc_amd, kw, NEW, pad_mode=pad) as m:
        for nfr in (1, 15, 16, 17, 33):
            n = _length(nfr, pad)
            assert m.num_frames(n) == nfr
            for nch in (1, 6):
                pcm = kf.channels(n + halo, 10 * nfr + nch, wav_pcm)[:nch]
                dense = as_np(m.process(_dev(pcm), halo=halo))
                assert dense.shape == (nch, nfr, 13)
                _check(dense, pcm, kw, NEW, pad, halo, "%d frames, %d channels" % (nfr, nch))
                for extra in (1, 2, 3):                                  # strides n + halo + extra: odd and even
                    stride = n + halo + extra
                    flat = np.zeros(stride * (nch - 1) + n + halo, np.int16)
                    for c in range(nch):
                        flat[c * stride: c * stride + n + halo] = pcm[c]
                    view = torch.as_strided(_dev(flat), (nch, n + halo), (stride, 1))
                    assert same(m.process(view, halo=halo), dense), (nfr, nch, stride)


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
@pytest.mark.parametrize("bank", ["htk40", "htk64", "htk23"])
def test_a_frame_does_not_depend_on_its_tile(mfcc_amd, wav_pcm, bank, output):
    """k hops of other samples in front: frame f becomes frame f + k, other tile, other neighbours, the same bits; a
    silent frame's -inf stays in its own row."""
    hop, L = 160, 400
    x = kf.signal("noise", hop * 40 + L, 77, wav_pcm)
    x[hop * 10: hop * 10 + 3 * L] = 0
    pre = kf.signal("uniform", hop * 17, 78, wav_pcm)
    with _open(mfcc_amd, BANKS[bank], NEW, output=output) as m:
        a = as_np(m.process(_dev(x)))
        assert a.shape[1] == m.num_features
        silent = np.isneginf(a[:, 0])
        assert silent.sum() >= 3 and np.isfinite(a[~silent]).all()
        if output == "logmel":
            assert np.isneginf(a[silent]).all()
        for k in (1, 5, 15, 16, 17):
            b = as_np(m.process(_dev(np.concatenate([pre[:k * hop], x]))))
            assert same(a[1:], b[k + 1:]), k


# ------------------------------------------------------------------------------------------------ the accepted range

LENGTHS = [160, 161, 255, 511]                     # the ends of mfcc_fused160mb::supported, one off, and an odd middle


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("L", LENGTHS)
def test_frame_lengths_of_the_accepted_range(mfcc_amd, wav_pcm, L, pad):
    """The six kinds at 37 frames, every coefficient of every frame bounded; then 1, 16 and 17 frames in a tensor that
    ends with the last channel's last sample, so slots L .. 511 of the last frame lie past the end of the buffer (352
    samples at L = 160)."""
    kw = dict(BANKS["htk40"], win_length=L)
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
    print("htk40, L %d, %s: worst error / bound %.3f" % (L, pad, worst))


@pytest.mark.parametrize("n_cep,lifter", [(1, 0.0), (16, 0.0), (13, 22.0), (16, 22.0)])
def test_cepstra_counts_and_the_lifter(mfcc_amd, wav_pcm, n_cep, lifter):
    kw = dict(BANKS["htk40"], nceptrums=n_cep, lifter=lifter)
    n = _length(37, "notebook")
    pcm = kf.channels(n, 7, wav_pcm)
    with _open(mfcc_amd, kw, NEW) as m:
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 37, n_cep)
        worst = _check(got, pcm, kw, NEW, what="%d cepstra, lifter %g" % (n_cep, lifter), all_bounded=True)
    print("htk40, %d cepstra, lifter %g: worst error / bound %.3f" % (n_cep, lifter, worst))


def test_log_mel_rows_of_a_handle_with_32_cepstra(mfcc_amd, wav_pcm):
    """nceptrums above the DCT's 16 is accepted for log-mel rows, which do not pass the DCT."""
    kw = dict(BANKS["htk40"], nceptrums=32)
    n = _length(37, "notebook")
    pcm = kf.channels(n, 7, wav_pcm)
    with _open(mfcc_amd, kw, NEW, output="logmel") as m:
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 37, 40) and m.num_features == 40
        _check(got, pcm, kw, NEW, what="log-mel at 32 cepstra", output="logmel", all_bounded=True)
    with _open(mfcc_amd, BANKS["htk40"], NEW, output="logmel") as m:
        assert same(m.process(_dev(pcm)), got)                           # the rows do not depend on nceptrums


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
@pytest.mark.parametrize("kernel", [NEW, GENERIC])
@pytest.mark.parametrize("bank", list(kf.MASK_BANKS))
def test_every_set_mask(mfcc_amd, wav_pcm, bank, kernel, output):
    """kernel_families.MASK_BANKS: no set at all, one K group only, a last block of one filter, three and four blocks
    (tests/test_fused512_tables_host.py proves the masks without a GPU); the generic kernel of the same handle under its
    own model."""
    n_mel, fmin, fmax, rate, _ = kf.MASK_BANKS[bank]
    kw = _htk(n_mel, fmin, fmax, rate, nceptrums=min(13, n_mel))
    if kernel == GENERIC:
        kw["impl"] = "generic"
    n = _length(37, "notebook")
    pcm = kf.channels(n, 7, wav_pcm)
    with _open(mfcc_amd, kw, kernel, output=output) as m:
        got = m.process(_dev(pcm))
        assert tuple(got.shape) == (len(kf.KINDS), 37, n_mel if output == "logmel" else min(13, n_mel))
        worst = _check(got, pcm, kw, kernel, what="%s %s" % (bank, output), output=output, all_bounded=True)
    print("%s %s on %s: worst error / bound %.3f" % (bank, output, kernel, worst))


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("L", [160, 511])
def test_sessions_and_banks_at_the_ends_of_the_frame_lengths(mfcc_amd, wav_pcm, L, pad):
    """A session fed in uneven chunks and flushed, and a raw bank of 4, equal the dense call bit for bit.  L = hop: a
    line never holds a whole hop of history behind the frames it has produced."""
    kw = dict(BANKS["htk40"], win_length=L)
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
@pytest.mark.parametrize("bank", ["htk40", "htk64"])
def test_every_float_entry_point_equals_the_dense_device_call(mfcc_amd, wav_pcm, bank, pad):
    import torch
    kw = BANKS[bank]
    L, hop = kw["win_length"], kw["hop"]
    n = 36 * hop + L + 7
    pcm = kf.channels(n, 11, wav_pcm, kinds=("speech", "noise", "silences", "uniform"))
    with _open(mfcc_amd, kw, NEW, pad_mode=pad) as m:
        R = as_np(m.process(_dev(pcm)))
        nf = m.num_frames(n)
        assert R.shape == (4, nf, 13)
        _check(R, pcm, kw, NEW, pad, what=bank)
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
            assert same(host[i], o), (bank, pad, "host", i)
            assert same(dev[i], o), (bank, pad, "device", i)
            assert same(packed[int(fo[i]):int(fo[i + 1])], o), (bank, pad, "packed", i)
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
            assert same(np.concatenate(rows), R[0]), (bank, pad, "session")
        # a raw bank of 4 with uneven chunks, some of them empty
        sizes = [(1, 159, 160, 161, 1000), (0, 700, 0, 33), (2048,), (399, 0, 1, 160)]
        with m.stream_bank(4) as b:
            rows = _feed(b, pcm, sizes, L)
            for u in range(4):
                assert same(rows[u], R[u]), (bank, pad, "bank", u)
    # an online bank equals the dense call of a handle with the same causal settings
    online = dict(normalize="meanvar", normalize_window=600, deltas=2)
    with _open(mfcc_amd, kw, NEW, pad_mode=pad, normalize_min_window=1, normalize_center=False, **online) as mo:
        Ro = as_np(mo.process(_dev(pcm)))
    with _open(mfcc_amd, kw, NEW, pad_mode=pad) as m, m.stream_bank(4, **online) as b:
        rows = _feed(b, pcm, sizes, L)
        for u in range(4):
            assert same(rows[u], Ro[u]), (bank, pad, "online bank", u)


@pytest.mark.parametrize("bank", ["htk40", "htk64"])
def test_dist_frame_shards_of_an_htk_handle_concatenate_to_the_one_call(mfcc_amd, wav_pcm, bank):
    from mfcc_amd import dist as md
    pcm = kf.signal("speech", _length(16 * 3 + 5, "notebook") + 53, 31, wav_pcm)
    with _open(mfcc_amd, BANKS[bank], NEW) as m:
        R = as_np(m.process(_dev(pcm)))
        nf = m.num_frames(len(pcm))
        compute = md.mfcc_compute(m)
        for world in (2, 3):
            parts = [md.process_frames_sharded(compute, pcm, rank, world, 13, n_frames=nf)[1] for rank in range(world)]
            assert same(np.concatenate(parts), R), (bank, world)


def test_post_passes_on_64_wide_rows_equal_the_direct_entries(mfcc_amd, wav_pcm):
    import torch
    hop, L = 160, 400
    kw = dict(BANKS["htk64"], output="logmel")
    utts = [kf.signal(k, hop * f + L + 3, 40 + i, wav_pcm)
            for i, (k, f) in enumerate((("speech", 70), ("silences", 33), ("noise", 16), ("speech", 1)))]
    devs = [_dev(u) for u in utts]
    with _open(mfcc_amd, kw, NEW) as m:
        assert m.num_features == 64
        raw = m.process_batch(devs)
        assert [tuple(r.shape) for r in raw] == [(f, 64) for f in (71, 34, 17, 2)]
        for u, r in zip(utts, raw):
            _check(r, u, kw, NEW, what="logmel", output="logmel")
        fo = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64)
        rows = torch.cat(list(raw))
        with _open(mfcc_amd, kw, NEW, normalize="meanvar") as mn:
            assert same(torch.cat(list(mn.process_batch(devs))), m.normalize_rows(rows.clone(), fo, mode="meanvar"))
        with _open(mfcc_amd, kw, NEW, normalize="mean", normalize_window=30) as ms:
            assert same(torch.cat(list(ms.process_batch(devs))), m.normalize_rows(rows.clone(), fo, mode="mean", window=30))
        with _open(mfcc_amd, kw, NEW, deltas=2) as md:
            assert md.num_features == 192
            assert same(torch.cat(list(md.process_batch(devs))), m.deltas_rows(rows, fo, order=2))
        # band 0 against its own mean (the default threshold is meant for C0: no log-mel band of this input passes it)
        with _open(mfcc_amd, kw, NEW, vad="select", vad_energy_threshold=0.0, vad_energy_mean_scale=1.0) as mv:
            sel = mv.process_batch(devs)
            voiced = m.vad_rows(rows, fo, energy_threshold=0.0, energy_mean_scale=1.0)
            picked, so = m.select_rows(rows, voiced, fo)
            assert [len(s) for s in sel] == np.diff(so.astype(np.int64)).tolist()
            assert same(torch.cat(list(sel)), picked)
            assert 0 < len(picked) <= len(rows)


# ------------------------------------------------------------------------------------------------ selection, refusals

def test_selection_on_an_htk_handle(mfcc_amd):
    # the covered range: frame lengths 160 .. 511, 1 .. 64 filters, any rate; cepstra up to 16, log-mel rows of any width
    for kw in (_htk(40, 20, 8000, win_length=160), _htk(40, 20, 8000, win_length=511), _htk(1, 0, 8000, nceptrums=1),
               _htk(17, 300, 3400, 8000), _htk(64, 0, None, 44100), _htk(64, 0, 8000, nceptrums=16),
               _htk(40, 20, 8000, nceptrums=32, output="logmel"), _htk(40, 20, 8000, impl="fused512")):
        with mfcc_amd.MFCC(**kw) as m:
            assert m.kernel_name() == NEW, kw
        with mfcc_amd.MFCC(**dict(kw, impl="generic")) as m:
            assert m.kernel_name() == GENERIC, kw
    # outside it AUTO runs the generic kernel and FUSED512 is refused: more than 16 cepstra, other hops, frame lengths
    # and transform sizes -- the 512 / 170 and 1024 / 341 shapes of the other fused forms among them
    for kw in (_htk(40, 20, 8000, nceptrums=17), _htk(40, 20, 8000, hop=170), _htk(40, 20, 8000, win_length=512),
               dict(nfft=512, nfilters=32, nceptrums=13, mel="htk"), dict(nfft=512, nfilters=16, nceptrums=16, mel="htk"),
               dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0, mel="htk", fmin=20), dict(G800)):
        with mfcc_amd.MFCC(**kw) as m:
            assert m.kernel_name() == GENERIC and m.mel == "htk", kw
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            mfcc_amd.MFCC(**dict(kw, impl="fused512"))
        assert e.value.code == mfcc_amd._lib.ERROR_UNSUPPORTED, kw


def test_the_fixed_path_refuses_an_htk_handle(mfcc_amd, wav_pcm, golden_dir, tmp_path):
    import os
    import torch
    U = mfcc_amd._lib.ERROR_UNSUPPORTED
    x = kf.signal("speech", 4000, 1, wav_pcm)
    offs = np.array([0, 2000, 4000], np.uint64)
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    # 512 / 170 / 32: the fixed path's own shape, refused only because of the bank
    for kw in (dict(nfft=512, nfilters=32, nceptrums=13, mel="htk"), dict(BANKS["htk40"])):
        with mfcc_amd.MFCC(**kw) as m:
            assert m.kernel_name(fixed=False) in (NEW, GENERIC)
            out = torch.empty((1, 64, 13), device="cuda", dtype=torch.int16)
            calls = [lambda: m.process_fixed(x), lambda: m.process_fixed(_dev(x)), lambda: m.process_fixed(_dev(x), halo=1),
                     lambda: m.process_batch([x, x], fixed=True), lambda: m.process_batch([_dev(x), _dev(x[:3000])], fixed=True),
                     lambda: m.process_packed(_dev(x), offs, fixed=True),
                     lambda: m.time_launches(_dev(x), out, fixed=True), lambda: m.stream(fixed=True),
                     lambda: m.stream_bank(3, fixed=True), lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=True),
                     lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=True)]
            for i, call in enumerate(calls):
                with pytest.raises(mfcc_amd.MfccHipError) as e:
                    call()
                assert e.value.code == U, (kw, i)
            assert len(m.process(x)) == m.num_frames(len(x))             # the float path of the same handle works


def test_notebook_bank_handles_are_unchanged(mfcc_amd, wav_pcm):
    """A notebook-bank framed handle and a plain handle report the kernels they reported before and return the bits of
    ``bank = NULL`` (mfcc_hip_create_framed), whether the bank is left out or spelled out."""
    import ctypes as C
    import torch
    L = mfcc_amd._lib
    lib = L.load()
    x = _dev(kf.channels(170 * 40 + 512 + 3, 9, wav_pcm))
    cases = [(dict(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=13), H160),
             (dict(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13), GENERIC),   # 40 notebook filters
             (dict(nfft=512, nfilters=32, nceptrums=13), "mfcc_fused512_w12_kernel"),
             (dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0), "mfcc_fused1024_w12bf_kernel")]
    for kw, kernel in cases:
        with mfcc_amd.MFCC(**kw) as m, mfcc_amd.MFCC(**dict(kw, mel="notebook", fmin=0.0, fmax=None)) as w:
            assert m.kernel_name() == w.kernel_name() == kernel and (m.mel, m.fmin) == ("notebook", 0.0)
            a = m.process(x)
            assert same(w.process(x), a)
            # the handle mfcc_hip_create_framed makes, driven through the C ABI
            h = C.c_void_p()
            L.check(lib.mfcc_hip_create_framed(C.byref(m._params), m.win_length, C.byref(h)))
            try:
                assert lib.mfcc_hip_kernel_name(h, 0).decode() == kernel
                bank = L.MelBank()
                L.check(lib.mfcc_hip_mel_bank_of(h, C.byref(bank)))
                assert (bank.struct_size, bank.kind, bank.low_hz, bank.high_hz) == (32, L.MEL_NOTEBOOK, 0.0, 0.0)
                out = torch.empty_like(a)
                nf = C.c_size_t(0)
                L.check(lib.mfcc_hip_process_i16_dev(h, x.data_ptr(), x.shape[1], x.stride(0), x.shape[0], 0,
                                                     out.data_ptr(), C.byref(nf)))
                L.check(lib.mfcc_hip_synchronize(h))
                assert nf.value == a.shape[1] and same(out, a)
            finally:
                lib.mfcc_hip_destroy(h)
    with mfcc_amd.MFCC(**BANKS["htk64_vggish"]) as m:
        bank = L.MelBank()
        L.check(lib.mfcc_hip_mel_bank_of(m._h, C.byref(bank)))
        assert (bank.kind, bank.low_hz, bank.high_hz) == (L.MEL_HTK, 125.0, 7500.0)
    with mfcc_amd.MFCC(**BANKS["htk23_48k"]) as m:
        L.check(lib.mfcc_hip_mel_bank_of(m._h, C.byref(bank)))
        assert (bank.kind, bank.low_hz, bank.high_hz) == (L.MEL_HTK, 20.0, 24000.0) and m.fmax == 24000.0
    # edges fp32 does not hold exactly: the attributes are the edges of the bank that was built
    with mfcc_amd.MFCC(**_htk(40, 20.1, 7600.3)) as m:
        L.check(lib.mfcc_hip_mel_bank_of(m._h, C.byref(bank)))
        assert (m.fmin, m.fmax) == (bank.low_hz, bank.high_hz) == (float(np.float32(20.1)), float(np.float32(7600.3)))
