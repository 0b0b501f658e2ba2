"""Sample formats on the GPU (``mfcc_hip_decode_dev``, ``mfcc_hip_set_sample_format``, ``MFCC(sample_format=...)``).

* D  the kernel against ``mfcc_hip_decode_host``, bit for bit: every format, lengths around the group of 8 and the
     workgroup, every input offset 0..7 samples and every output offset 0..7 int16 (head, tail, the narrow-load
     fallback, a length shorter than the head), a length that takes the grid-stride loop round twice, sentinels around
     every output, inputs that end at the last byte of their allocation;
* R  what the direct entry refuses;
* E  every entry point of a handle with a format against the S16 handle on the decoded samples;
* S  sessions and banks; the setter is BUSY while one lives;
* M  the scratch area growing and shrinking between calls; S16 untouched.

Everything is ``array_equal``: there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as dr
from kernel_families import same
from oracle.mfcc_float import synth_pcm

pytestmark = pytest.mark.gpu

FORMATS = list(dr.FORMATS)
CODED = [f for f in FORMATS if f != "s16"]
SENTINEL = 0x5a5a
GUARD = 32                                  # int16: 64 bytes on each side of every output
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 1027, 70001]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


@pytest.fixture(scope="module")
def handle(mfcc_amd):
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        yield m


def raw_samples(fmt, n, seed):
    """n random samples of the format as a NumPy array: every byte / word value, floats beyond +-1 with ties, NaN and
    infinities among them."""
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        return rng.integers(-32768, 32768, size=n).astype(np.int16)
    if dr.SIZES[fmt] == 1:
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    if fmt != "f32":
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    x = rng.uniform(-1.2, 1.2, size=n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, -2.5 / 32768, 1.0, -1.0, -0.0, 1e-45], np.float32)
    k = min(n, len(special))
    if k:
        x[rng.choice(n, size=k, replace=False)] = special[:k]
    return x


def decode_dev_into(mfcc_amd, handle, fmt, p_in, n, arena, at):
    """mfcc_hip_decode_dev of the n samples at device address p_in to arena[at : at + n], on the current torch stream."""
    from mfcc_amd import _lib as L
    with handle._on_torch_stream(arena.device):
        rc = L.load().mfcc_hip_decode_dev(handle._h, dr.CODES[fmt], C.c_void_p(p_in), n,
                                          C.c_void_p(arena.data_ptr() + 2 * at))
    assert rc == 0, (fmt, n, at, rc)


def check_lengths(mfcc_amd, handle, fmt, lengths, in_offsets, out_offsets, seed):
    import torch
    for n in lengths:
        src = raw_samples(fmt, n + 8, seed + n)
        slot = (2 * GUARD + 8 + n + 7) // 8 * 8                  # a multiple of 8 int16: every slot starts 16-byte aligned
        for io in in_offsets:
            x = src[io:io + n]
            want = mfcc_amd.decode(x, fmt)                       # mfcc_hip_decode_host
            # the input allocated exactly: io samples of slack in front, the run ends at the tensor's last byte
            t = torch.from_numpy(src[:io + n].copy()).cuda()
            assert t.numel() == io + n
            t_in = t.data_ptr() + io * dr.SIZES[fmt]             # (a slice of no element has no address in torch)
            arena = torch.full((slot * len(out_offsets),), SENTINEL, dtype=torch.int16, device="cuda")
            assert arena.data_ptr() % 16 == 0
            for k, oo in enumerate(out_offsets):
                decode_dev_into(mfcc_amd, handle, fmt, t_in, n, arena, k * slot + GUARD + oo)
            got = arena.cpu().numpy().reshape(len(out_offsets), slot)
            for k, oo in enumerate(out_offsets):
                a = GUARD + oo
                assert np.array_equal(got[k, a:a + n], want), (fmt, n, io, oo)
                assert np.all(got[k, :a] == SENTINEL) and np.all(got[k, a + n:] == SENTINEL), (fmt, n, io, oo)


# ------------------------------------------------------------------------------------------------ D

@pytest.mark.parametrize("fmt", FORMATS)
def test_direct_entry_every_length_and_alignment(mfcc_amd, handle, fmt):
    check_lengths(mfcc_amd, handle, fmt, LENGTHS, range(8), range(8), seed=100 * dr.CODES[fmt])


def one_trip_samples():
    """Samples one trip of the decode grid covers on this GPU (mfcc_fc::decode_grid: 8 workgroups of 256 lanes per CU,
    8 samples per lane; tests/test_decode_host.py holds the rule)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 * 8


@pytest.mark.parametrize("fmt", CODED)
def test_direct_entry_second_trip_of_the_grid(mfcc_amd, handle, fmt):
    """70 001 samples fit one trip of a grid sized from the CU count on any GPU with more than four CUs: the next length
    that goes round twice is one trip plus that."""
    trip = one_trip_samples()
    n = 70001 if 70001 > trip + 16 else trip + 70001
    assert (n - 7) // 8 > trip // 8
    check_lengths(mfcc_amd, handle, fmt, [n], [0, 1], [0, 3], seed=7)


# ------------------------------------------------------------------------------------------------ R

def test_direct_entry_refusals(mfcc_amd, handle):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    INV = L.ERROR_INVALID_PARAM
    buf = torch.full((4096,), SENTINEL, dtype=torch.int16, device="cuda")
    base = buf.data_ptr()

    def call(fmt, p_in, n, p_out, h=handle._h):
        return lib.mfcc_hip_decode_dev(h, fmt, C.c_void_p(p_in), n, C.c_void_p(p_out))
    # overlapping ranges, either way round, by one byte
    assert call(L.SAMPLE_ULAW, base, 100, base) == INV
    assert call(L.SAMPLE_ULAW, base + 199, 100, base) == INV
    assert call(L.SAMPLE_S32, base, 100, base + 398) == INV
    assert call(L.SAMPLE_S16, base, 100, base + 198) == INV
    # a misaligned pointer of a 4-byte format, a misaligned output
    for f in (L.SAMPLE_I2S32, L.SAMPLE_S32, L.SAMPLE_F32):
        for off in (1, 2, 3):
            assert call(f, base + 4096 + off, 10, base) == INV, (f, off)
    assert call(L.SAMPLE_ULAW, base + 4096, 10, base + 1) == INV
    # an unknown format, NULL pointers, no handle
    assert call(7, base + 4096, 10, base) == INV and call(-1, base + 4096, 10, base) == INV
    assert call(L.SAMPLE_ULAW, 0, 10, base) == INV and call(L.SAMPLE_ULAW, base + 4096, 10, 0) == INV
    assert call(L.SAMPLE_ULAW, base + 4096, 10, base, h=None) == INV
    # n = 0 looks at no pointer
    assert call(L.SAMPLE_F32, 0, 0, 0) == L.SUCCESS
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    # ... and ranges that touch without overlapping are taken
    with handle._on_torch_stream(buf.device):
        assert call(L.SAMPLE_ULAW, base + 200, 100, base) == L.SUCCESS
    # the Python entry
    x = torch.from_numpy(raw_samples("alaw", 1000, 1)).cuda()
    assert same(mfcc_amd.decode(x, "alaw"), dr.decode(x.cpu().numpy(), "alaw"))
    assert same(mfcc_amd.decode(x.view(10, 100), "alaw", mfcc=handle), dr.decode(x.cpu().numpy(), "alaw").reshape(10, 100))
    with pytest.raises(TypeError):
        mfcc_amd.decode(x, "f32")


# ------------------------------------------------------------------------------------------------ E

CONFIGS = {
    "headline": dict(nfft=512, hop=170, nfilters=32, nceptrums=13),
    "fixed": dict(nfft=512, nfilters=16, nceptrums=16),
    "htk": dict(nfft=512, hop=160, win_length=400, nfilters=23, nceptrums=13, mel="htk", fmin=20),
    "cmvn_dd": dict(nfft=512, nfilters=32, nceptrums=13, normalize="meanvar", deltas=2),
}


@pytest.fixture(scope="module")
def twins(mfcc_amd):
    """The S16 handle of every configuration, made once."""
    made = {k: mfcc_amd.MFCC(**kw) for k, kw in CONFIGS.items()}
    yield made
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def coded(mfcc_amd):
    """Two channels of 2000 samples in every format, and what they decode to (host rules, checked against the reference)."""
    pcm = synth_pcm(4000, seed=11).reshape(2, 2000)
    rng = np.random.default_rng(12)
    out = {}
    for f in CODED:
        raw = dr.encode_like(pcm, f, rng)
        dec = mfcc_amd.decode(raw, f)
        assert np.array_equal(dec, dr.decode(raw, f))
        if f not in ("ulaw", "alaw", "u8"):
            assert np.array_equal(dec, pcm)
        out[f] = (raw, dec)
    return out


def strided(torch, a, pad=24):
    """(channels, n) on the device with a channel stride of n + pad samples."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    buf[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    t = buf[:, :a.shape[1]]
    assert t.stride(0) == a.shape[1] + pad and t.stride(1) == 1
    return t


@pytest.mark.parametrize("fmt", CODED)
def test_dense_device_call_with_halo_and_stride(mfcc_amd, twins, coded, fmt):
    import torch
    raw, dec = coded[fmt]
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["headline"]) as m:
        assert m.kernel_name() == twins["headline"].kernel_name() == "mfcc_fused512_w12_kernel"
        for halo in (1, 0):
            got = m.process(strided(torch, raw), halo=halo)
            want = twins["headline"].process(strided(torch, dec), halo=halo)
            assert got.shape[1] > 0 and same(got, want), (fmt, halo)
        # one channel, a pointer that is aligned to the sample size and to nothing more
        got = m.process(strided(torch, raw)[1, 1:])
        assert same(got, twins["headline"].process(torch.from_numpy(dec[1, 1:].copy()).cuda()))
        with pytest.raises(TypeError):
            m.process(torch.from_numpy(dec).cuda())


@pytest.mark.parametrize("fmt", CODED)
def test_process_fixed(mfcc_amd, twins, coded, fmt):
    import torch
    raw, dec = coded[fmt]
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["fixed"]) as m:
        want = twins["fixed"].process_fixed(dec)
        assert want.dtype == np.int16 and want.shape[1] > 0
        assert same(m.process_fixed(raw), want)
        assert same(m.process_fixed(torch.from_numpy(raw).cuda()), want)
        assert same(m.process_fixed(strided(torch, raw), halo=1), twins["fixed"].process_fixed(strided(torch, dec), halo=1))


@pytest.mark.parametrize("fmt", CODED)
def test_framed_htk_handle(mfcc_amd, twins, coded, fmt):
    import torch
    raw, dec = coded[fmt]
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["htk"]) as m:
        assert m.kernel_name() == twins["htk"].kernel_name() == "mfcc_fused512_h160_mb_kernel"
        assert same(m.process(torch.from_numpy(raw).cuda()), twins["htk"].process(torch.from_numpy(dec).cuda()))
        assert same(m.process(raw), twins["htk"].process(dec))


@pytest.mark.parametrize("fmt", CODED)
def test_batch_with_normalization_and_deltas(mfcc_amd, twins, coded, fmt):
    import torch
    raw, dec = coded[fmt]
    lens = [0, 511, 512, 1300]
    cut = lambda a: [a.reshape(-1)[sum(lens[:i]) + 7:sum(lens[:i]) + 7 + n].copy() for i, n in enumerate(lens)]
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["cmvn_dd"]) as m:
        want = twins["cmvn_dd"].process_batch(cut(dec))
        assert [len(w) for w in want] == [0, 0, 1, 5] and want[3].shape[1] == 39
        for got in (m.process_batch(cut(raw)), m.process_batch([torch.from_numpy(u).cuda() for u in cut(raw)])):
            assert len(got) == 4 and all(same(g, w) for g, w in zip(got, want)), fmt


@pytest.mark.parametrize("fmt", CODED)
def test_process_packed_and_host_process(mfcc_amd, twins, coded, fmt):
    import torch
    raw, dec = coded[fmt]
    offsets = np.array([3, 700, 700, 2100, 3999], dtype=np.uint64)            # one empty utterance, a start off 0
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["headline"]) as m:
        got, fo = m.process_packed(torch.from_numpy(raw.reshape(-1)).cuda(), offsets)
        want, wfo = twins["headline"].process_packed(torch.from_numpy(dec.reshape(-1)).cuda(), offsets)
        assert np.array_equal(fo, wfo) and int(fo[-1]) > 0 and same(got, want)
        # equal lengths: the ragged entry's multi-channel route
        got, fo = m.process_packed(torch.from_numpy(raw.reshape(-1)).cuda(), np.arange(5, dtype=np.uint64) * 1000)
        want, wfo = twins["headline"].process_packed(torch.from_numpy(dec.reshape(-1)).cuda(), np.arange(5, dtype=np.uint64) * 1000)
        assert np.array_equal(fo, wfo) and same(got, want)
        # host buffers: two channels, then one channel from a pointer off every alignment
        assert same(m.process(raw), twins["headline"].process(dec))
        assert same(m.process(raw[0, 5:]), twins["headline"].process(dec[0, 5:]))
        with pytest.raises(TypeError):
            m.process_packed(torch.from_numpy(dec.reshape(-1)).cuda(), offsets)


@pytest.mark.parametrize("fmt", ["ulaw", "f32"])
def test_host_buffers_through_the_chunked_copy_pipeline(mfcc_amd, twins, monkeypatch, fmt):
    """1 MB chunks (cut by sample count: 512 Ki samples): a long channel goes in frame ranges with a history sample in
    front, short channels two per chunk, utterances in groups -- every chunk's raw bytes are copied from the right
    place and decoded in front of its kernel.  With normalization and deltas the chunks fill one result on the device."""
    monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
    rng = np.random.default_rng(50)
    for cfg, shape in (("headline", (2, 1_300_001)), ("headline", (5, 200_003)), ("cmvn_dd", (2, 700_001)),
                       ("fixed", (1, 1_100_003))):
        pcm = synth_pcm(shape[0] * shape[1], seed=51).reshape(shape)
        raw = dr.encode_like(pcm, fmt, rng)
        dec = dr.decode(raw, fmt)
        run = (lambda m, x: m.process_fixed(x)) if cfg == "fixed" else (lambda m, x: m.process(x))
        with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS[cfg]) as m:
            got = run(m, raw)
        assert same(got, run(twins[cfg], dec)), (fmt, cfg, shape)
    lens = [300_000, 0, 700_001, 5, 400_000, 513]
    pcm = synth_pcm(sum(lens), seed=52)
    raw = dr.encode_like(pcm, fmt, rng)
    dec = dr.decode(raw, fmt)
    cut = lambda a: [a[sum(lens[:i]):sum(lens[:i + 1])] for i in range(len(lens))]
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["headline"]) as m:
        got = m.process_batch(cut(raw))
    want = twins["headline"].process_batch(cut(dec))
    assert [len(g) for g in got] == [len(w) for w in want] and all(same(g, w) for g, w in zip(got, want))


def test_misaligned_device_pointer_of_a_word_format_is_refused(mfcc_amd):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    x = torch.zeros(4000, dtype=torch.float32, device="cuda")
    out = torch.zeros((64, 13), dtype=torch.float32, device="cuda")
    nf = C.c_size_t(0)
    with mfcc_amd.MFCC(sample_format="f32", **CONFIGS["headline"]) as m:
        for off in (1, 2):
            assert lib.mfcc_hip_process_i16_dev(m._h, C.c_void_p(x.data_ptr() + off), 2000, 2000, 1, 0,
                                                C.c_void_p(out.data_ptr()), C.byref(nf)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_process_i16_dev(m._h, C.c_void_p(x.data_ptr() + 4), 2000, 2000, 1, 0,
                                            C.c_void_p(out.data_ptr()), C.byref(nf)) == L.SUCCESS
        m.synchronize()


# ------------------------------------------------------------------------------------------------ S

def test_stream_session_in_ulaw_chunks(mfcc_amd, twins, coded):
    raw, dec = coded["ulaw"]
    x, d = raw.reshape(-1), dec.reshape(-1)
    with mfcc_amd.MFCC(sample_format="ulaw", pad_mode="stream", **CONFIGS["headline"]) as m, \
            mfcc_amd.MFCC(pad_mode="stream", **CONFIGS["headline"]) as m16:
        want = m16.process(d[:3000])
        assert same(m.process(x[:3000]), want)
        for chunk in (1, 169, 170, 700):
            with m.stream() as s:
                rows = [s.push(x[a:min(a + chunk, 3000)]) for a in range(0, 3000, chunk)]
                rows.append(s.flush())
                assert same(np.concatenate(rows), want), chunk
                with pytest.raises(TypeError):
                    s.push(d[:10])
        with m.stream(fixed=True) as s, m16.stream(fixed=True) as s16:
            assert same(np.concatenate([s.push(x[:999]), s.push(x[999:2000]), s.flush()]),
                        np.concatenate([s16.push(d[:999]), s16.push(d[999:2000]), s16.flush()]))


PUSHES = [(700, 170, 0), (1, 600, 512), (1299, 730, 0)]                       # one empty line in the first and the last


def _lines(a):
    """The three lines' whole signals and their chunks, cut out of a flat array."""
    a = a.reshape(-1)
    starts, lines = [0, 2000, 3488], []
    for u in range(3):
        at, chunks = starts[u], []
        for p in PUSHES:
            chunks.append(a[at:at + p[u]].copy())
            at += p[u]
        lines.append(chunks)
    return lines


@pytest.mark.parametrize("fmt", ["ulaw", "f32", "i2s32"])
def test_stream_bank_mixed_chunks(mfcc_amd, twins, coded, fmt):
    import torch
    raw, dec = coded[fmt]
    lr, ld = _lines(raw), _lines(dec)
    want = [twins["headline"].process(np.concatenate(ld[u])) for u in range(3)]
    assert [len(w) for w in want] == [9, 6, 1]
    with mfcc_amd.MFCC(sample_format=fmt, **CONFIGS["headline"]) as m:
        with m.stream_bank(3) as bank:
            got = [bank.push([lr[u][k] for u in range(3)]) for k in range(3)]
            for u in range(3):
                assert same(np.concatenate([g[u] for g in got]), want[u]), (fmt, u)
            with pytest.raises(TypeError):
                bank.push([ld[u][0] for u in range(3)])
        with m.stream_bank(3) as bank:
            rows = [[] for _ in range(3)]
            for k in range(3):
                chunks = [lr[u][k] for u in range(3)]
                offs = (np.concatenate([[0], np.cumsum([len(c) for c in chunks])]) + 5).astype(np.uint64)
                flat = torch.from_numpy(np.concatenate([raw.reshape(-1)[:5]] + chunks)).cuda()
                out, fo = bank.push_packed(flat, offs)
                for u in range(3):
                    rows[u].append(out[int(fo[u]):int(fo[u + 1])].cpu().numpy())
            for u in range(3):
                assert same(np.concatenate(rows[u]), want[u]), (fmt, u)


def test_online_bank_and_busy_setter(mfcc_amd, coded):
    from mfcc_amd import _lib as L
    raw, dec = coded["alaw"]
    lr, ld = _lines(raw), _lines(dec)
    cfg = dict(normalize="meanvar", normalize_window=50, deltas=1)
    with mfcc_amd.MFCC(normalize_min_window=1, normalize_center=False, pad_mode="stream", **cfg, **CONFIGS["headline"]) as one:
        want = [one.process(np.concatenate(ld[u])) for u in range(3)]
    with mfcc_amd.MFCC(sample_format="alaw", pad_mode="stream", **CONFIGS["headline"]) as m:
        bank = m.stream_bank(3, **cfg)
        got = [bank.push([lr[u][k] for u in range(3)]) for k in range(3)]
        tails = bank.flush()
        for u in range(3):
            assert same(np.concatenate([g[u] for g in got] + [tails[u]]), want[u]), u
        # the format cannot change under a live bank
        assert m._lib.mfcc_hip_set_sample_format(m._h, L.SAMPLE_F32) == L.ERROR_BUSY
        with pytest.raises(mfcc_amd.MfccHipError):
            m.set_sample_format("s16")
        assert m.sample_format == "alaw" and m._lib.mfcc_hip_sample_format(m._h) == L.SAMPLE_ALAW
        bank.close()
        assert m._lib.mfcc_hip_set_sample_format(m._h, 7) == L.ERROR_INVALID_PARAM
        m.set_sample_format("f32")
        assert m.sample_format == "f32" and m._lib.mfcc_hip_sample_format(m._h) == L.SAMPLE_F32
    assert L.load().mfcc_hip_set_sample_format(None, L.SAMPLE_S16) == L.ERROR_INVALID_PARAM
    assert L.load().mfcc_hip_sample_format(None) == L.SAMPLE_S16


# ------------------------------------------------------------------------------------------------ M

def test_scratch_area_is_reused_across_sizes_and_formats(mfcc_amd, twins):
    import torch
    rng = np.random.default_rng(21)
    with mfcc_amd.MFCC(**CONFIGS["headline"]) as m:
        for i, n in enumerate((65536, 600, 131072, 600, 65536)):
            fmt = ("ulaw", "f32")[i % 2]
            pcm = synth_pcm(n, seed=30 + i)
            raw = dr.encode_like(pcm, fmt, rng)
            dec = dr.decode(raw, fmt)
            m.set_sample_format(fmt)
            want = twins["headline"].process(torch.from_numpy(dec).cuda())
            assert same(m.process(torch.from_numpy(raw).cuda()), want), (i, fmt, n)
            assert same(m.process(raw), want.cpu().numpy()), (i, fmt, n)


def test_s16_is_untouched(mfcc_amd, twins):
    import torch
    from mfcc_amd import _lib as L
    pcm = synth_pcm(5000, seed=40)
    with mfcc_amd.MFCC(**CONFIGS["headline"]) as fresh:
        assert fresh.sample_format == "s16" and fresh._lib.mfcc_hip_sample_format(fresh._h) == L.SAMPLE_S16
        want = fresh.process(torch.from_numpy(pcm).cuda()).cpu().numpy()
        want_fixed = fresh.process_fixed(pcm)
        name = fresh.kernel_name()
    with mfcc_amd.MFCC(**CONFIGS["headline"]) as m:
        m.set_sample_format("ulaw")
        assert m.kernel_name() == name
        m.process(torch.zeros(5000, dtype=torch.uint8, device="cuda"))
        m.set_sample_format("s16")
        assert m._lib.mfcc_hip_sample_format(m._h) == L.SAMPLE_S16 and m.kernel_name() == name
        assert same(m.process(torch.from_numpy(pcm).cuda()), want)
        assert same(m.process(pcm), want) and same(m.process_fixed(pcm), want_fixed)
        with pytest.raises(TypeError):
            m.process(torch.zeros(5000, dtype=torch.uint8, device="cuda"))
