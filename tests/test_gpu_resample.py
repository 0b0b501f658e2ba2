"""Sample-rate conversion on the GPU.

K  the kernel (``mfcc_hip_resample_dev``) against ``mfcc_hip_resample_host`` bit for bit -- the host entry is held to the
   NumPy rule and the float64 design by tests/test_resample_host.py -- on every ratio of the list: output lengths around
   the lane's group of 8 and the workgroup's tile of 2048, every input offset against every output offset with sentinels
   on both sides of every output, a length that takes the grid loop round twice, the saturating input, and 16 : 1, which
   runs the unstaged kernel.
R  what the direct entry and ``mfcc_hip_set_input_rate`` refuse, BUSY and UNSUPPORTED.
E  every entry point of a handle with ``input_rate`` against the same handle without it on ``mfcc_amd.resample(x)``.
S  ``MFCC.resampler``: pushes plus flush against the one-shot result, its plan, reset, and composed with a bank.
M  the scratch area across sizes; a handle whose rate was cleared against a fresh one."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as rr
from kernel_families import same

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a
GUARD = 32                                  # int16: 64 bytes on each side of every output
TILE = 2048                                 # mfcc_rs::kTile
OK, INVALID, UNSUPPORTED, SMALL = 0, -101, -105, -106
UNSTAGED = (16000, 1000)                    # 16 : 1, K = 512: a tile's input does not fit the staging area
IDS = ["%d_%d" % r for r in rr.RATIOS]


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


def resample_dev_into(handle, ratio, p_in, n, arena, at, cap):
    """mfcc_hip_resample_dev of the n samples at device address p_in to arena[at : at + cap], on the current torch stream."""
    from mfcc_amd import _lib as L
    with handle._on_torch_stream(arena.device):
        return L.load().mfcc_hip_resample_dev(handle._h, ratio[0], ratio[1], C.c_void_p(p_in), n,
                                              C.c_void_p(arena.data_ptr() + 2 * at), cap)


def check(mfcc_amd, handle, ratio, src, n, in_offsets, out_offsets):
    """the n samples at src[io:] for every io, into every output offset: the host entry's bits, sentinels untouched"""
    import torch
    n_out = mfcc_amd.resample_count(n, *ratio)
    slot = (2 * GUARD + 8 + n_out + 7) // 8 * 8              # a multiple of 8 int16: every slot starts 16-byte aligned
    for io in in_offsets:
        want = mfcc_amd.resample(src[io:io + n], *ratio)     # mfcc_hip_resample_host
        assert want.shape == (n_out,)
        # the input allocated exactly: io samples of slack in front, the run ends at the tensor's last byte
        t = torch.from_numpy(src[:io + n].copy()).cuda() if io + n else torch.zeros(8, dtype=torch.int16, device="cuda")
        arena = torch.full((slot * len(out_offsets),), SENTINEL, dtype=torch.int16, device="cuda")
        assert arena.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
        for k, oo in enumerate(out_offsets):
            assert resample_dev_into(handle, ratio, t.data_ptr() + 2 * io, n, arena, k * slot + GUARD + oo, n_out) == OK
        got = arena.cpu().numpy().reshape(len(out_offsets), slot)
        for k, oo in enumerate(out_offsets):
            a = GUARD + oo
            assert np.array_equal(got[k, a:a + n_out], want), (ratio, n, io, oo)
            assert np.all(got[k, :a] == SENTINEL) and np.all(got[k, a + n_out:] == SENTINEL), (ratio, n, io, oo)


def lengths_of(ratio):
    """input lengths: 0, 1, H, K + 1, and the shortest with 7, 8, 9, a tile - 1, a tile, a tile + 1 and two tiles + 3
    outputs (an upsampling ratio reaches only every L / M-th count: then the next one above)"""
    L, M, H, K = rr.geometry(*ratio)
    return [0, 1, H, K + 1] + [-(-m * M // L) for m in (7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]


def samples(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


# ------------------------------------------------------------------------------------------------ K

@pytest.mark.parametrize("ratio", rr.RATIOS + [UNSTAGED], ids=IDS + ["unstaged_16_1"])
def test_kernel_every_length(mfcc_amd, handle, ratio):
    for n in lengths_of(ratio):
        check(mfcc_amd, handle, ratio, samples(n + 8, n), n, [0, 3], [0, 5])


@pytest.mark.parametrize("ratio", rr.RATIOS + [UNSTAGED], ids=IDS + ["unstaged_16_1"])
def test_kernel_every_alignment(mfcc_amd, handle, ratio):
    """input offsets 0 .. 7 against output offsets 0 .. 7 int16, on a tile and a bit"""
    L, M, H, K = rr.geometry(*ratio)
    n = -(-(TILE + 13) * M // L)
    check(mfcc_amd, handle, ratio, samples(n + 8, 99), n, range(8), range(8))


def test_kernel_second_trip_of_the_grid(mfcc_amd, handle):
    """70 001 outputs are 35 tiles, one trip of a grid of 8 workgroups per CU on any GPU with more than four CUs: so also
    one trip plus that."""
    import torch
    trip = torch.cuda.get_device_properties(0).multi_processor_count * 8 * TILE
    for ratio in [(48000, 16000), (8000, 16000)]:
        L, M, H, K = rr.geometry(*ratio)
        for outs in (70001, trip + 70001):
            n = -(-outs * M // L)
            assert mfcc_amd.resample_count(n, *ratio) >= outs
            check(mfcc_amd, handle, ratio, samples(n + 8, 7), n, [1], [3])


def test_kernel_rebinds_the_table(mfcc_amd, handle):
    """one call after another on changing ratios: the handle keeps the last table and
    rebinds it"""
    for ratio in [(8000, 16000), (44100, 16000), (8000, 16000), (7, 5)]:
        check(mfcc_amd, handle, ratio, samples(5000 + 8, 3), 5000, [2], [1])


@pytest.mark.parametrize("ratio", rr.RATIOS, ids=IDS)
def test_kernel_saturating_input(mfcc_amd, handle, ratio):
    """every output's worst input in turn is not one signal; this one drives phase p of a far output to -32768 sum|T|
    and its neighbours hard, with full-scale runs around it"""
    L, M, H, K = rr.geometry(*ratio)
    t = mfcc_amd.resample_taps(*ratio)
    n = -(-(TILE + 300) * M // L)
    x = np.where(np.arange(n) % (2 * H) < H, -32768, 32767).astype(np.int16)
    for m in (TILE - 1, TILE + 100):
        q, p = m * M // L, m * M % L
        x[q - H + 1:q + H + 1] = np.where(t[p] > 0, -32768, 32767)
    want = mfcc_amd.resample(x, *ratio)
    assert want[TILE - 1] == -32768 and want[TILE + 100] == -32768 and (want == 32767).any()
    check(mfcc_amd, handle, ratio, x, n, [0], [0, 1])


# ------------------------------------------------------------------------------------------------ R

def test_direct_entry_refusals(mfcc_amd, handle):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    buf = torch.full((4096,), SENTINEL, dtype=torch.int16, device="cuda")
    x = torch.zeros(1024, dtype=torch.int16, device="cuda")
    p, q = x.data_ptr(), buf.data_ptr()

    def call(i, o, p_in, n, p_out, cap, h=handle._h):
        return lib.mfcc_hip_resample_dev(h, i, o, C.c_void_p(p_in), n, C.c_void_p(p_out), cap)

    assert call(8000, 16000, p, 1024, q, 2048, h=None) == INVALID
    assert call(0, 16000, p, 1024, q, 2048) == INVALID and call(8000, -1, p, 1024, q, 2048) == INVALID
    assert call(16000, 16001, p, 1024, q, 4096) == UNSUPPORTED and call(1001, 1000, p, 1024, q, 4096) == UNSUPPORTED
    assert call(8000, 16000, p, 1024, q, 2047) == SMALL
    assert call(8000, 16000, 0, 1024, q, 2048) == INVALID and call(8000, 16000, p, 1024, 0, 2048) == INVALID
    assert call(8000, 16000, p + 1, 1023, q, 2048) == INVALID and call(8000, 16000, p, 1024, q + 1, 2048) == INVALID
    assert call(8000, 16000, q + 2048, 1024, q, 2048) == INVALID                  # the output's end overlaps the input
    assert call(8000, 16000, p, 1 << 40, q, 1 << 42) == INVALID
    assert call(8000, 16000, 0, 0, 0, 0) == OK                                    # n = 0 looks at no pointer
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    with pytest.raises(TypeError):
        mfcc_amd.resample(torch.zeros(8, dtype=torch.int32, device="cuda"), 8000, 16000)
    with pytest.raises(TypeError):
        mfcc_amd.resample(np.zeros(8, np.float32), 8000, 16000)
    with pytest.raises(ValueError):
        mfcc_amd.resample(np.zeros(8, np.int16), 0, 16000)
    with pytest.raises(mfcc_amd.MfccHipError):
        mfcc_amd.resample(np.zeros(8, np.int16), 16000, 16001)


def test_python_entry(mfcc_amd, handle):
    import torch
    x = samples(12345, 1)
    for ratio in [(8000, 16000), (44100, 16000)]:
        want = mfcc_amd.resample(x, *ratio)
        for m in (None, handle):
            got = mfcc_amd.resample(torch.from_numpy(x).cuda(), *ratio, mfcc=m)
            assert got.dtype == torch.int16 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        assert mfcc_amd.resample(torch.zeros(0, dtype=torch.int16, device="cuda"), *ratio).shape == (0,)


# ------------------------------------------------------------------------------------------------ R: the handle's rate

F512 = dict(nfft=512, nfilters=32, nceptrums=13)


def test_set_input_rate_refusals(mfcc_amd):
    from mfcc_amd import _lib as L
    import torch
    lib = L.load()
    BUSY = -104
    with mfcc_amd.MFCC(**F512) as m:
        assert m.input_rate is None and lib.mfcc_hip_input_rate(m._h) == 0 and lib.mfcc_hip_input_rate(None) == 0
        assert lib.mfcc_hip_set_input_rate(None, 8000) == INVALID and lib.mfcc_hip_set_input_rate(m._h, -1) == INVALID
        assert lib.mfcc_hip_set_input_rate(m._h, 16001) == UNSUPPORTED and lib.mfcc_hip_set_input_rate(m._h, 1001 * 16) == UNSUPPORTED
        assert lib.mfcc_hip_input_rate(m._h) == 0
        with pytest.raises(ValueError):
            m.set_input_rate(-8000)
        with pytest.raises(TypeError):
            m.set_input_rate(8000.0)
        for rate in (0, None, 16000):                                   # the handle's own rate: off
            m.set_input_rate(rate)
            assert m.input_rate is None and lib.mfcc_hip_input_rate(m._h) == 0
        # BUSY while a session, a bank, a gate or a resampler lives
        for live in (m.stream, lambda: m.stream_bank(2), lambda: m.power_gate(2), lambda: m.resampler(2, 8000)):
            obj = live()
            assert lib.mfcc_hip_set_input_rate(m._h, 8000) == BUSY and lib.mfcc_hip_input_rate(m._h) == 0
            obj.close()
        m.set_input_rate(8000)
        assert m.input_rate == 8000 and lib.mfcc_hip_input_rate(m._h) == 8000
        # UNSUPPORTED with a rate: sessions, banks, a shard with halo
        for make in (m.stream, lambda: m.stream(fixed=True), lambda: m.stream_bank(2), lambda: m.stream_bank(2, fixed=True),
                     lambda: m.stream_bank(2, normalize="mean", normalize_window=50)):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                make()
            assert e.value.code == UNSUPPORTED
        x = torch.zeros(4001, dtype=torch.int16, device="cuda")
        for fn in (m.process, m.process_fixed):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                fn(x, halo=1)
            assert e.value.code == UNSUPPORTED
        m.power_gate(2).close()                                         # rows in, not samples: not refused
        m.set_input_rate(None)
        m.stream().close()
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(samplerate=22050.5, input_rate=8000, **F512)
    assert e.value.code == INVALID
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(input_rate=16001, **F512)
    assert e.value.code == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ E: every entry point

CONFIGS = {
    "f512": (dict(F512), 8000),
    "f512_48k_in": (dict(F512), 48000),
    "htk400": (dict(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13, mel="htk"), 44100),
    "f1024": (dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0), 8000),
    "g256": (dict(nfft=256, nfilters=20, nceptrums=13, power_scale=0), 11025),
}


@pytest.fixture(scope="module", params=list(CONFIGS))
def twins(request, mfcc_amd):
    """(the handle with an input rate, the same handle without, the rate)"""
    kw, rate = CONFIGS[request.param]
    with mfcc_amd.MFCC(input_rate=rate, **kw) as a, mfcc_amd.MFCC(**kw) as b:
        assert a.kernel_name() == b.kernel_name() and a.input_rate == rate and b.input_rate is None
        yield a, b, rate


def speechlike(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 6000 * np.sin(0.05 * t + rng.uniform(0, 6)) + 3000 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def strided(torch, a, pad=24):
    """a (channels, n) array as a CUDA tensor whose rows lie `pad` samples apart"""
    big = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.from_numpy(a).dtype, device="cuda")
    big[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return big[:, :a.shape[1]]


def test_dense_entries(mfcc_amd, twins):
    import torch
    a, b, rate = twins
    n = 9000 * rate // 16000 + 5
    x = np.stack([speechlike(n, s) for s in range(3)])
    y = np.stack([mfcc_amd.resample(c, rate, 16000) for c in x])
    want = b.process(y)
    assert want.shape[1] == a.num_frames(n) and want.shape[1] > 16
    assert same(a.process(x[0]), want[0]) and same(a.process(x), want)                       # host buffers
    assert same(a.process(torch.from_numpy(x[0]).cuda()), want[0])                           # one channel on the device
    xs = strided(torch, x)
    assert xs.stride(0) > n
    assert same(a.process(xs), want)                                                         # three strided channels
    out = torch.empty((3, want.shape[1], want.shape[2]), device="cuda")
    assert a.time_launches(xs, out, warmup=1, iters=2) > 0 and same(out, want)               # mfcc_hip_time_dev
    short = x[0][:a.win_length * rate // 16000 // 2]                                         # no frame: no sample is read
    assert a.process(torch.from_numpy(short).cuda()).shape[0] == b.process(mfcc_amd.resample(short, rate, 16000)).shape[0]


def ragged_lengths(a, rate):
    """input lengths whose resampled lengths are 0, 1, (as near as the ratio gets) one below a frame, and one tile of
    frames plus one"""
    L, M, H, K = rr.geometry(rate, 16000)
    flen, hop = a.win_length, a.hop
    back = lambda n2: n2 * M // L                     # the longest input with at most n2 outputs
    return [0, 1, back(flen - 1), back(flen + 16 * hop), back(flen), 3000 * M // L]


def same_rows(got, want):
    return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))


def test_ragged_entries(mfcc_amd, twins):
    import torch
    a, b, rate = twins
    lens = ragged_lengths(a, rate)
    utts = [speechlike(n, 10 + i) for i, n in enumerate(lens)]
    res = [mfcc_amd.resample(u, rate, 16000) for u in utts]
    assert len(res[0]) == 0 and len(res[2]) < a.win_length <= len(res[4])
    want = b.process_batch(res)
    assert [len(w) for w in want] == [a.num_frames(n) for n in lens] and len(want[3]) == 17
    assert same_rows(a.process_batch(utts), want)                                            # host buffers
    flat = torch.from_numpy(np.concatenate([np.zeros(3, np.int16)] + utts)).cuda()           # offsets[0] = 3
    off = np.concatenate([[0], np.cumsum(lens)]) + 3
    got, fo = a.process_packed(flat, off)
    assert same_rows([got[int(fo[i]):int(fo[i + 1])] for i in range(len(lens))], want)
    eq = [utts[5]] * 3                                                                       # equal lengths: the uniform route
    assert same_rows(a.process_batch([torch.from_numpy(u).cuda() for u in eq]), b.process_batch([res[5]] * 3))
    assert a.process_batch([]) == [] and same_rows(a.process_batch([utts[1]]), [want[1]])


def test_fixed_entries(mfcc_amd):
    import torch
    kw, rate = dict(F512, pad_mode="stream"), 8000
    with mfcc_amd.MFCC(input_rate=rate, **kw) as a, mfcc_amd.MFCC(**kw) as b:
        x = np.stack([speechlike(5000, s) for s in range(2)])
        y = np.stack([mfcc_amd.resample(c, rate, 16000) for c in x])
        want = b.process_fixed(y)
        assert want.dtype == np.int16 and want.shape[1] > 16
        assert same(a.process_fixed(x), want) and same(a.process_fixed(strided(torch, x)), want)
        lens = [0, 1, 255, 600, 4000]
        utts = [speechlike(n, 20 + i) for i, n in enumerate(lens)]
        wantb = b.process_batch([mfcc_amd.resample(u, rate, 16000) for u in utts], fixed=True)
        assert same_rows(a.process_batch(utts, fixed=True), wantb)
        assert same_rows(a.process_batch([torch.from_numpy(u).cuda() for u in utts], fixed=True), wantb)


def test_ulaw_at_8k(mfcc_amd):
    import torch
    with mfcc_amd.MFCC(sample_format="ulaw", input_rate=8000, **F512) as a, mfcc_amd.MFCC(**F512) as b:
        rng = np.random.default_rng(3)
        x = rng.integers(0, 256, (3, 6001), dtype=np.uint8)
        y = np.stack([mfcc_amd.resample(mfcc_amd.decode(c, "ulaw"), 8000, 16000) for c in x])
        want = b.process(y)
        assert same(a.process(x), want) and same(a.process(strided(torch, x)), want)
        lens = [0, 1, 700, 3001]
        utts = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
        wantb = b.process_batch([mfcc_amd.resample(mfcc_amd.decode(u, "ulaw"), 8000, 16000) for u in utts])
        assert same_rows(a.process_batch(utts), wantb)
        assert same_rows(a.process_batch([torch.from_numpy(u).cuda() for u in utts]), wantb)


def test_post_chain_with_selection(mfcc_amd):
    import torch
    kw = dict(F512, normalize="meanvar", deltas=2, vad="select")
    with mfcc_amd.MFCC(input_rate=8000, **kw) as a, mfcc_amd.MFCC(**kw) as b:
        # loud stretches and quiet ones: the selection has something to drop
        utts = [(speechlike(n, 30 + i) * np.where(np.arange(n) % 2000 < 1200, 1.0, 0.01)).astype(np.int16)
                for i, n in enumerate([4000, 0, 2600, 4000])]
        want = b.process_batch([mfcc_amd.resample(u, 8000, 16000) for u in utts])
        assert 0 < sum(len(w) for w in want) < sum(a.num_frames(len(u)) for u in utts)           # some frames dropped
        assert same_rows(a.process_batch(utts), want)
        assert same_rows(a.process_batch([torch.from_numpy(u).cuda() for u in utts]), want)


def write_wav(path, x, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(x.astype("<i2").tobytes())


def test_convert_expects_the_input_rate(mfcc_amd, tmp_path):
    x = speechlike(8000, 5)
    write_wav(tmp_path / "a8.wav", x, 8000)
    write_wav(tmp_path / "a16.wav", mfcc_amd.resample(x, 8000, 16000), 16000)
    kw = dict(F512, pad_mode="stream")
    with mfcc_amd.MFCC(input_rate=8000, **kw) as a, mfcc_amd.MFCC(**kw) as b:
        for fixed in (True, False):
            n = a.convert(str(tmp_path / "a8.wav"), str(tmp_path / "got.mfcc"), fixed=fixed)
            assert n == b.convert(str(tmp_path / "a16.wav"), str(tmp_path / "want.mfcc"), fixed=fixed) and n > 16
            assert (tmp_path / "got.mfcc").read_bytes() == (tmp_path / "want.mfcc").read_bytes()
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            a.convert(str(tmp_path / "a16.wav"), str(tmp_path / "no.mfcc"))
        assert e.value.code == UNSUPPORTED
        n = a.convert(str(tmp_path / "a8.wav"), str(tmp_path / "got.mfcc"))
        assert a.convert_many([str(tmp_path / "a8.wav")] * 2, [str(tmp_path / "m0.mfcc"), str(tmp_path / "m1.mfcc")]) == [n, n]
        assert (tmp_path / "m1.mfcc").read_bytes() == (tmp_path / "got.mfcc").read_bytes()


# ------------------------------------------------------------------------------------------------ S: live lines

def chunkings(rng, total, lines, steps):
    """per step, the chunk length of every line: cuts of `total` with empty and 1-sample chunks among them"""
    per_line = []
    for _ in range(lines):
        cuts = np.sort(rng.integers(0, total + 1, steps - 3))
        lens = np.diff(np.concatenate([[0], cuts, [total]])).astype(int).tolist()
        for extra in (0, 1):
            lens.insert(int(rng.integers(0, len(lens) + 1)), extra)
        per_line.append(lens)
    return [[per_line[u][s] for u in range(lines)] for s in range(steps)]


@pytest.mark.parametrize("rate,fmt", [(48000, "s16"), (8000, "ulaw")], ids=["48k_s16", "8k_ulaw"])
def test_resampler_lines(mfcc_amd, rate, fmt):
    import torch
    lines, total = 5, 20000 * rate // 16000
    rng = np.random.default_rng(rate)
    raw = rng.integers(0, 256, (lines, total + 1), dtype=np.uint8) if fmt == "ulaw" else \
        np.stack([speechlike(total + 1, 40 + u) for u in range(lines)])
    whole = [mfcc_amd.resample(mfcc_amd.decode(raw[u, :total + 1], fmt), rate, 16000) for u in range(lines)]
    with mfcc_amd.MFCC(**F512) as m, m.resampler(lines, rate, fmt) as rs, m.stream_bank(lines) as bank:
        assert len(rs) == lines and rs.in_rate == rate and rs.out_rate == 16000 and not rs.seen.any()
        got, rows, pos = [[] for _ in range(lines)], [[] for _ in range(lines)], [0] * lines

        def take(out, oo, fed):
            r, fo = bank.push_packed(out, oo)                          # composed on the device: nothing visits the host
            for u in fed:
                got[u].append(out[int(oo[u]):int(oo[u + 1])])
                rows[u].append(r[int(fo[u]):int(fo[u + 1])])

        for lens in chunkings(rng, total, lines, 9):           # + the 1-sample chunk: total + 1
            chunks = [raw[u, pos[u]:pos[u] + lens[u]] for u in range(lines)]
            flat = torch.from_numpy(np.concatenate([np.zeros(2, raw.dtype)] + chunks)).cuda()
            off = np.concatenate([[0], np.cumsum(lens)]) + 2
            want_oo = rs.plan(off)
            out, oo = rs.push_packed(flat, off)
            assert np.array_equal(oo, want_oo)                          # the plan is what the push returns
            take(out, oo, range(lines))
            pos = [p + n for p, n in zip(pos, lens)]
            assert np.array_equal(rs.seen, pos)
        assert pos == [total + 1] * lines
        want_oo = rs.plan(flush=True)
        out, oo = rs.flush_packed()
        assert np.array_equal(oo, want_oo) and not rs.seen.any()
        take(out, oo, range(lines))
        for u in range(lines):
            assert same(torch.cat(got[u]), whole[u]), u                 # pushes plus flush: the one-shot result
            assert same(torch.cat(rows[u]), m.process(whole[u])), u     # ... and its frames
        # reset restarts a line; the host route; a flush of some lines
        first = rs.push([raw[u, :700] for u in range(lines)])
        rs.reset([1, 3])
        assert np.array_equal(rs.seen, [700, 0, 700, 0, 700])
        second = rs.push([raw[u, 700:1500] if u % 2 == 0 else raw[u, :1500] for u in range(lines)])
        tail = rs.flush([3, 0])
        one = [mfcc_amd.resample(mfcc_amd.decode(raw[u, :1500], fmt), rate, 16000) for u in range(lines)]
        assert same(np.concatenate([first[0], second[0], tail[1]]), one[0]) and same(np.concatenate([second[3], tail[0]]), one[3])
        assert np.array_equal(rs.seen, [0, 1500, 1500, 0, 1500])
        # refusals consume nothing
        from mfcc_amd import _lib as L
        oo = np.zeros(lines + 1, np.uint64)
        off = np.arange(lines + 1, dtype=np.uint64) * 100
        flat = torch.from_numpy(raw[0, :500].copy()).cuda()
        small = torch.empty(1, dtype=torch.int16, device="cuda")
        lib = L.load()
        assert lib.mfcc_hip_resampler_push_dev(rs._r, L.ptr(flat), L.ptr(off), L.ptr(small), 1, L.ptr(oo)) == SMALL
        assert int(oo[-1]) > 1 and np.array_equal(oo, rs.plan(off))
        assert lib.mfcc_hip_resampler_push_dev(rs._r, L.ptr(flat), L.ptr(off[::-1].copy()), L.ptr(small), 1 << 20, L.ptr(oo)) == INVALID
        assert lib.mfcc_hip_resampler_flush_dev(rs._r, None, 0, L.ptr(small), 1, L.ptr(oo)) == SMALL
        assert np.array_equal(rs.seen, [0, 1500, 1500, 0, 1500])


# ------------------------------------------------------------------------------------------------ M: scratch, and no rate

def test_scratch_grows_and_is_reused(mfcc_amd):
    import torch
    with mfcc_amd.MFCC(input_rate=8000, **F512) as a, mfcc_amd.MFCC(**F512) as b:
        for n in (3000, 40000, 1200, 40001, 3000):
            x = np.stack([speechlike(n, n + s) for s in range(2)])
            want = b.process(np.stack([mfcc_amd.resample(c, 8000, 16000) for c in x]))
            assert same(a.process(strided(torch, x)), want), n
            utts = [x[0], x[1][:n // 3]]
            assert same_rows(a.process_batch([torch.from_numpy(u).cuda() for u in utts]),
                             b.process_batch([mfcc_amd.resample(u, 8000, 16000) for u in utts])), n


def test_no_rate_is_the_plain_handle(mfcc_amd):
    import torch
    x = np.stack([speechlike(9000, s) for s in range(2)])
    with mfcc_amd.MFCC(input_rate=8000, **F512) as a, mfcc_amd.MFCC(**F512) as fresh:
        a.process(x)
        a.set_input_rate(None)
        assert a.input_rate is None and a.num_frames(9000) == fresh.num_frames(9000)
        assert same(a.process(x), fresh.process(x)) and same(a.process(strided(torch, x)), fresh.process(x))
        assert same_rows(a.process_batch([x[0], x[1][:4000]]), fresh.process_batch([x[0], x[1][:4000]]))
        a.stream_bank(2).close()
