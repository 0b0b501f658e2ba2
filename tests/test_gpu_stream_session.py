"""Streaming / online session (mfcc_hip_stream_*): any chunking of a stream reproduces the one-shot result
bit for bit, both contracts, both framing modes -- the core's sink/source/reset interface
(mfcc/core/mfcc.py:28-30,116; wav2mfcc.py:27-42; receiver loop software/cepstrum.c:93-159)."""
import numpy as np
import pytest

from kernel_families import same
from oracle import mfcc_fixed as mx
from oracle import mfcc_float as mf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _chunks(n, kind, rng):
    pos = 0
    while pos < n:
        if kind == "driver":                      # the host driver's own pattern: 512, then 170 per round (main.c:134)
            c = 512 if pos == 0 else 170
        elif kind == "random":
            c = int(rng.choice([1, 2, 7, 169, 170, 171, 341, 511, 512, 513, 1000, 4096, 30000]))
        else:
            c = int(kind)
        yield pos, min(n, pos + c)
        pos += c


def _run(sess, pcm, kind, seed=0):
    rng = np.random.default_rng(seed)
    rows = [sess.push(pcm[a:b]) for a, b in _chunks(len(pcm), kind, rng)]
    rows.append(sess.flush())
    return np.concatenate(rows)


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("pad_mode", ["stream", "notebook"])
def test_any_chunking_equals_one_shot(mfcc_amd, wav_pcm, fixed, pad_mode):
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=32, pad_mode=pad_mode) as m:
        one = m.process_fixed(wav_pcm) if fixed else m.process(wav_pcm)
        with m.stream(fixed=fixed) as s:
            for kind in ("driver", 170, 171, 4096, "random", len(wav_pcm)):
                got = _run(s, wav_pcm, kind, seed=3)
                assert got.dtype == one.dtype and got.shape == one.shape, (kind, got.shape, one.shape)
                assert np.array_equal(got, one), kind
                assert s.pending == 0                                    # flush leaves a reset session
            # one sample at a time (the RTL's own rate): the first 6000 samples, then the rest in one push
            rows = [s.push(wav_pcm[i:i + 1]) for i in range(6000)]
            assert sum(len(r) for r in rows) == (6000 - 512) // 170 + 1
            rows += [s.push(wav_pcm[6000:]), s.flush()]
            assert np.array_equal(np.concatenate(rows), one)
    # and the one-shot result is the oracle's
    if fixed:
        assert np.array_equal(one, mx.mfcc_fixed_ref(wav_pcm, nceptrums=32, pad_mode=pad_mode))
    else:
        ref = mf.mfcc_float_ref(wav_pcm, n_cep=32, pad_mode=pad_mode)
        assert np.abs(one - ref).max() / np.abs(ref).max() < 2e-5


def test_reset_mid_stream_and_short_streams(mfcc_amd, wav_pcm):
    """`reset` (bit 31 of a word, wav2mfcc.py:27-36) drops the frame in progress and the pre-emphasis history;
    streams shorter than a frame give the driver's single zero-padded frame; an empty flush too."""
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=16, pad_mode="stream") as m, m.stream(fixed=True) as s:
        assert s.push(wav_pcm[:1000]).shape == (3, 16) and s.pending == 1000 - 3 * 170
        s.reset()
        assert s.pending == 0
        got = np.concatenate([s.push(wav_pcm[5000:9000]), s.flush()])
        assert np.array_equal(got, m.process_fixed(wav_pcm[5000:9000]))
        for n in (0, 1, 100, 511):
            got = np.concatenate([s.push(wav_pcm[:n]), s.flush()])
            assert got.shape == (1, 16)
            assert np.array_equal(got, m.process_fixed(wav_pcm[:n]))
            assert np.array_equal(got, mx.mfcc_fixed_ref(wav_pcm[:n], nceptrums=16, pad_mode="stream"))
        # two sessions on one handle are independent
        with m.stream(fixed=True) as s2:
            a = s.push(wav_pcm[:700])
            b = s2.push(wav_pcm[20000:20700])
            a2, b2 = s.push(wav_pcm[700:1400]), s2.push(wav_pcm[20700:21400])
            assert np.array_equal(np.concatenate([a, a2]), m.process_fixed(wav_pcm[:1400])[:len(a) + len(a2)])
            assert np.array_equal(np.concatenate([b, b2]), m.process_fixed(wav_pcm[20000:21400])[:len(b) + len(b2)])


def test_stream_feeds_the_serial_wire_format(mfcc_amd, wav_pcm):
    """The UART byte stream (0xa55a + n_cep big-endian int16 per frame, misc/magic.py:27-39) packed from the
    streamed columns equals the one packed from the one-shot result; the receiver decodes it back."""
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=16, pad_mode="stream") as m, m.stream(fixed=True) as s:
        one = m.process_fixed(wav_pcm)
        wire = b"".join(mfcc_amd.wire.pack_columns(s.push(wav_pcm[a:a + 4000])) for a in range(0, len(wav_pcm), 4000))
        wire += mfcc_amd.wire.pack_columns(s.flush())
    assert wire == mfcc_amd.wire.pack_columns(one)
    cols, used = mfcc_amd.wire.unpack_columns(wire, 16)
    assert used == len(wire) and np.array_equal(cols, one)


def test_push_with_a_small_buffer_leaves_the_session_untouched(mfcc_amd, wav_pcm):
    import ctypes as C
    lib = mfcc_amd.load_library()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m, m.stream() as s:
        x = np.ascontiguousarray(wav_pcm[:2000])
        out = np.empty((2, 13), np.float32)
        nf = C.c_size_t(0)
        rc = lib.mfcc_hip_stream_push(s._s, x.ctypes.data, x.size, out.ctypes.data, out.size, C.byref(nf))
        assert rc == -106 and nf.value == 9 and s.pending == 0           # BUFFER_SMALL, nothing consumed
        assert np.array_equal(s.push(x), m.process(x))


# ---- what the C entry points answer at their edges (include/mfcc_hip.h: mfcc_hip_stream_*), through ctypes.  The one-shot
# call is the witness wherever rows come out; 3000 samples of the golden wav: 15 frames at 512 / 170, 450 pending

N_EDGE = 3000


def _open(mfcc_amd, fixed, pad_mode="stream", **kw):
    return mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=16 if fixed else 13, pad_mode=pad_mode, **kw)


def _one_shot(m, fixed, x):
    return m.process_fixed(x) if fixed else m.process(x)


def _c_push(s, x, n, out, cap, want_nf=True):
    """mfcc_hip_stream_push with any argument NULL (None); returns (rc, *n_frames_out or None)."""
    import ctypes as C
    nf = C.c_size_t(12345)
    rc = s._lib.mfcc_hip_stream_push(s._s, None if x is None else x.ctypes.data, n, None if out is None else out.ctypes.data,
                                     cap, C.byref(nf) if want_nf else None)
    return rc, (int(nf.value) if want_nf else None)


def _c_flush(s, out, cap, want_nf=True):
    import ctypes as C
    nf = C.c_size_t(12345)
    rc = s._lib.mfcc_hip_stream_flush(s._s, None if out is None else out.ctypes.data, cap, C.byref(nf) if want_nf else None)
    return rc, (int(nf.value) if want_nf else None)


@pytest.mark.parametrize("fixed", [False, True])
def test_push_refusals_consume_nothing_and_empty_pushes_succeed(mfcc_amd, wav_pcm, fixed):
    from mfcc_amd import _lib as L
    x = np.ascontiguousarray(wav_pcm[:N_EDGE])
    with _open(mfcc_amd, fixed) as m, m.stream(fixed=fixed) as s:
        one = _one_shot(m, fixed, x)
        W = one.shape[1]
        out = np.empty((16, W), one.dtype)
        head = s.push(x[:1000])
        assert head.shape == (3, W) and s.pending == 490
        # NULL samples with n > 0: INVALID_PARAM, whatever the output buffer is like
        for o, cap in ((out, out.size), (out, 1), (None, 0), (None, out.size)):
            assert _c_push(s, None, 2000, o, cap)[0] == L.ERROR_INVALID_PARAM and s.pending == 490
        assert _c_push(s, None, 2000, None, 0, want_nf=False)[0] == L.ERROR_INVALID_PARAM and s.pending == 490
        # BUFFER_SMALL: the count is written all the same, a NULL count is accepted, nothing is consumed
        rest = x[1000:]
        for o, cap in ((out, 11 * W), (out, 12 * W - 1), (None, out.size)):
            assert _c_push(s, rest, rest.size, o, cap) == (L.ERROR_BUFFER_SMALL, 12) and s.pending == 490
            assert _c_push(s, rest, rest.size, o, cap, want_nf=False)[0] == L.ERROR_BUFFER_SMALL and s.pending == 490
        # n = 0: success with 0 frames, with and without pointers
        assert _c_push(s, None, 0, None, 0) == (0, 0) and s.pending == 490
        assert _c_push(s, rest, 0, out, out.size) == (0, 0) and s.pending == 490
        assert _c_push(s, None, 0, None, 0, want_nf=False)[0] == 0 and s.pending == 490
        # a push that completes no frame needs no output buffer; one that does may leave the count out
        assert _c_push(s, rest, 21, None, 0) == (0, 0) and s.pending == 511
        assert _c_push(s, rest[21:], rest.size - 21, out, 12 * W, want_nf=False)[0] == 0 and s.pending == 450
        assert same(np.concatenate([head, out[:12], s.flush()]), one)


@pytest.mark.parametrize("fixed", [False, True])
def test_flush_with_a_small_buffer_keeps_the_pending_samples(mfcc_amd, wav_pcm, fixed):
    from mfcc_amd import _lib as L
    x = np.ascontiguousarray(wav_pcm[:N_EDGE])
    with _open(mfcc_amd, fixed) as m, m.stream(fixed=fixed) as s:
        one = _one_shot(m, fixed, x)
        W = one.shape[1]
        assert same(s.push(x), one[:-1]) and s.pending == 450
        row = np.empty((1, W), one.dtype)
        for o, cap in ((None, 0), (None, W), (row, W - 1), (row, 0)):
            assert _c_flush(s, o, cap) == (L.ERROR_BUFFER_SMALL, 1) and s.pending == 450
            assert _c_flush(s, o, cap, want_nf=False)[0] == L.ERROR_BUFFER_SMALL and s.pending == 450
        assert _c_flush(s, row, W) == (0, 1) and s.pending == 0
        assert same(row, one[-1:])
        # the flush left a reset session: its next flush is the one of a fresh one (below), a NULL count is accepted
        assert _c_flush(s, row, W, want_nf=False)[0] == 0
        assert same(row, _one_shot(m, fixed, x[:0]))


@pytest.mark.parametrize("fixed", [False, True])
def test_flush_of_a_fresh_session_is_the_tail_frame_of_no_samples(mfcc_amd, wav_pcm, fixed):
    with _open(mfcc_amd, fixed) as m:
        empty = _one_shot(m, fixed, wav_pcm[:0])
        assert empty.shape[0] == 1
        with m.stream(fixed=fixed) as s:
            for _ in range(2):                                           # ... and again: every flush leaves a reset session
                got = s.flush()
                assert got.dtype == empty.dtype and same(got, empty) and s.pending == 0


@pytest.mark.parametrize("fixed", [False, True])
def test_notebook_flush_gives_no_row_and_resets(mfcc_amd, wav_pcm, fixed):
    x = np.ascontiguousarray(wav_pcm[:N_EDGE])
    with _open(mfcc_amd, fixed, pad_mode="notebook") as m, m.stream(fixed=fixed) as s:
        one = _one_shot(m, fixed, x)
        assert len(one) == 15
        assert _c_flush(s, None, 0) == (0, 0) and s.pending == 0         # fresh: nothing, and no buffer is needed
        assert len(s.push(x[:700])) == 2 and s.pending == 360
        assert _c_flush(s, None, 0) == (0, 0) and s.pending == 0
        assert len(s.push(x[:100])) == 0 and s.pending == 100
        assert s.flush().shape == (0, one.shape[1]) and s.pending == 0
        assert same(s.push(x), one) and s.flush().shape[0] == 0   # history and pending samples are gone


@pytest.mark.parametrize("fixed", [False, True])
def test_a_used_session_after_flush_or_reset_equals_a_fresh_one(mfcc_amd, wav_pcm, fixed):
    x = np.ascontiguousarray(wav_pcm[:N_EDGE])
    with _open(mfcc_amd, fixed) as m, m.stream(fixed=fixed) as s:
        one = _one_shot(m, fixed, x)
        fresh = _run(s, x, 700)
        assert same(fresh, one)
        assert same(_run(s, x, 700), one)                      # behind a flush
        s.reset()
        assert same(_run(s, x, 171), one)                      # behind a flush and a reset
        s.push(wav_pcm[5000:5900])
        s.reset()
        assert s.pending == 0 and same(_run(s, x, 700), one)   # behind a reset mid-stream


@pytest.mark.parametrize("fixed,fmt", [(False, "s16"), (True, "s16"), (False, "alaw")])
def test_a_session_is_a_bank_of_one(mfcc_amd, wav_pcm, fixed, fmt):
    import decode_ref as dr
    x = dr.encode_like(wav_pcm[:N_EDGE], fmt, np.random.default_rng(5))
    cuts = [0, 1, 171, 512, 513, 513, 1200, 1370, N_EDGE]                # no frame, one, several; an empty chunk
    with _open(mfcc_amd, fixed, sample_format=fmt) as m, m.stream(fixed=fixed) as s, m.stream_bank(1, fixed=fixed) as bank:
        for a, b in zip(cuts, cuts[1:]):
            rows, = bank.push([x[a:b]])
            got = s.push(x[a:b])
            assert got.dtype == rows.dtype and same(got, rows), (a, b)
            assert s.pending == int(bank.pending[0])
        tail, = bank.flush()
        assert same(s.flush(), tail) and tail.shape[0] == 1
        assert s.pending == 0 and int(bank.pending[0]) == 0
