"""Centred framing on the GPU (include/mfcc_hip.h "centring").

The contract is bit identity: a centred handle on ``x`` returns what the same handle uncentred returns on
``center_pad(x)`` (the host function, itself held to ``np.pad`` on the CPU) -- every kernel family, every entry point,
dense and ragged, NumPy and device tensors, behind every sample format and an input rate.  The kernel is also run alone
on every format, length class and alignment, with poison around its output; the frames are held to ``torch.stft`` by the
power spectrum's own error bound; the refusals leave the handle as it was; and the stage reads and writes past sample
2^31 and byte 2^32.

The shapes are the smallest at which the stage or the kernels behind it can go wrong: one frame (``n = PL + 1``), a tile
of 16 frames plus one (``16 hop``), and the hop's residues 0, 1 and ``hop - 1``; a channel stride that is no multiple of
8 and views that start 1, 3 and 5 samples past a 16-byte boundary.
"""
import ctypes as C

import numpy as np
import pytest

import center_ref as cr
import far_offsets as fo
import kernel_families as kf
import spectrum_ref as sr
from kernel_families import as_np, same
from mfcc_amd import _lib as L
from test_gpu_far_inputs import Arena, _far_equals_near, _format_inputs, _inputs, _ragged, _skw, SHAPES

pytestmark = pytest.mark.gpu

MODES = cr.MODES
KINDS3 = ["speech", "uniform", "silences"]

# id -> (MFCC() arguments, kernel of process, environment)
HANDLES = {
    "512_w12": (dict(nfft=512, nfilters=32, nceptrums=13), "mfcc_fused512_w12_kernel", {}),
    "512_w4": (dict(nfft=512, nfilters=32, nceptrums=13), "mfcc_fused512_kernel", {"MFCC_HIP_FUSED512": "w4"}),
    "512_h160": (dict(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=13), "mfcc_fused512_h160_kernel", {}),
    "512_h160_htk40": (dict(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13, mel="htk", fmin=20, fmax=8000,
                            output="logmel"), "mfcc_fused512_h160_mb_kernel", {}),
    "1024": (dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0), "mfcc_fused1024_w12bf_kernel", {}),
    "g256_200": (dict(nfft=256, hop=80, win_length=200, nfilters=20, nceptrums=13, power_scale=0),
                 "mfcc_float_generic_kernel", {}),
    "g64": (dict(nfft=64, nfilters=8, nceptrums=8, power_scale=0), "mfcc_float_generic_kernel", {}),
}


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _open(mfcc_amd, monkeypatch, hid, **over):
    """The handle ``hid`` with ``over`` on top; fails unless it runs the kernel the id names."""
    kw, kernel, env = HANDLES[hid]
    for var in ("MFCC_HIP_FUSED512", "MFCC_HIP_FUSED1024"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    m = mfcc_amd.MFCC(**dict(kw, **over))
    assert m.kernel_name() == kernel, (hid, m.kernel_name())
    return m


def _framing(kw):
    nfft = kw["nfft"]
    return nfft, kw.get("hop") or nfft // 3, kw.get("win_length") or nfft


def _bank(mfcc_amd, m):
    m.set_filterbank(mfcc_amd.htk_filterbank(80, nfft=m.nfft), "log2")


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _misaligned(x, start):
    """``x`` (channels, n) on the device with channel stride ``n + 3``, channel 0 ``start`` samples past a 16-byte boundary."""
    import torch
    nch, n = x.shape
    buf = torch.full((16 + nch * (n + 3),), fo.POISON_I16, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (nch, n), (n + 3, 1), storage_offset=8 + start)
    view.copy_(_dev(x))
    assert view.data_ptr() % 16 == 2 * ((8 + start) % 8)
    return view


ENTRIES = ("process", "power_spectrum", "filterbank")


# ------------------------------------------------------------------------------------------- bit identity, every family
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hid", list(HANDLES))
def test_centred_handle_is_the_plain_handle_on_the_padded_signal(mfcc_amd, monkeypatch, wav_pcm, hid, mode):
    nfft, hop, flen = _framing(HANDLES[hid][0])
    pl = cr.left_pad(nfft, flen)
    with _open(mfcc_amd, monkeypatch, hid, center=mode) as m, _open(mfcc_amd, monkeypatch, hid) as plain:
        assert m.center == mode and plain.center is None
        _bank(mfcc_amd, m)
        _bank(mfcc_amd, plain)
        for n in (pl + 1, 16 * hop, 16 * hop + 1, 17 * hop - 1):
            x = kf.channels(n, 40 + n, wav_pcm, KINDS3)
            p = np.stack([mfcc_amd.center_pad(c, mode, nfft=nfft, hop=hop, win_length=flen) for c in x])
            frames = 1 + n // hop
            assert p.shape == (3, (frames - 1) * hop + flen) and m.num_frames(n) == frames == plain.num_frames(p.shape[1])
            for entry in ENTRIES:
                want = getattr(plain, entry)(_dev(p))
                assert want.shape[:2] == (3, frames)
                what = "%s %s %s n=%d" % (hid, mode, entry, n)
                assert same(getattr(m, entry)(x), want), what + " (NumPy)"
                assert same(getattr(m, entry)(x[1]), want[1]), what + " (NumPy, one channel)"
                assert same(getattr(m, entry)(_dev(x[2])), want[2]), what + " (device, one channel)"
                for start in (1, 3, 5):
                    assert same(getattr(m, entry)(_misaligned(x, start)), want), what + " (device, start %d)" % start


# ------------------------------------------------------------------------------------------------------------ ragged
RAGGED_HANDLES = ["512_w12", "512_h160", "g256_200"]          # tile records, pack and gather on a fused and a generic kernel


def _corpora(nfft, hop, flen):
    return {"mixed": cr.corpus_lengths(nfft, hop, flen), "reversed": cr.corpus_lengths(nfft, hop, flen)[::-1],
            "equal": [5 * hop] * 3}


def _utterances(lens, wav_pcm, seed):
    kinds = ["speech", "noise", "uniform", "silences"]
    return [kf.signal(kinds[i % 4], v, seed + i, wav_pcm) for i, v in enumerate(lens)]


def _flat(utts, first):
    """(device tensor with ``first`` poison samples in front, offsets)"""
    offs = first + np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.uint64)
    flat = np.concatenate([np.full(first, fo.POISON_I16, np.int16)] + list(utts))
    return _dev(flat), offs


def _plan(lens, nfft, hop, flen, mode):
    return np.concatenate([[0], np.cumsum([cr.frames(v, nfft, hop, flen, mode) for v in lens])])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hid", RAGGED_HANDLES)
def test_ragged_calls_give_every_utterance_its_dense_rows(mfcc_amd, monkeypatch, wav_pcm, hid, mode):
    nfft, hop, flen = _framing(HANDLES[hid][0])
    with _open(mfcc_amd, monkeypatch, hid, center=mode) as m:
        _bank(mfcc_amd, m)
        for name, lens in _corpora(nfft, hop, flen).items():
            utts = _utterances(lens, wav_pcm, 300)
            plan = _plan(lens, nfft, hop, flen, mode)
            assert plan[-1] > 0 and (name == "equal" or 0 in np.diff(plan))      # utterances without a frame are in it
            dense = {e: [getattr(m, e)(_dev(u)) for u in utts] for e in ENTRIES}
            for first in (0, 7):
                flat, offs = _flat(utts, first)
                for entry, packed in (("process", m.process_packed), ("power_spectrum", m.power_spectrum_packed),
                                      ("filterbank", m.filterbank_packed)):
                    rows, fro = packed(flat, offs)
                    assert list(fro) == list(plan), (hid, mode, name, entry)
                    for i in range(len(utts)):
                        assert same(rows[int(fro[i]):int(fro[i + 1])], dense[entry][i]), \
                            "%s %s %s %s: utterance %d (offsets from %d)" % (hid, mode, name, entry, i, first)
            for batch in (m.process_batch(utts), m.process_batch([_dev(u) for u in utts])):
                assert len(batch) == len(utts)
                for i, got in enumerate(batch):
                    assert same(got, dense["process"][i]), "%s %s %s process_batch: utterance %d" % (hid, mode, name, i)


@pytest.mark.parametrize("post", [dict(normalize="meanvar", deltas=2), dict(vad="select")], ids=["meanvar_deltas2", "vad_select"])
@pytest.mark.parametrize("hid", RAGGED_HANDLES)
def test_ragged_calls_with_the_chain_behind_them(mfcc_amd, monkeypatch, wav_pcm, hid, post):
    nfft, hop, flen = _framing(HANDLES[hid][0])
    with _open(mfcc_amd, monkeypatch, hid, center=True, **post) as m, _open(mfcc_amd, monkeypatch, hid, **post) as plain:
        for name, lens in _corpora(nfft, hop, flen).items():
            utts = _utterances(lens, wav_pcm, 400)
            # one utterance through the same handle (a vad handle takes it through the ragged entry), and the plain
            # handle on the host-padded utterance
            single = [m.process(_dev(u)) for u in utts]
            for u, one in zip(utts, single):
                p = mfcc_amd.center_pad(u, "reflect", nfft=nfft, hop=hop, win_length=flen)
                if len(p):
                    assert same(one, plain.process(_dev(p))), (hid, name, len(u))
                else:
                    assert one.shape[0] == 0
            for first in (0, 7):
                flat, offs = _flat(utts, first)
                rows, fro = m.process_packed(flat, offs)
                assert rows.shape == (int(fro[-1]), m.num_features)
                if "vad" not in post:
                    assert list(fro) == list(_plan(lens, nfft, hop, flen, "reflect"))
                for i in range(len(utts)):
                    assert same(rows[int(fro[i]):int(fro[i + 1])], single[i]), (hid, name, i, first)


# ------------------------------------------------------------------------------------------------------ kernel direct
FORMATS = ["s16", "ulaw", "alaw", "u8", "i2s32", "s32", "f32"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_center_dev_is_center_host_of_the_decoded_samples(mfcc_amd, monkeypatch, fmt, mode):
    import torch
    hid = "512_h160"
    nfft, hop, flen = _framing(HANDLES[hid][0])
    pl = cr.left_pad(nfft, flen)
    code = mfcc_amd.api._sample_args(fmt)[1]
    with _open(mfcc_amd, monkeypatch, hid) as m:
        for n in (pl + 1, pl + 9, 1000, 4099):
            x = _format_inputs(fmt, n, 1)[0]
            want = mfcc_amd.center_pad(mfcc_amd.decode(x, fmt), mode, nfft=nfft, hop=hop, win_length=flen)
            np_ = len(want)
            assert np_ == cr.padded_len(n, nfft, hop, flen, mode) > 0
            src = torch.zeros(n + 16, dtype=getattr(torch, x.dtype.name), device="cuda")
            dst = torch.empty(np_ + 32, dtype=torch.int16, device="cuda")
            want_d = _dev(want)
            for di in range(8):
                src[di:di + n] = _dev(x)
                for do in range(8):
                    dst.fill_(fo.SENTINEL_I16)
                    out = dst[8 + do:8 + do + np_]
                    n_out = C.c_size_t(0)
                    m._call(dst.device, "center_dev", m._h, L.CENTER_REFLECT if mode == "reflect" else L.CENTER_ZEROS, code,
                            L.ptr(src[di:di + n]), n, L.ptr(out), np_, C.byref(n_out))
                    assert n_out.value == np_
                    assert torch.equal(out, want_d), "%s %s n=%d in+%d out+%d" % (fmt, mode, n, di, do)
                    assert bool((dst[:8 + do] == fo.SENTINEL_I16).all()) and bool((dst[8 + do + np_:] == fo.SENTINEL_I16).all()), \
                        "%s %s n=%d in+%d out+%d: wrote outside [out, out + N')" % (fmt, mode, n, di, do)
        # the Python form, a short capacity and a signal without a frame
        x = _format_inputs(fmt, 1000, 1)[0]
        want = mfcc_amd.center_pad(mfcc_amd.decode(x, fmt), mode, nfft=nfft, hop=hop, win_length=flen)
        with _open(mfcc_amd, monkeypatch, hid, sample_format=fmt) as mf:
            assert same(mfcc_amd.center_pad(_dev(x), mode, mfcc=mf), want)
        dst = torch.full((len(want),), fo.SENTINEL_I16, dtype=torch.int16, device="cuda")
        n_out = C.c_size_t(0)
        rc = m._call(dst.device, "center_dev", m._h, 1, code, L.ptr(_dev(x)), 1000, L.ptr(dst), len(want) - 1, C.byref(n_out),
                     ok=(L.ERROR_BUFFER_SMALL,))
        assert rc == L.ERROR_BUFFER_SMALL and n_out.value == len(want) and bool((dst == fo.SENTINEL_I16).all())
        rc = m._call(dst.device, "center_dev", m._h, 1, code, L.ptr(_dev(x)), pl, L.ptr(dst), len(want), C.byref(n_out))
        assert rc == L.SUCCESS and n_out.value == 0 and bool((dst == fo.SENTINEL_I16).all())


# -------------------------------------------------------------------------------------------------------- chain order
def test_decode_then_resample_then_centre(mfcc_amd, monkeypatch, wav_pcm):
    hid = "512_w12"
    nfft, hop, flen = _framing(HANDLES[hid][0])
    rng = np.random.default_rng(9)

    def by_hand(u):
        y = mfcc_amd.resample(mfcc_amd.decode(u, "ulaw"), 8000, 16000)
        return mfcc_amd.center_pad(y, "reflect", nfft=nfft, hop=hop, win_length=flen)

    with _open(mfcc_amd, monkeypatch, hid, sample_format="ulaw", input_rate=8000, center=True) as m, \
            _open(mfcc_amd, monkeypatch, hid) as plain:
        x = rng.integers(0, 256, (3, 8 * hop + 1)).astype(np.uint8)
        p = np.stack([by_hand(c) for c in x])
        want = plain.process(_dev(p))
        assert want.shape[1] == m.num_frames(x.shape[1]) == 1 + (2 * x.shape[1]) // hop
        assert same(m.process(_dev(x)), want) and same(m.process(x), want)
        lens = [0, 1, 100, 129, 5 * hop, 3 * hop + 7]             # at 8 kHz: 0, 2 and 200 samples give no frame at 16 kHz
        utts = [rng.integers(0, 256, v).astype(np.uint8) for v in lens]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        rows, fro = m.process_packed(_dev(np.concatenate(utts)), offs)
        assert list(np.diff(fro)) == [m.num_frames(v) for v in lens] and list(np.diff(fro))[:3] == [0, 0, 0]
        for i, u in enumerate(utts):
            p = by_hand(u)
            got = rows[int(fro[i]):int(fro[i + 1])]
            assert got.shape[0] == (plain.num_frames(len(p)) if len(p) else 0)
            if len(p):
                assert same(got, plain.process(_dev(p))), i
        for i, got in enumerate(m.process_batch(utts)):
            assert same(got, rows[int(fro[i]):int(fro[i + 1])]), i


# ------------------------------------------------------------------------------------- against the published definition
@pytest.mark.parametrize("nfft,hop,flen", [(512, 160, 400), (512, 170, 512)], ids=["512_160_400", "512_170_512"])
def test_power_spectrum_is_torch_stft_power(mfcc_amd, wav_pcm, nfft, hop, flen):
    """Every element within ``spectrum_ref.bound`` of ``|torch.stft(center=True, pad_mode="reflect")|**2 / power_scale**2``
    in float64, the constant as it stands; 33 frames, none of them all zero, so no element is excused."""
    scale = sr.power_scale_of(nfft)
    window = mfcc_amd.window("hann", flen).astype(np.float64)
    n = 32 * hop + 5
    zero = np.zeros(33, dtype=bool)
    with mfcc_amd.MFCC(nfft=nfft, hop=hop, win_length=flen, window="hann", preemph=0, center=True, nfilters=8, nceptrums=8,
                       power_scale=scale) as m:
        assert m.num_frames(n) == 33
        for i, kind in enumerate(["speech", "noise", "sine8"]):
            x = sr.signal(kind, n, 11 + i, wav_pcm, nfft)
            ref = cr.stft_power(x, nfft, hop, flen, window) / (scale * scale)
            assert ref.shape == (33, nfft // 2 + 1)
            b = sr.bound(ref)
            sr.assert_not_blind(b, zero, kind)
            for got in (m.power_spectrum(x), as_np(m.power_spectrum(_dev(x)))):
                worst = sr.check(got, ref, b, "%d/%d/%d %s" % (nfft, hop, flen, kind))
                print("%d/%d/%d %s: worst |got - torch.stft| / bound %.3f" % (nfft, hop, flen, kind, worst))


# ----------------------------------------------------------------------------------------------------------- refusals
def _refused(mfcc_amd, code, fn, *a, **kw):
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def test_refusals_leave_the_handle_as_it_was(mfcc_amd, monkeypatch, wav_pcm):
    hid = "512_w12"
    nfft, hop, flen = _framing(HANDLES[hid][0])
    x = kf.signal("speech", 16 * hop + 1, 3, wav_pcm)
    UNSUPPORTED, BUSY = L.ERROR_UNSUPPORTED, L.ERROR_BUSY
    with _open(mfcc_amd, monkeypatch, hid, center=True) as m:
        _bank(mfcc_amd, m)
        before = m.process(_dev(x))
        assert before.shape[0] == 17

        def unchanged():
            assert m.center == "reflect" and same(m.process(_dev(x)), before)

        _refused(mfcc_amd, UNSUPPORTED, m.process, _dev(np.concatenate([[0], x]).astype(np.int16)), halo=1)
        unchanged()
        for call in (lambda: m.process_fixed(_dev(x)), lambda: m.process_fixed(x),
                     lambda: m.process_packed(_dev(x), [0, len(x)], fixed=True), lambda: m.process_batch([x], fixed=True)):
            _refused(mfcc_amd, UNSUPPORTED, call)
            unchanged()
        for call in (m.stream, lambda: m.stream(fixed=True), lambda: m.stream_bank(2), lambda: m.stream_bank(2, filterbank=True),
                     lambda: m.resampler(2, 8000)):
            _refused(mfcc_amd, UNSUPPORTED, call)
            unchanged()
        with pytest.raises(ValueError):
            m.set_center("edge")
        assert L.load().mfcc_hip_set_center(m._h, 3) == L.ERROR_INVALID_PARAM
        unchanged()
        m.set_center("zeros")
        assert m.center == "zeros" and m.process(_dev(x)).shape == before.shape and not same(m.process(_dev(x)), before)
        m.set_center(None)
        assert m.center is None and m.process(_dev(x)).shape[0] == m.num_frames(len(x)) == (len(x) - 512) // hop + 1
    # a stream-padding handle frames past the end: it cannot be centred
    with _open(mfcc_amd, monkeypatch, hid, pad_mode="stream") as m:
        before = m.process(_dev(x))
        _refused(mfcc_amd, UNSUPPORTED, m.set_center, True)
        assert m.center is None and same(m.process(_dev(x)), before)
        m.set_center(None)
    with pytest.raises(mfcc_amd.MfccHipError) as e:
        mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream", center=True)
    assert e.value.code == UNSUPPORTED
    # BUSY while a bank lives, fine once it is closed
    with _open(mfcc_amd, monkeypatch, hid) as m:
        before = m.process(_dev(x))
        bank = m.stream_bank(2)
        _refused(mfcc_amd, BUSY, m.set_center, True)
        assert m.center is None and same(m.process(_dev(x)), before)
        bank.close()
        m.set_center(True)
        assert m.center == "reflect" and m.process(_dev(x)).shape[0] == 17


# ----------------------------------------------------------------------------------------------------- far addressing
@pytest.fixture(scope="module")
def arena():
    import torch
    a = Arena()
    yield a
    assert bool((a.i16[:1 << 20] == fo.POISON_I16).all()) and bool((a.i16[fo.GUARD - (1 << 20):fo.GUARD] == fo.POISON_I16).all())
    del a.i16, a.words
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", MODES)
def test_centring_reads_far_channels(mfcc_amd, arena, wav_pcm, mode):
    cfg = (512, 160, 400)
    n = SHAPES["spectrum512_h160"][0]
    x = _inputs(n, 770, wav_pcm)
    with mfcc_amd.MFCC(**_skw(cfg, center=mode)) as m, mfcc_amd.MFCC(**_skw(cfg)) as plain:
        got = _far_equals_near(arena, x, m.power_spectrum, "centred %s" % mode)
        p = mfcc_amd.center_pad(x[2], mode, nfft=512, hop=160, win_length=400)
        assert same(got[2], plain.power_spectrum(p))                   # the channel across sample 2^32


@pytest.mark.parametrize("lens", ["ragged", "uniform"])
def test_centring_reads_far_utterances(mfcc_amd, arena, wav_pcm, lens):
    cfg = (512, 160, 400)
    ls = fo.ragged_lens(cfg[2], cfg[1]) if lens == "ragged" else fo.uniform_lens(cfg[2], cfg[1])
    with mfcc_amd.MFCC(**_skw(cfg, center=True)) as m:
        _ragged(arena, ls, wav_pcm, m.power_spectrum_packed, m.power_spectrum, "centred %s" % lens)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, center=True) as m:      # the tile-record route
        assert m.kernel_name() == "mfcc_fused512_w12_kernel"
        _ragged(arena, fo.ragged_lens(512, 170), wav_pcm, m.process_packed, m.process, "centred w12 %s" % lens)
