"""The power-spectrum output on the GPU: ``MFCC.power_spectrum`` / ``power_spectrum_packed`` of both kernels
(mfcc_spectrum512_kernel at 512 / 170 and at hop 160, mfcc_spectrum_generic_kernel everywhere else) against the float64
reference and the per-element bound of tests/spectrum_ref.py, whose docstring has the bound, the measured constant
C_SPEC = 8 and the not-blind conditions.

Every comparison goes through ``sr.check``: it raises on a shape mismatch, a NaN, a negative value, anything but +0.0 in
an all-zero frame, and an element over its bound.  A test asserts ``spectrum_kernel_name()`` before anything else, so that
a handle rerouted to the other kernel fails loudly instead of testing the wrong code."""
import ctypes as C

import numpy as np
import pytest

import kernel_families as kf
import logmel_bound as lb
import spectrum_ref as sr
from kernel_families import as_np, same
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu

FUSED, GENERIC = "mfcc_spectrum512_kernel", "mfcc_spectrum_generic_kernel"
# (nfft, hop, frame length) -> the kernel the handle must report
FUSED_CFGS = [(512, 170, 512), (512, 160, 400), (512, 160, 160), (512, 160, 512)]
GENERIC_CFGS = [(64, 21, 64), (256, 80, 200), (1024, 341, 1024), (512, 171, 512)]
SENTINEL = -7.0


def _id(cfg):
    return "%d_%d_%d" % cfg


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _kw(cfg, **over):
    nfft, hop, flen = cfg
    kw = dict(nfft=nfft, hop=hop, nfilters=8, nceptrums=8, power_scale=sr.power_scale_of(nfft))
    if flen != nfft:
        kw["win_length"] = flen
    kw.update(over)
    return kw


def _open(mfcc_amd, cfg, kernel, **over):
    m = mfcc_amd.MFCC(**_kw(cfg, **over))
    name = m.spectrum_kernel_name()
    if name != kernel:
        m.close()
        raise AssertionError("%s: power_spectrum runs %s, not %s" % (cfg, name, kernel))
    assert m.num_bins == cfg[0] // 2 + 1 == mfcc_amd.spectrum_bins(**{k: v for k, v in _kw(cfg).items() if k != "win_length"})
    return m


def _strided(x, base=5):
    """``x`` (channels, n) on the device on an odd channel stride behind an odd base offset."""
    import torch
    nch, n = x.shape
    stride = (n | 1) + 2
    flat = np.zeros(base + nch * stride + 16, x.dtype)
    for c in range(nch):
        flat[base + c * stride: base + c * stride + n] = x[c]
    return torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (stride, 1), storage_offset=base)


def _check(got, x, cfg, what, pad_mode="notebook", halo=0, ref=None):
    nfft, hop, flen = cfg
    if ref is None:
        ref = sr.reference(x, nfft, hop, flen, pad_mode=pad_mode, halo=halo)
    b = sr.bound(ref)
    zero = sr.zero_frames(x, nfft, hop, flen, pad_mode, halo)
    sr.assert_not_blind(b, zero, what)
    got = as_np(got)
    assert got.dtype == np.float32
    return sr.check(got, ref, b, what), zero


# ---------------------------------------------------------------------------------------------------- golden wav
def test_golden_wav_through_both_kernels(mfcc_amd, wav_pcm):
    import torch
    cfg = (512, 170, 512)
    ref = sr.reference(wav_pcm)
    x = torch.from_numpy(np.ascontiguousarray(wav_pcm)).cuda()
    for kernel, over in ((FUSED, {}), (GENERIC, dict(impl="generic"))):
        with _open(mfcc_amd, cfg, kernel, nfilters=32, nceptrums=13, **over) as m:
            got = m.power_spectrum(x)
            assert tuple(got.shape) == (1046, 257)
            worst, zero = _check(got, wav_pcm, cfg, "golden wav " + kernel, ref=ref)
        print("golden wav %s: worst error / bound %.3f, %d all-zero frames" % (kernel, worst, int(zero.sum())))


# ---------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("cfg", FUSED_CFGS + GENERIC_CFGS, ids=_id)
def test_shapes(mfcc_amd, wav_pcm, cfg):
    """Frames per channel 1, 15, 16, 17, 33 x channels 1, 3, 6 (the six kinds) on an odd channel stride behind an odd base
    offset; then ``out=`` views offset by 0..3 floats inside a buffer of sentinels."""
    import torch
    nfft, hop, flen = cfg
    kernel = FUSED if cfg in FUSED_CFGS else GENERIC
    full = sr.input_list(nfft, hop, flen, wav_pcm)[:6]
    ref_full = sr.reference(full, nfft, hop, flen)              # the frames of a prefix are a prefix of these
    worst = 0.0
    with _open(mfcc_amd, cfg, kernel) as m:
        for frames in (1, 15, 16, 17, 33):
            n = sr.samples_for(frames, flen, hop)
            for nch in (1, 3, 6):
                x = full[:nch, :n]
                got = m.power_spectrum(_strided(x))
                assert tuple(got.shape) == (nch, frames, m.num_bins)
                w, _ = _check(got, x, cfg, "%s %d frames x %d channels" % (kernel, frames, nch), ref=ref_full[:nch, :frames])
                worst = max(worst, w)
        # out= at every alignment of a row's first float mod 16 bytes; nothing outside the view may change
        for frames, nch in ((17, 3), (1, 1)):
            x = _strided(full[:nch, :sr.samples_for(frames, flen, hop)])
            plain = m.power_spectrum(x)
            count = nch * frames * m.num_bins
            for off in range(4):
                buf = torch.full((count + 11,), SENTINEL, dtype=torch.float32, device="cuda")
                view = buf[off:off + count].view(nch, frames, m.num_bins)
                back = m.power_spectrum(x, out=view)
                assert back.data_ptr() == view.data_ptr()
                assert same(view, plain), "%s: out= at offset %d differs" % (cfg, off)
                outside = torch.cat([buf[:off], buf[off + count:]])
                assert bool((outside == SENTINEL).all()), "%s: out= at offset %d wrote outside its view" % (cfg, off)
        # a 1-D channel comes back as (frames, bins)
        one = m.power_spectrum(torch.from_numpy(full[0, :sr.samples_for(17, flen, hop)].copy()).cuda())
        assert tuple(one.shape) == (17, m.num_bins)
    print("shapes %s %s: worst error / bound %.3f" % (cfg, kernel, worst))


def test_impl_generic_selects_the_generic_kernel_at_512(mfcc_amd, wav_pcm):
    for cfg in ((512, 170, 512), (512, 160, 400)):
        x = sr.input_list(*cfg, wav_pcm)[:3]
        with _open(mfcc_amd, cfg, GENERIC, impl="generic") as m:
            _check(m.power_spectrum(_strided(x)), x, cfg, "impl=generic %s" % (cfg,))


# ---------------------------------------------------------------------------------------------------- padding, halo
@pytest.mark.parametrize("cfg", [(512, 170, 512), (512, 160, 400), (256, 80, 200), (1024, 341, 1024)], ids=_id)
def test_stream_padding_and_halo(mfcc_amd, wav_pcm, cfg):
    nfft, hop, flen = cfg
    kernel = FUSED if cfg in FUSED_CFGS else GENERIC
    x = sr.input_list(nfft, hop, flen, wav_pcm)
    silences = sr.KINDS.index("silences")
    for pad_mode, halo in (("stream", 0), ("notebook", 1), ("stream", 1)):
        with _open(mfcc_amd, cfg, kernel, pad_mode=pad_mode) as m:
            got = m.power_spectrum(_strided(x), halo=halo)
            assert got.shape[1] == sr.num_frames(x.shape[1] - halo, flen, hop, pad_mode)
            worst, zero = _check(got, x, cfg, "%s %s halo %d" % (kernel, pad_mode, halo), pad_mode, halo)
        assert zero[silences].any(), "the silences channel has no all-zero frame"
        z = as_np(got)[silences][zero[silences]]
        assert z.size and not z.any() and not np.signbit(z).any()              # +0.0, bit for bit
        print("%s %s %s halo %d: worst error / bound %.3f, %d all-zero frames" % (cfg, kernel, pad_mode, halo, worst, zero.sum()))


# ---------------------------------------------------------------------------------------------------- ragged
@pytest.mark.parametrize("cfg", [(512, 170, 512), (512, 160, 400), (256, 80, 200)], ids=_id)
@pytest.mark.parametrize("pad_mode", ["notebook", "stream"])
def test_ragged_is_bit_identical_to_dense_calls(mfcc_amd, wav_pcm, cfg, pad_mode):
    import torch
    from mfcc_amd import _lib as L
    nfft, hop, flen = cfg
    kernel = FUSED if cfg in FUSED_CFGS else GENERIC
    lengths = [0, 1, flen - 1, flen, flen + hop - 1, flen + hop, sr.samples_for(5 * 16 + 3, flen, hop)]
    utts = [kf.signal(sr.KINDS[i % 6], max(n, 1), 31 + i, wav_pcm)[:n] for i, n in enumerate(lengths)]
    flat = torch.from_numpy(np.concatenate(utts)).cuda()
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    with _open(mfcc_amd, cfg, kernel, pad_mode=pad_mode) as m:
        # the library's own frame counts (tests/test_cabi_host.py, tests/test_framed_host.py hold them to the oracle)
        want_fo = np.concatenate([[0], np.cumsum([m.num_frames(n) for n in lengths])])
        assert all(m.num_frames(n) == sr.num_frames(n, flen, hop, pad_mode) for n in lengths if n >= flen)
        rows, fo = m.power_spectrum_packed(flat, offsets)
        assert np.array_equal(np.asarray(fo, np.int64), want_fo) and tuple(rows.shape) == (int(want_fo[-1]), m.num_bins)
        for u, x in enumerate(utts):
            if want_fo[u + 1] == want_fo[u]:
                continue
            dense = m.power_spectrum(torch.from_numpy(np.ascontiguousarray(x)).cuda())
            assert same(rows[int(fo[u]):int(fo[u + 1])], dense), "%s: utterance %d (%d samples) differs" % (cfg, u, len(x))
        # the longest utterance against the reference as well
        _check(rows[int(fo[-2]):], utts[-1], cfg, "ragged %s" % (cfg,), pad_mode)
        # capacity 0: BUFFER_SMALL, with the frame offsets a caller sizes its buffer by
        fo0 = np.full(len(lengths) + 1, 99, np.uint64)
        rc = m._call(flat.device, "spectrum_ragged_i16_dev", m._h, L.ptr(flat), L.ptr(offsets), len(lengths), None, 0,
                     L.ptr(fo0), ok=(L.ERROR_BUFFER_SMALL,))
        assert rc == L.ERROR_BUFFER_SMALL and np.array_equal(fo0.astype(np.int64), want_fo)
        # out= of the right shape is filled in place
        out = torch.full((int(want_fo[-1]), m.num_bins), SENTINEL, dtype=torch.float32, device="cuda")
        rows2, _ = m.power_spectrum_packed(flat, offsets, out=out)
        assert rows2.data_ptr() == out.data_ptr() and same(out, rows)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- steady state
@pytest.mark.parametrize("cfg", [(512, 170, 512), (512, 160, 400)], ids=_id)
def test_steady_state_of_the_tile_loop(mfcc_amd, wav_pcm, cfg):
    """The batch shape of tests/test_gpu_steady_state.py: channels of three tiles, the last one partial, about 4.5 x CUs
    tiles, so that workgroups run a first, a middle and a last tile; bit-identical to slices where no workgroup gets a
    second tile, and within bound."""
    import torch
    nfft, hop, flen = cfg
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    tpc, frames, nch = sr.steady_shape(cu)
    n_tiles, stride = nch * tpc, 2 * cu                      # launch_geom.hpp: kTwoPerCu
    three = min(stride, n_tiles - 2 * stride)                # workgroups that run three tiles
    assert stride % tpc and three >= 1, (cu, tpc, nch, three)
    per_slice = max(1, (cu // 2) // tpc)                     # channels of a slice: at most CUs / 2 tiles
    assert per_slice * tpc <= max(tpc, cu // 2)
    x = sr.batch_inputs(nfft, hop, flen, wav_pcm, nch, frames)
    view = _strided(x)
    with _open(mfcc_amd, cfg, FUSED) as m:
        assert m.num_frames(x.shape[1]) == frames
        whole = m.power_spectrum(view)
        assert tuple(whole.shape) == (nch, frames, 257)
        parts = [m.power_spectrum(view[a:a + per_slice]) for a in range(0, nch, per_slice)]
        torch.cuda.synchronize()
    assert same(whole, torch.cat(parts)), "%s: the batch differs from its slices" % (cfg,)
    worst, zero = _check(whole, x, cfg, "steady state %s" % (cfg,))
    print("steady state %s: %d channels, %d three-tile workgroups, worst error / bound %.3f, %d all-zero frames"
          % (cfg, nch, three, worst, int(zero.sum())))


# ---------------------------------------------------------------------------------------------------- entry points
@pytest.mark.parametrize("cfg", [(512, 170, 512), (256, 80, 200)], ids=_id)
def test_host_call_equals_device_call(mfcc_amd, wav_pcm, cfg):
    import torch
    kernel = FUSED if cfg in FUSED_CFGS else GENERIC
    x = sr.input_list(*cfg, wav_pcm, frames=17)
    with _open(mfcc_amd, cfg, kernel) as m:
        host = m.power_spectrum(x)
        assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.shape == (len(x), 17, m.num_bins)
        assert same(host, m.power_spectrum(torch.from_numpy(x).cuda()))
        assert same(m.power_spectrum(x[2]), host[2])


@pytest.mark.parametrize("cfg", [(512, 170, 512), (512, 160, 400), (256, 80, 200)], ids=_id)
def test_host_call_in_chunks_equals_device_call(mfcc_amd, wav_pcm, monkeypatch, cfg):
    """The host entry's copy pipeline with 1 MB chunks: whole channels per chunk (three channels of 1.2 MB) and the
    frame-range chunks of one long channel, each with its halo sample and a forced frame count."""
    import torch
    kernel = FUSED if cfg in FUSED_CFGS else GENERIC
    chans = np.stack([kf.signal(k, 600_000, 41 + i, wav_pcm) for i, k in enumerate(("speech", "silences", "uniform"))])
    long = kf.signal("silences", 1_500_000, 47, wav_pcm)
    for pad_mode in ("notebook", "stream"):
        with _open(mfcc_amd, cfg, kernel, pad_mode=pad_mode) as m:
            dev_c = m.power_spectrum(torch.from_numpy(chans).cuda())
            dev_l = m.power_spectrum(torch.from_numpy(long).cuda())
            whole_l = m.power_spectrum(long)
            monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
            host_c, host_l = m.power_spectrum(chans), m.power_spectrum(long)
            monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        assert same(host_c, dev_c), "%s %s: channels in chunks differ from the device call" % (cfg, pad_mode)
        assert same(host_l, dev_l) and same(whole_l, dev_l), "%s %s: frame-range chunks differ" % (cfg, pad_mode)


def test_sample_format_and_input_rate_apply(mfcc_amd, wav_pcm):
    import torch
    cfg = (512, 160, 400)
    pcm = wav_pcm[3000:3000 + 6000]
    ulaw = np.random.default_rng(5).integers(0, 256, 6000).astype(np.uint8)
    with _open(mfcc_amd, cfg, FUSED) as plain:
        with _open(mfcc_amd, cfg, FUSED, sample_format="ulaw") as m:
            want = plain.power_spectrum(mfcc_amd.decode(ulaw, "ulaw"))
            assert same(m.power_spectrum(ulaw), want)
            assert same(m.power_spectrum(torch.from_numpy(ulaw).cuda()), want)
        with _open(mfcc_amd, cfg, FUSED, input_rate=8000) as m:
            want = plain.power_spectrum(mfcc_amd.resample(pcm, 8000, 16000))
            assert m.num_frames(len(pcm)) == len(want)
            assert same(m.power_spectrum(pcm), want)
            assert same(m.power_spectrum(torch.from_numpy(np.ascontiguousarray(pcm)).cuda()), want)
        with _open(mfcc_amd, cfg, FUSED, sample_format="ulaw", input_rate=8000) as m:
            want = plain.power_spectrum(mfcc_amd.resample(mfcc_amd.decode(ulaw, "ulaw"), 8000, 16000))
            assert same(m.power_spectrum(torch.from_numpy(ulaw).cuda()), want)
            rows, fo = m.power_spectrum_packed(torch.from_numpy(np.concatenate([ulaw, ulaw[:2500]])).cuda(), [0, 6000, 8500])
            assert same(rows[:int(fo[1])], want)


def test_settings_that_do_not_apply_are_ignored(mfcc_amd, wav_pcm):
    import torch
    cfg = (512, 160, 400)
    x = torch.from_numpy(sr.input_list(*cfg, wav_pcm, frames=17)).cuda()
    with _open(mfcc_amd, cfg, FUSED) as plain:
        want = plain.power_spectrum(x)
        want_packed, want_fo = plain.power_spectrum_packed(x.reshape(-1), [0, 3000, 7000])
    busy = dict(nfilters=40, nceptrums=13, output="logmel", mel="htk", fmin=20.0, normalize="meanvar", deltas=2, pcen=True)
    with _open(mfcc_amd, cfg, FUSED, **busy) as m:
        assert m.num_features == 120
        assert same(m.power_spectrum(x), want)
        assert same(m.power_spectrum(x, halo=1), plain_halo(mfcc_amd, cfg, x))
        rows, fo = m.power_spectrum_packed(x.reshape(-1), [0, 3000, 7000])
        assert same(rows, want_packed) and np.array_equal(fo, want_fo)
        # ... and the handle is what it was: its own output still has its width and its passes
        feats = m.process(x)
        assert tuple(feats.shape) == (x.shape[0], 17, 120)
    with _open(mfcc_amd, cfg, FUSED, vad="select") as m:
        assert same(m.power_spectrum(x), want)


def plain_halo(mfcc_amd, cfg, x):
    with _open(mfcc_amd, cfg, FUSED) as plain:
        return plain.power_spectrum(x, halo=1)


# ---------------------------------------------------------------------------------------------------- the product
def test_consistent_with_the_log_mel_output(mfcc_amd, wav_pcm):
    """512 / 170 / 32: log2(power @ W.T) with the library's own mel matrix, contracted in float64 on the host, is held to
    the log-mel reference of tests/logmel_bound.py under its fp32 model -- the new output against the one the suite
    already trusts."""
    import torch
    from mfcc_amd import _lib as L
    cfg = (512, 170, 512)
    x = np.stack([kf.signal(k, sr.samples_for(33, 512, 170), 21 + i, wav_pcm) for i, k in enumerate(("speech", "noise", "uniform"))])
    W = mfcc_amd.get_table(L.TABLE_MEL_DENSE_F32, nfft=512, nfilters=32, nceptrums=13).reshape(32, 257).astype(np.float64)
    ref, bound = lb.reference_and_bound(x, "fp32/fp32", nfft=512, hop=170, n_mel=32, sample_rate=16000, power_scale=512.0)
    for kernel, over in ((FUSED, {}), (GENERIC, dict(impl="generic"))):
        with _open(mfcc_amd, cfg, kernel, nfilters=32, nceptrums=13, **over) as m:
            power = as_np(m.power_spectrum(torch.from_numpy(x).cuda())).astype(np.float64)
        with np.errstate(divide="ignore"):
            logmel = np.log2(power @ W.T)
        worst = eb.check(logmel, ref, bound, "log2(power @ W.T) " + kernel)
        print("consistency %s: worst error / log-mel bound %.3f" % (kernel, worst))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(mfcc_amd, wav_pcm):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    x = torch.from_numpy(wav_pcm[:4000].copy()).cuda()
    got = C.c_size_t(0)
    with _open(mfcc_amd, (512, 170, 512), FUSED) as m:
        nf, bins = m.num_frames(4000), m.num_bins
        out = torch.empty((1, nf, bins), dtype=torch.float32, device="cuda")
        call = lib.mfcc_hip_spectrum_i16_dev
        assert call(None, L.ptr(x), 4000, 4000, 1, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM
        assert call(m._h, None, 4000, 4000, 1, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM
        assert call(m._h, L.ptr(x), 4000, 4000, 1, 0, None, C.byref(got)) == L.ERROR_INVALID_PARAM
        assert call(m._h, L.ptr(x), 3999, 4000, 1, 2, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM      # halo = 2
        assert call(m._h, L.ptr(x), 3999, 4000, 1, -1, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM
        assert call(m._h, L.ptr(x), 2000, 1000, 2, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM      # stride < n
        assert call(m._h, L.ptr(x), 4000, 4000, 1, 0, out.data_ptr() + 2, C.byref(got)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_spectrum_i16(m._h, None, 4000, 1, None, 0, C.byref(got)) == L.ERROR_INVALID_PARAM
        host = np.empty(nf * bins - 1, np.float32)
        assert lib.mfcc_hip_spectrum_i16(m._h, L.ptr(wav_pcm[:4000].copy()), 4000, 1, L.ptr(host), host.size,
                                         C.byref(got)) == L.ERROR_BUFFER_SMALL and got.value == nf
        fo = np.zeros(2, np.uint64)
        off = np.array([0, 4000], np.uint64)
        rag = lib.mfcc_hip_spectrum_ragged_i16_dev
        assert rag(m._h, L.ptr(x), None, 1, L.ptr(out), out.numel(), L.ptr(fo)) == L.ERROR_INVALID_PARAM
        assert rag(m._h, L.ptr(x), L.ptr(off), 1, L.ptr(out), out.numel(), None) == L.ERROR_INVALID_PARAM
        assert rag(m._h, None, L.ptr(off), 1, L.ptr(out), out.numel(), L.ptr(fo)) == L.ERROR_INVALID_PARAM
        assert rag(m._h, L.ptr(x), L.ptr(off[::-1].copy()), 1, L.ptr(out), out.numel(), L.ptr(fo)) == L.ERROR_INVALID_PARAM
        # rows x bins beyond the limit of spectrum_plan.hpp: refused, whatever the capacity says
        huge = np.array([0, 1 << 60], np.uint64)
        assert rag(m._h, L.ptr(x), L.ptr(huge), 1, L.ptr(out), (1 << 64) - 1, L.ptr(fo)) == L.ERROR_INVALID_PARAM
        assert call(m._h, L.ptr(x), 1 << 60, 1 << 60, 1, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM
        # the Python layer
        with pytest.raises(ValueError, match="halo"):
            m.power_spectrum(x, halo=2)
        with pytest.raises(TypeError):
            m.power_spectrum(torch.from_numpy(wav_pcm[:4000].copy()))           # a torch tensor on the wrong device
        with pytest.raises(TypeError):
            m.power_spectrum(x.to(torch.int32))
        for bad in (torch.empty((1, nf, bins - 1), dtype=torch.float32, device="cuda"),
                    torch.empty((1, nf + 1, bins), dtype=torch.float32, device="cuda"),
                    torch.empty((1, nf, bins), dtype=torch.float64, device="cuda"),
                    torch.empty((1, nf, bins), dtype=torch.float32),
                    torch.empty((1, nf, 2 * bins), dtype=torch.float32, device="cuda")[:, :, ::2]):
            with pytest.raises(ValueError, match="out must be"):
                m.power_spectrum(x, out=bad)
        with pytest.raises(ValueError, match="out must be"):
            m.power_spectrum_packed(x, [0, 4000], out=torch.empty((nf, m.num_features), dtype=torch.float32, device="cuda"))
        # there is no fixed-point form: no entry, no argument
        assert not [s for s in L.SYMBOLS if "spectrum" in s and "fixed" in s]
        with pytest.raises(TypeError):
            m.power_spectrum(x, fixed=True)
        with pytest.raises(TypeError):
            m.power_spectrum_packed(x, [0, 4000], fixed=True)
        # the handle still works afterwards
        assert tuple(m.power_spectrum(x).shape) == (nf, bins)
    with _open(mfcc_amd, (512, 160, 400), FUSED, input_rate=8000) as m:
        with pytest.raises(mfcc_amd.MfccHipError) as e:                          # as process: a rated handle takes no halo
            m.power_spectrum(x, halo=1)
        assert e.value.code == L.ERROR_UNSUPPORTED
