"""The filterbank output on the GPU: ``MFCC.set_filterbank`` / ``filterbank`` / ``filterbank_packed`` of both kernels
(mfcc_fbank512_kernel at 512 / 170 and at hop 160, mfcc_fbank_generic_kernel everywhere else and under ``impl="generic"``)
against the float64 reference and the per-element bound of tests/fbank_ref.py, whose docstring has the bound, its
conditions and the exact results.

Every comparison goes through ``fr.check``: it raises on a shape mismatch, a NaN, a negative energy, anything but the exact
result in an all-zero frame or an empty band, and an element over its bound; it returns how many elements the log
condition set aside, and every test here asserts 0.  A test asserts ``filterbank_kernel_name()`` before anything else."""
import ctypes as C

import numpy as np
import pytest

import fbank_ref as fr
import kernel_families as kf
import melbank_ref as mr
import spectrum_ref as sr
from kernel_families import as_np, same

pytestmark = pytest.mark.gpu

FUSED, GENERIC = "mfcc_fbank512_kernel", "mfcc_fbank_generic_kernel"
FUSED_CFGS = [(512, 170, 512), (512, 160, 400)]
SENTINEL = -7.0
FULL_KINDS = ("const_min", "sine8")          # bin-exact under a full-length window: ENERGY scale only there


def _id(cfg):
    return "%d_%d_%d" % cfg[:3]


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


def _open(mfcc_amd, cfg, kernel, W=None, scale="energy", floor=0.0, **over):
    m = mfcc_amd.MFCC(**_kw(cfg, **over))
    try:
        assert m.filterbank_kernel_name() == "" and m.num_bands == 0
        if W is not None:
            m.set_filterbank(W, scale, floor)
            assert m.filterbank_kernel_name() == kernel, "%s: filterbank runs %s, not %s" % (cfg, m.filterbank_kernel_name(), kernel)
            assert m.num_bands == len(W)
    except BaseException:
        m.close()
        raise
    return m


def _kernel_of(cfg, over=()):
    return FUSED if cfg in FUSED_CFGS and dict(over).get("impl") != "generic" else GENERIC


def _strided(x, base=5):
    """``x`` (channels, n) on the device on an odd channel stride behind an odd base offset."""
    import torch
    nch, n = x.shape
    stride = (n | 1) + 2
    flat = np.zeros(base + nch * stride + 16, x.dtype)
    for c in range(nch):
        flat[base + c * stride: base + c * stride + n] = x[c]
    return torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (stride, 1), storage_offset=base)


_REFS = {}


def _inputs(cfg, wav_pcm):
    """(7, n) int16, one channel per kind, 33 notebook frames; its float64 power and all-zero frames per framing --
    computed once per shape and shared, read-only."""
    if cfg not in _REFS:
        x = sr.input_list(*cfg, wav_pcm)
        x.setflags(write=False)
        _REFS[cfg] = (x, {})
    return _REFS[cfg]


def _power(cfg, wav_pcm, pad_mode="notebook", halo=0):
    x, memo = _inputs(cfg, wav_pcm)
    if (pad_mode, halo) not in memo:
        p = sr.reference(x, *cfg, pad_mode=pad_mode, halo=halo)
        z = sr.zero_frames(x, *cfg, pad_mode, halo)
        p.setflags(write=False)
        z.setflags(write=False)
        memo[(pad_mode, halo)] = (p, z)
    return (x,) + memo[(pad_mode, halo)]


def _log_kinds(cfg):
    return [i for i, k in enumerate(sr.KINDS) if cfg[2] != cfg[0] or k not in FULL_KINDS]


def _check(got, p_ref, zero, W, scale, floor, what, kernel=GENERIC):
    """``got`` (channels, frames, bands) against the reference of the channels it was computed from; nothing set aside.
    ``kernel``: what computed it -- the fused kernel contracts a matrix that does not fit its LDS in bf16-split terms and
    is held to that arithmetic's bound then (``fbank_ref.form_of``); everything else to the fp32 chain's."""
    e_ref, b_e = fr.energy_ref_and_bound(p_ref, W, fr.form_of(W, kernel))
    fr.assert_not_blind(b_e, fr.pinned_mask(zero, W), what)
    got = as_np(got)
    assert got.dtype == np.float32
    worst, aside = fr.check(got, e_ref, b_e, scale, floor, what)
    assert aside == 0, "%s: %d element(s) set aside" % (what, aside)
    return worst


def _matrices(nfft=512):
    return [("htk80", fr.htk_weights(80, nfft)), ("htk23", fr.htk_weights(23, nfft, fmin=20.0)), ("htk128", fr.htk_weights(128, nfft)),
            ("edge", fr.edge_band(nfft)), ("dense", fr.dense_random(128, nfft))]


# ---------------------------------------------------------------------------------------------------- matrices, scales
@pytest.mark.parametrize("cfg,over", [((512, 170, 512), {}), ((512, 160, 400), {}), ((512, 170, 512), dict(impl="generic")),
                                      ((512, 160, 400), dict(impl="generic"))], ids=["170", "160_400", "170_generic", "160_400_generic"])
def test_matrices_and_scales_at_512(mfcc_amd, wav_pcm, cfg, over):
    """Every matrix in ENERGY scale on all seven kinds and in LOG2 on the kinds the log bound sees; then the other scales
    and floors on the bank with an empty band."""
    kernel = _kernel_of(cfg, over)
    x, p_ref, zero = _power(cfg, wav_pcm)
    lk = _log_kinds(cfg)
    xd = _strided(x)
    with _open(mfcc_amd, cfg, kernel, **over) as m:
        for name, W in _matrices():
            m.set_filterbank(W, "energy")
            assert m.filterbank_kernel_name() == kernel and m.num_bands == len(W)
            got = m.filterbank(xd)
            assert tuple(got.shape) == (len(x), 33, len(W))
            we = _check(got, p_ref, zero, W, "energy", 0.0, "%s %s energy" % (kernel, name), kernel)
            wl = 0.0
            if name != "edge":              # bins 0 and nfft / 2 alone hold too little of a frame for the log condition
                m.set_filterbank(W, "log2")
                wl = _check(m.filterbank(xd)[lk], p_ref[lk], zero[lk], W, "log2", 0.0, "%s %s log2" % (kernel, name), kernel)
            print("%s %s %s: worst error / bound %.3f (energy), %.3f (log2)" % (cfg, kernel, name, we, wl))
        W = fr.htk_weights(128)
        assert (fr.nnz(W) == 0).sum() == 1 and zero[lk].any()
        for scale, floor in (("ln", 1.1920929e-07), ("log10", 1e-10), ("log2", 1.0)):
            m.set_filterbank(W, scale, floor)
            _check(m.filterbank(xd)[lk], p_ref[lk], zero[lk], W, scale, floor, "%s htk128 %s floor %g" % (kernel, scale, floor))


@pytest.mark.parametrize("cfg,n_bands", [((1024, 341, 1024), 40), ((256, 80, 200), 23), ((64, 21, 64), 7)], ids=["1024", "256_200", "64"])
def test_generic_shapes(mfcc_amd, wav_pcm, cfg, n_bands):
    x, p_ref, zero = _power(cfg, wav_pcm)
    lk = _log_kinds(cfg)
    xd = _strided(x)
    W = fr.htk_weights(n_bands, cfg[0])
    D = fr.dense_random(16, cfg[0])
    with _open(mfcc_amd, cfg, GENERIC) as m:
        for name, w in (("htk%d" % n_bands, W), ("dense16", D), ("edge", fr.edge_band(cfg[0]))):
            m.set_filterbank(w, "energy")
            assert m.filterbank_kernel_name() == GENERIC
            we = _check(m.filterbank(xd), p_ref, zero, w, "energy", 0.0, "%s %s energy" % (cfg, name))
            wl = 0.0
            if name != "edge":
                m.set_filterbank(w, "ln", 1e-10)
                wl = _check(m.filterbank(xd)[lk], p_ref[lk], zero[lk], w, "ln", 1e-10, "%s %s ln" % (cfg, name))
            print("%s generic %s: worst error / bound %.3f (energy), %.3f (ln)" % (cfg, name, we, wl))


@pytest.mark.parametrize("cfg,over", [((512, 170, 512), {}), ((512, 160, 400), {}), ((512, 160, 400), dict(impl="generic")),
                                      ((256, 80, 200), {})], ids=["170", "160_400", "160_400_generic", "256_200"])
def test_selection_matrices_return_the_power_spectrum(mfcc_amd, wav_pcm, cfg, over):
    """Matrices of one 1.0 per band that together pick every bin: the ENERGY rows against ``power_spectrum`` of the same
    call within G * P (G = 2 * 2^-24: one weight) -- a wrong bin map, column 16 (bins 16 + 32 j) or the duplicates of
    column 0 show here."""
    kernel = _kernel_of(cfg, over)
    x, _, _ = _power(cfg, wav_pcm)
    xd = _strided(x)
    seen = np.zeros(cfg[0] // 2 + 1, int)
    with _open(mfcc_amd, cfg, kernel, **over) as m:
        power = as_np(m.power_spectrum(xd)).astype(np.float64)
        for idx, W in fr.selections(cfg[0]):
            m.set_filterbank(W, "energy")
            assert m.filterbank_kernel_name() == kernel
            got = as_np(m.filterbank(xd)).astype(np.float64)
            want = power[..., idx]
            bad = np.abs(got - want) > 2.0 * fr.U * want
            assert not bad.any(), "%s: bins %s differ from power_spectrum" % (cfg, sorted(set(idx[np.argwhere(bad)[:, -1]].tolist())))
            seen[idx] += 1
    assert (seen >= 1).all()


@pytest.mark.parametrize("cfg", FUSED_CFGS, ids=_id)
def test_wide_selection_matrices_on_the_mfma_form(mfcc_amd, wav_pcm, cfg):
    """Two 1.0 per band, half a spectrum apart, that together pick every bin: bands too wide for the fused kernel's LDS,
    so its MFMA form contracts them.  The ENERGY rows against the sum of the two ``power_spectrum`` values of the same
    call within G * E (the bf16 form's G at two weights) -- a wrong (block, K step) list, operand layout or bin shows
    here, bins 0 and 256 and the step past bin 256 included."""
    x, _, _ = _power(cfg, wav_pcm)
    xd = _strided(x)
    seen = np.zeros(257, int)
    with _open(mfcc_amd, cfg, FUSED) as m:
        power = as_np(m.power_spectrum(xd)).astype(np.float64)
        for idx, idx2, W in fr.wide_selections():
            assert fr.form_of(W, FUSED) == "bf16"
            m.set_filterbank(W, "energy")
            assert m.filterbank_kernel_name() == FUSED
            got = as_np(m.filterbank(xd)).astype(np.float64)
            want = power[..., idx] + power[..., idx2]
            bad = np.abs(got - want) > fr.g_of(W, "bf16") * want
            assert not bad.any(), "%s: bands %s differ from power_spectrum" % (cfg, sorted(set(np.argwhere(bad)[:, -1].tolist()))[:32])
            seen[idx] += 1
            seen[idx2] += 1
    assert (seen >= 2).all()


@pytest.mark.parametrize("cfg", FUSED_CFGS, ids=_id)
def test_mfma_form_shapes_and_out_views(mfcc_amd, wav_pcm, cfg):
    """The MFMA form of the fused kernel (dense matrices of 23, 127 and 13 bands: partial blocks, an empty second block
    of a wave) at frames per channel 1, 15, 16, 17, 33 x channels 1, 3, in ``out=`` views offset by 0..3 floats inside
    sentinels; all four scales; bit-identical rows from a ragged call."""
    import torch
    nfft, hop, flen = cfg
    x, p_ref, zero = _power(cfg, wav_pcm)
    lk = _log_kinds(cfg)
    with _open(mfcc_amd, cfg, FUSED) as m:
        for n_bands in (23, 127, 13):
            W = fr.dense_random(n_bands, nfft, seed=n_bands)
            W[n_bands // 2] = 0.0                                  # an empty band inside
            assert fr.form_of(W, FUSED) == "bf16"
            m.set_filterbank(W, "energy")
            for frames in (1, 15, 16, 17, 33):
                n = sr.samples_for(frames, flen, hop)
                for nch in (1, 3):
                    xs = _strided(x[:nch, :n])
                    count = nch * frames * n_bands
                    off = (frames + nch) % 4
                    buf = torch.full((count + 11,), SENTINEL, dtype=torch.float32, device="cuda")
                    view = buf[off:off + count].view(nch, frames, n_bands)
                    m.filterbank(xs, out=view)
                    _check(view, p_ref[:nch, :frames], zero[:nch, :frames], W, "energy", 0.0,
                           "mfma form %d bands, %d frames x %d channels" % (n_bands, frames, nch), FUSED)
                    assert same(view, m.filterbank(xs))
                    outside = torch.cat([buf[:off], buf[off + count:]])
                    assert bool((outside == SENTINEL).all()), "%s: out= at offset %d wrote outside its view" % (cfg, off)
        xd = _strided(x)
        for scale, floor in (("log2", 0.0), ("ln", 1.1920929e-07), ("log10", 1e-10)):
            m.set_filterbank(W, scale, floor)
            got = m.filterbank(xd)
            _check(got[lk], p_ref[lk], zero[lk], W, scale, floor, "mfma form %s floor %g" % (scale, floor), FUSED)
        n = x.shape[1]
        rows, fo = m.filterbank_packed(torch.from_numpy(np.concatenate([x[1], x[2, :n - 777]])).cuda(), [0, n, 2 * n - 777])
        assert same(rows[:int(fo[1])], got[1]) and same(rows[int(fo[1]):], m.filterbank(torch.from_numpy(x[2, :n - 777].copy()).cuda()))


# ---------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("cfg", FUSED_CFGS + [(256, 80, 200)], ids=_id)
def test_shapes_and_out_views(mfcc_amd, wav_pcm, cfg):
    """Frames per channel 1, 15, 16, 17, 33 x channels 1, 3 on an odd channel stride behind an odd base offset; then
    ``out=`` views offset by 0..3 floats inside sentinels, at row widths (23, 127) that move the alignment from row to row."""
    import torch
    nfft, hop, flen = cfg
    kernel = _kernel_of(cfg)
    x, p_ref, zero = _power(cfg, wav_pcm)
    W = fr.htk_weights(80 if nfft == 512 else 23, nfft)
    with _open(mfcc_amd, cfg, kernel, W, "energy") as m:
        for frames in (1, 15, 16, 17, 33):
            n = sr.samples_for(frames, flen, hop)
            for nch in (1, 3):
                got = m.filterbank(_strided(x[:nch, :n]))
                assert tuple(got.shape) == (nch, frames, len(W))
                _check(got, p_ref[:nch, :frames], zero[:nch, :frames], W, "energy", 0.0, "%s %d frames x %d channels" % (kernel, frames, nch))
        for n_bands in (23, 127):
            Wn = fr.htk_weights(n_bands, nfft)
            m.set_filterbank(Wn, "log2", 1e-10)
            for frames, nch in ((17, 3), (1, 1)):
                xs = _strided(x[:nch, :sr.samples_for(frames, flen, hop)])
                plain = m.filterbank(xs)
                count = nch * frames * n_bands
                for off in range(4):
                    buf = torch.full((count + 11,), SENTINEL, dtype=torch.float32, device="cuda")
                    view = buf[off:off + count].view(nch, frames, n_bands)
                    back = m.filterbank(xs, out=view)
                    assert back.data_ptr() == view.data_ptr()
                    assert same(view, plain), "%s: out= at offset %d differs" % (cfg, off)
                    outside = torch.cat([buf[:off], buf[off + count:]])
                    assert bool((outside == SENTINEL).all()), "%s: out= at offset %d wrote outside its view" % (cfg, off)
        one = m.filterbank(torch.from_numpy(x[0, :sr.samples_for(17, flen, hop)].copy()).cuda())
        assert tuple(one.shape) == (17, 127)


# ---------------------------------------------------------------------------------------------------- padding, halo
@pytest.mark.parametrize("cfg", FUSED_CFGS + [(256, 80, 200)], ids=_id)
def test_stream_padding_and_halo(mfcc_amd, wav_pcm, cfg):
    nfft, hop, flen = cfg
    kernel = _kernel_of(cfg)
    W = fr.htk_weights(128 if nfft == 512 else 23, nfft)
    silences = sr.KINDS.index("silences")
    lk = _log_kinds(cfg)
    for pad_mode, halo in (("stream", 0), ("notebook", 1), ("stream", 1)):
        x, p_ref, zero = _power(cfg, wav_pcm, pad_mode, halo)
        with _open(mfcc_amd, cfg, kernel, W, "energy", pad_mode=pad_mode) as m:
            got = m.filterbank(_strided(x), halo=halo)
            assert got.shape[1] == sr.num_frames(x.shape[1] - halo, flen, hop, pad_mode)
            _check(got, p_ref, zero, W, "energy", 0.0, "%s %s halo %d" % (kernel, pad_mode, halo))
            assert zero[silences].any()
            z = as_np(got)[silences][zero[silences]]
            assert z.size and not z.any() and not np.signbit(z).any()              # +0.0, bit for bit
            m.set_filterbank(W, "log2", 0.0)
            got = m.filterbank(_strided(x), halo=halo)
            _check(got[lk], p_ref[lk], zero[lk], W, "log2", 0.0, "%s %s halo %d log2" % (kernel, pad_mode, halo))
            assert np.isneginf(as_np(got)[silences][zero[silences]]).all()


# ---------------------------------------------------------------------------------------------------- ragged
@pytest.mark.parametrize("cfg", FUSED_CFGS + [(256, 80, 200)], ids=_id)
@pytest.mark.parametrize("pad_mode", ["notebook", "stream"])
def test_ragged_is_bit_identical_to_dense_calls(mfcc_amd, wav_pcm, cfg, pad_mode):
    import torch
    from mfcc_amd import _lib as L
    nfft, hop, flen = cfg
    kernel = _kernel_of(cfg)
    W = fr.htk_weights(80 if nfft == 512 else 23, nfft)
    lengths = [0, 1, flen - 1, flen, flen + hop - 1, flen + hop, sr.samples_for(5 * 16 + 3, flen, hop)]
    utts = [kf.signal(sr.KINDS[i % 6], max(n, 1), 31 + i, wav_pcm)[:n] for i, n in enumerate(lengths)]
    flat = torch.from_numpy(np.concatenate(utts)).cuda()
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    with _open(mfcc_amd, cfg, kernel, W, "log10", 1e-10, pad_mode=pad_mode) as m:
        want_fo = np.concatenate([[0], np.cumsum([m.num_frames(n) for n in lengths])])
        rows, fo = m.filterbank_packed(flat, offsets)
        assert np.array_equal(np.asarray(fo, np.int64), want_fo) and tuple(rows.shape) == (int(want_fo[-1]), len(W))
        for u, x in enumerate(utts):
            if want_fo[u + 1] == want_fo[u]:
                continue
            dense = m.filterbank(torch.from_numpy(np.ascontiguousarray(x)).cuda())
            assert same(rows[int(fo[u]):int(fo[u + 1])], dense), "%s: utterance %d (%d samples) differs" % (cfg, u, len(x))
        # equal lengths run as channels
        eq = torch.from_numpy(np.concatenate([utts[-1][:3000], utts[-1][3000:6000]])).cuda()
        rows_eq, fo_eq = m.filterbank_packed(eq, [0, 3000, 6000])
        assert same(rows_eq, m.filterbank(eq.view(2, 3000)).reshape(-1, len(W)))
        # the longest utterance against the reference as well
        p_ref = sr.reference(utts[-1], *cfg, pad_mode=pad_mode)
        zero = sr.zero_frames(utts[-1], *cfg, pad_mode, 0)
        _check(rows[int(fo[-2]):], p_ref, zero, W, "log10", 1e-10, "ragged %s" % (cfg,))
        # capacity 0: BUFFER_SMALL, with the frame offsets a caller sizes its buffer by
        fo0 = np.full(len(lengths) + 1, 99, np.uint64)
        rc = m._call(flat.device, "fbank_ragged_i16_dev", m._h, L.ptr(flat), L.ptr(offsets), len(lengths), None, 0,
                     L.ptr(fo0), ok=(L.ERROR_BUFFER_SMALL,))
        assert rc == L.ERROR_BUFFER_SMALL and np.array_equal(fo0.astype(np.int64), want_fo)
        out = torch.full((int(want_fo[-1]), len(W)), SENTINEL, dtype=torch.float32, device="cuda")
        rows2, _ = m.filterbank_packed(flat, offsets, out=out)
        assert rows2.data_ptr() == out.data_ptr() and same(out, rows)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- steady state
_STEADY = {}


def _steady_inputs(cfg, cu, wav_pcm):
    """The batch of ``spectrum_ref.steady_shape`` with its float64 power and all-zero frames: computed once per
    configuration and shared by both contraction forms, read-only."""
    if cfg not in _STEADY:
        nfft, hop, flen = cfg
        tpc, frames, nch = sr.steady_shape(cu)
        x = sr.batch_inputs(nfft, hop, flen, wav_pcm, nch, frames)
        p_ref, zero = sr.reference(x, nfft, hop, flen), sr.zero_frames(x, nfft, hop, flen, "notebook", 0)
        for a in (x, p_ref, zero):
            a.setflags(write=False)
        _STEADY[cfg] = (x, p_ref, zero)
    return _STEADY[cfg]


def _steady_state(mfcc_amd, wav_pcm, cfg, W, what):
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    tpc, frames, nch = sr.steady_shape(cu)
    per_slice = max(1, (cu // 2) // tpc)
    x, p_ref, zero = _steady_inputs(cfg, cu, wav_pcm)
    view = _strided(x)
    with _open(mfcc_amd, cfg, FUSED, W, "energy") as m:
        assert m.num_frames(x.shape[1]) == frames
        whole = m.filterbank(view)
        assert tuple(whole.shape) == (nch, frames, len(W))
        parts = [m.filterbank(view[a:a + per_slice]) for a in range(0, nch, per_slice)]
        torch.cuda.synchronize()
    assert same(whole, torch.cat(parts)), "%s: the batch differs from its slices" % (cfg,)
    worst = _check(whole, p_ref, zero, W, "energy", 0.0, "steady state %s %s" % (what, cfg), FUSED)
    print("steady state %s %s: %d channels, worst error / bound %.3f" % (what, cfg, nch, worst))


@pytest.mark.parametrize("cfg", FUSED_CFGS, ids=_id)
def test_steady_state_of_the_tile_loop(mfcc_amd, wav_pcm, cfg):
    """The batch of ``spectrum_ref.steady_shape``: workgroups run a first, a middle and a last tile; bit-identical to slices
    where no workgroup gets a second tile, and within bound, at 80 bands (weights in LDS: the fp32 contraction)."""
    W = fr.htk_weights(80)
    assert fr.form_of(W, FUSED) == "f32"
    _steady_state(mfcc_amd, wav_pcm, cfg, W, "htk80")


@pytest.mark.parametrize("cfg", FUSED_CFGS, ids=_id)
def test_steady_state_of_the_tile_loop_on_the_mfma_form(mfcc_amd, wav_pcm, cfg):
    """The same batch through the other tail of the shared tile loop: a dense 128 x 257 matrix, whose weights do not fit
    the LDS, so the MFMA contraction runs behind every first, middle and last tile."""
    W = fr.dense_random(128)
    assert fr.form_of(W, FUSED) != "f32"
    _steady_state(mfcc_amd, wav_pcm, cfg, W, "dense128")


# ---------------------------------------------------------------------------------------------------- entry points
@pytest.mark.parametrize("cfg", [(512, 170, 512), (512, 160, 400), (256, 80, 200)], ids=_id)
def test_host_call_equals_device_call_also_in_chunks(mfcc_amd, wav_pcm, monkeypatch, cfg):
    """The host entry, whole and through the copy pipeline in 1 MB chunks: whole channels per chunk and the frame-range
    chunks of one long channel."""
    import torch
    kernel = _kernel_of(cfg)
    W = fr.htk_weights(80 if cfg[0] == 512 else 23, cfg[0])
    x17, _, _ = _power(cfg, wav_pcm)
    x17 = np.ascontiguousarray(x17[:, :sr.samples_for(17, cfg[2], cfg[1])])
    chans = np.stack([kf.signal(k, 600_000, 41 + i, wav_pcm) for i, k in enumerate(("speech", "silences", "uniform"))])
    long = kf.signal("silences", 1_500_000, 47, wav_pcm)
    with _open(mfcc_amd, cfg, kernel, W, "log2", 1e-10, pad_mode="stream") as m:
        host = m.filterbank(x17)
        assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.shape == (len(x17), m.num_frames(x17.shape[1]), len(W))
        assert same(host, m.filterbank(torch.from_numpy(x17).cuda())) and same(m.filterbank(x17[2]), host[2])
        dev_c = m.filterbank(torch.from_numpy(chans).cuda())
        dev_l = m.filterbank(torch.from_numpy(long).cuda())
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        host_c, host_l = m.filterbank(chans), m.filterbank(long)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
    assert same(host_c, dev_c), "%s: channels in chunks differ from the device call" % (cfg,)
    assert same(host_l, dev_l), "%s: frame-range chunks differ" % (cfg,)


def test_sample_format_and_input_rate_apply(mfcc_amd, wav_pcm):
    import torch
    cfg = (512, 160, 400)
    W = fr.htk_weights(80)
    pcm = wav_pcm[3000:3000 + 6000]
    ulaw = np.random.default_rng(5).integers(0, 256, 6000).astype(np.uint8)
    with _open(mfcc_amd, cfg, FUSED, W, "log2") as plain:
        with _open(mfcc_amd, cfg, FUSED, W, "log2", sample_format="ulaw") as m:
            want = plain.filterbank(mfcc_amd.decode(ulaw, "ulaw"))
            assert same(m.filterbank(ulaw), want)
            assert same(m.filterbank(torch.from_numpy(ulaw).cuda()), want)
        with _open(mfcc_amd, cfg, FUSED, W, "log2", input_rate=8000) as m:
            want = plain.filterbank(mfcc_amd.resample(pcm, 8000, 16000))
            assert m.num_frames(len(pcm)) == len(want)
            assert same(m.filterbank(pcm), want)
            assert same(m.filterbank(torch.from_numpy(np.ascontiguousarray(pcm)).cuda()), want)
            rows, fo = m.filterbank_packed(torch.from_numpy(np.concatenate([pcm, pcm[:2500]])).cuda(), [0, 6000, 8500])
            assert same(rows[:int(fo[1])], want)


def test_settings_that_do_not_apply_are_ignored(mfcc_amd, wav_pcm):
    import torch
    cfg = (512, 160, 400)
    W = fr.htk_weights(80)
    x = torch.from_numpy(np.ascontiguousarray(_inputs(cfg, wav_pcm)[0][:, :sr.samples_for(17, 400, 160)])).cuda()
    with _open(mfcc_amd, cfg, FUSED, W, "ln", 1e-10) as plain:
        want, want_halo = plain.filterbank(x), plain.filterbank(x, halo=1)
        want_packed, want_fo = plain.filterbank_packed(x.reshape(-1), [0, 3000, 7000])
    busy = dict(nfilters=40, nceptrums=13, output="logmel", mel="htk", fmin=20.0, normalize="meanvar", deltas=2, pcen=True)
    with _open(mfcc_amd, cfg, FUSED, W, "ln", 1e-10, **busy) as m:
        assert m.num_features == 120
        assert same(m.filterbank(x), want) and same(m.filterbank(x, halo=1), want_halo)
        rows, fo = m.filterbank_packed(x.reshape(-1), [0, 3000, 7000])
        assert same(rows, want_packed) and np.array_equal(fo, want_fo)
        # ... and the handle is what it was: its own output and the spectrum still have their widths
        assert tuple(m.process(x).shape) == (x.shape[0], 17, 120)
        assert tuple(m.power_spectrum(x).shape) == (x.shape[0], 17, 257)
    with _open(mfcc_amd, cfg, FUSED, W, "ln", 1e-10, vad="select") as m:
        assert same(m.filterbank(x), want)


def test_replacing_the_matrix_between_enqueued_calls(mfcc_amd, wav_pcm):
    """Two calls enqueued back to back with another matrix each, no synchronization in between: each has its own result;
    then the matrix is removed."""
    import torch
    cfg = (512, 170, 512)
    x = torch.from_numpy(np.stack([kf.signal("speech", 400_000, 3 + i, wav_pcm) for i in range(8)])).cuda()
    A, B = fr.htk_weights(80), fr.dense_random(128)
    for over in ({}, dict(impl="generic")):
        with _open(mfcc_amd, cfg, _kernel_of(cfg, over), **over) as m:
            m.set_filterbank(A, "log2")
            want_a = m.filterbank(x).clone()
            m.set_filterbank(B, "energy")
            want_b = m.filterbank(x).clone()
            torch.cuda.synchronize()
            m.set_filterbank(A, "log2")
            got_a = m.filterbank(x)
            m.set_filterbank(B, "energy")
            got_b = m.filterbank(x)
            m.set_filterbank(None)
            torch.cuda.synchronize()
            assert same(got_a, want_a) and same(got_b, want_b)
            assert m.num_bands == 0 and m.filterbank_kernel_name() == ""
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                m.filterbank(x)
            assert e.value.code == mfcc_amd._lib.ERROR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------- the product
def test_consistent_with_the_log_mel_output(mfcc_amd, wav_pcm):
    """400 / 160 / 512, HTK 40 bands from 20 Hz: with W the handle's own MEL_DENSE table and scale log2, the rows sit
    within the sum of both bounds of that handle's ``output="logmel"`` rows."""
    import torch
    from mfcc_amd import _lib as L
    cfg = (512, 160, 400)
    kw = dict(nfilters=40, nceptrums=13, mel="htk", fmin=20.0, fmax=8000.0, output="logmel")
    x = np.stack([kf.signal(k, sr.samples_for(33, 400, 160), 21 + i, wav_pcm) for i, k in enumerate(("speech", "noise", "uniform"))])
    W = mfcc_amd.get_table(L.TABLE_MEL_DENSE_F32, win_length=400, mel="htk", fmin=20.0, fmax=8000.0, nfft=512, hop=160,
                           nfilters=40, nceptrums=13).reshape(40, 257)
    e_ref, b_e = fr.reference_and_bound(x, W, *cfg)
    _, fb_bound, kept = fr.log_ref_and_bound(e_ref, b_e, "log2", 0.0)
    assert kept.all()
    for over, model in ((dict(), "bf16x2/fp32"), (dict(impl="generic"), "fp32/fp32")):
        _, lm_bound = mr.reference_and_bound(x, model, 400, 160, nfft=512, n_mel=40, n_cep=13, output="logmel", low=20.0, high=8000.0)
        with _open(mfcc_amd, cfg, _kernel_of(cfg, over), W, "log2", **dict(kw, **over)) as m:
            xd = torch.from_numpy(x).cuda()
            a, b = as_np(m.filterbank(xd)).astype(np.float64), as_np(m.process(xd)).astype(np.float64)
        assert a.shape == b.shape == (3, 33, 40) and np.isfinite(a).all() and np.isfinite(b).all()
        r = np.abs(a - b) / (fb_bound + lm_bound)
        assert r.max() <= 1.0, "filterbank and log-mel rows differ by %.3g x the sum of their bounds" % r.max()
        print("consistency %s: worst difference / (both bounds) %.3f" % (model, r.max()))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(mfcc_amd, wav_pcm):
    import torch
    from mfcc_amd import _lib as L
    lib = L.load()
    x = torch.from_numpy(wav_pcm[:4000].copy()).cuda()
    got = C.c_size_t(0)
    W = fr.htk_weights(80)
    with _open(mfcc_amd, (512, 170, 512), FUSED) as m:
        nf = m.num_frames(4000)
        out = torch.empty((1, nf, 80), dtype=torch.float32, device="cuda")
        call, rag = lib.mfcc_hip_fbank_i16_dev, lib.mfcc_hip_fbank_ragged_i16_dev
        off, fo = np.array([0, 4000], np.uint64), np.zeros(2, np.uint64)
        # no matrix: UNSUPPORTED from every compute entry
        assert call(m._h, L.ptr(x), 4000, 4000, 1, 0, L.ptr(out), C.byref(got)) == L.ERROR_UNSUPPORTED
        assert rag(m._h, L.ptr(x), L.ptr(off), 1, L.ptr(out), out.numel(), L.ptr(fo)) == L.ERROR_UNSUPPORTED
        host = np.empty(nf * 80, np.float32)
        assert lib.mfcc_hip_fbank_i16(m._h, L.ptr(wav_pcm[:4000].copy()), 4000, 1, L.ptr(host), host.size, C.byref(got)) == L.ERROR_UNSUPPORTED
        with pytest.raises(mfcc_amd.MfccHipError):
            m.filterbank(x)
        # what mfcc_hip_set_fbank refuses leaves the handle as it was
        good = L.Fbank(struct_size=32, n_bands=80, scale=L.FBANK_LOG2, floor=0.0)
        bads = [L.Fbank(struct_size=28, n_bands=80, scale=1), L.Fbank(struct_size=32, n_bands=0, scale=1),
                L.Fbank(struct_size=32, n_bands=129, scale=1), L.Fbank(struct_size=32, n_bands=80, scale=4),
                L.Fbank(struct_size=32, n_bands=80, scale=-1), L.Fbank(struct_size=32, n_bands=80, scale=1, floor=-1.0),
                L.Fbank(struct_size=32, n_bands=80, scale=1, floor=float("nan")), L.Fbank(struct_size=32, n_bands=80, scale=1, floor=float("inf"))]
        res = L.Fbank(struct_size=32, n_bands=80, scale=1)
        res.reserved[2] = 1
        for p in bads + [res]:
            assert lib.mfcc_hip_set_fbank(m._h, C.byref(p), L.ptr(W)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_set_fbank(m._h, C.byref(good), None) == L.ERROR_INVALID_PARAM
        for v in (np.nan, np.inf, -1e-30):
            w = W.copy()
            w[79, 256] = v
            assert lib.mfcc_hip_set_fbank(m._h, C.byref(good), L.ptr(w)) == L.ERROR_INVALID_PARAM
        assert m.num_bands == 0
        with pytest.raises(ValueError):
            m.set_filterbank(W[:, :256])
        m.set_filterbank(W, "log2")
        assert lib.mfcc_hip_set_fbank(m._h, C.byref(bads[2]), L.ptr(W)) == L.ERROR_INVALID_PARAM and m.num_bands == 80
        # the spectrum's refusals
        assert call(m._h, None, 4000, 4000, 1, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM
        assert call(m._h, L.ptr(x), 4000, 4000, 1, 0, None, C.byref(got)) == L.ERROR_INVALID_PARAM
        assert call(m._h, L.ptr(x), 3999, 4000, 1, 2, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM      # halo = 2
        assert call(m._h, L.ptr(x), 2000, 1000, 2, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM      # stride < n
        assert call(m._h, L.ptr(x), 4000, 4000, 1, 0, out.data_ptr() + 2, C.byref(got)) == L.ERROR_INVALID_PARAM   # misaligned
        assert call(m._h, L.ptr(x), 1 << 60, 1 << 60, 1, 0, L.ptr(out), C.byref(got)) == L.ERROR_INVALID_PARAM
        assert lib.mfcc_hip_fbank_i16(m._h, L.ptr(wav_pcm[:4000].copy()), 4000, 1, L.ptr(host), host.size - 1,
                                      C.byref(got)) == L.ERROR_BUFFER_SMALL and got.value == nf
        assert rag(m._h, L.ptr(x), None, 1, L.ptr(out), out.numel(), L.ptr(fo)) == L.ERROR_INVALID_PARAM
        assert rag(m._h, L.ptr(x), L.ptr(off[::-1].copy()), 1, L.ptr(out), out.numel(), L.ptr(fo)) == L.ERROR_INVALID_PARAM
        huge = np.array([0, 1 << 60], np.uint64)
        assert rag(m._h, L.ptr(x), L.ptr(huge), 1, L.ptr(out), (1 << 64) - 1, L.ptr(fo)) == L.ERROR_INVALID_PARAM
        # the Python layer
        with pytest.raises(ValueError, match="halo"):
            m.filterbank(x, halo=2)
        with pytest.raises(TypeError):
            m.filterbank(torch.from_numpy(wav_pcm[:4000].copy()))           # a torch tensor on the wrong device
        for bad in (torch.empty((1, nf, 79), dtype=torch.float32, device="cuda"), torch.empty((1, nf, 80), dtype=torch.float64, device="cuda"),
                    torch.empty((1, nf, 80), dtype=torch.float32), torch.empty((1, nf, 257), dtype=torch.float32, device="cuda")):
            with pytest.raises(ValueError, match="out must be"):
                m.filterbank(x, out=bad)
        with pytest.raises(TypeError):
            m.filterbank(x, fixed=True)
        assert not [s for s in L.SYMBOLS if "fbank" in s and "fixed" in s]
        assert tuple(m.filterbank(x).shape) == (nf, 80)
