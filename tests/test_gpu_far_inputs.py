"""Every kernel and route reads samples that lie past sample 2^31, sample 2^32 and byte 2^32 of the buffer it is given.

One module-scoped arena of tests/far_offsets.py's layout (2^31 guard elements of the sample type in front of the used
region, 17.2 GB in all) is filled with poison once; a test writes only its channels or utterances and puts the poison
back.  Dense calls take three or four channels of three tiles (37 frames, the last tile partial) on an odd stride just
under 2^31 samples (2^30 for 4-byte samples): one near the base, one straddling each line, one wholly beyond 2^32.  The
result must equal, bit for bit, the same handle's result on a contiguous copy -- a truncated offset reads poison or
another channel's samples, every channel has its own -- and the channel that straddles the farthest line is held to the
kernel's own reference.  Ragged calls take ``offsets[0]`` just under 2^32 and are held to one call per utterance.
tests/test_far_offsets_host.py proves on the CPU that every case crosses its lines and that no truncation leaves the arena.

Measured on an MI355X (pytest --durations=0), 59 tests in 3.8 s: 1.9 s to make and fill the arena once; the slowest
calls are x512 0.14 s, x1024_64 0.09 s and f512 0.09 s; every other test, each decode format, the resampler and every
ragged route included, takes 0.01 s or less.
"""
import numpy as np
import pytest

import far_offsets as fo
import fbank_ref as fr
import kernel_families as kf
import spectrum_ref as sr
from kernel_families import as_np, open_handle, run, same
from oracle import error_bound as eb
from test_gpu_grid_cap import FORMS

pytestmark = pytest.mark.gpu

KINDS = ["speech", "noise", "uniform", "square"]          # one per channel: no two channels hold the same samples
SHAPES = fo.dense_input_shapes()


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


class Arena:
    """The allocation and its views by sample type; ``base`` elements of the type's guard lie in front of a view's used
    region."""

    def __init__(self):
        import torch
        self.words = torch.empty(fo.INPUT_ARENA_WORDS, dtype=torch.int32, device="cuda")
        self.i16 = self.words.view(torch.int16)
        fo.fill(self.i16, fo.POISON_I16)

    def typed(self, dtype):
        import torch
        return self.words.view(getattr(torch, np.dtype(dtype).name))

    def strided(self, x):
        """``x`` (channels, n) written on the dense layout of its sample size: (view, Layout)"""
        import torch
        nch, n = x.shape
        stride, lay = fo.dense_input(n, x.dtype.itemsize)
        assert nch == len(lay.spans) and lay.spans[0].start == 5
        view = torch.as_strided(self.typed(x.dtype), (nch, n), (stride, 1), storage_offset=fo.GUARD + 5)
        view.copy_(torch.from_numpy(x).cuda())
        return view, lay

    def flat(self, utts, offs, lay):
        """The used region as one 1-D int16 tensor with the utterances written at ``offs``."""
        import torch
        flat = self.i16[fo.GUARD:fo.GUARD + lay.used]
        for u, a in zip(utts, offs):
            flat[a:a + len(u)] = torch.from_numpy(np.ascontiguousarray(u)).cuda()
        return flat

    def restore(self, lay):
        """Poison back over what a test wrote (whole half words: the pattern has that period)."""
        import torch
        torch.cuda.synchronize()
        for s in lay.spans:
            a, b = (fo.GUARD + s.start) * lay.esize, (fo.GUARD + s.end) * lay.esize
            self.i16[a // 2:(b + 1) // 2].fill_(fo.POISON_I16)


@pytest.fixture(scope="module")
def arena():
    import torch
    a = Arena()
    yield a
    # the guard was never written: a sample of it at both ends, then free
    assert bool((a.i16[:1 << 20] == fo.POISON_I16).all()) and bool((a.i16[fo.GUARD - (1 << 20):fo.GUARD] == fo.POISON_I16).all())
    del a.i16, a.words
    torch.cuda.empty_cache()


def _inputs(n, seed, wav_pcm, nch=4):
    return np.stack([kf.signal(KINDS[c], n, seed + c, wav_pcm) for c in range(nch)])


def _far_equals_near(arena, x, call, what):
    """``call`` on the far layout of ``x`` and on a contiguous copy: the same bits.  Returns the far result on the host."""
    import torch
    view, lay = arena.strided(x)
    try:
        far = call(view)
        near = call(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert same(far, near), "%s: channels %s apart differ from a contiguous copy" % (what, view.stride(0))
        return as_np(far)
    finally:
        arena.restore(lay)


# ---------------------------------------------------------------------------------------------------- dense: families
@pytest.mark.parametrize("fam", kf.ALL, ids=kf.IDS)
def test_family_reads_far_channels(mfcc_amd, arena, wav_pcm, fam):
    n = SHAPES[fam.id][0]
    x = _inputs(n, 700, wav_pcm)
    with open_handle(mfcc_amd, fam) as m:                         # asserts kernel_name() first
        assert m.num_frames(n) == fo.DENSE_FRAMES
        got = _far_equals_near(arena, x, lambda v: run(m, fam, v), fam.id)
    kf.check_oracle(fam, got[2], x[2], what="far channel")        # the one across sample 2^32


@pytest.mark.parametrize("form", list(FORMS))
def test_fused_form_reads_far_channels(mfcc_amd, arena, wav_pcm, monkeypatch, form):
    kw, env, kernel, _, flen, hop, model, reference = FORMS[form]
    for var in ("MFCC_HIP_FUSED512", "MFCC_HIP_FUSED1024"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    n = SHAPES[form][0]
    assert n == hop * (fo.DENSE_FRAMES - 1) + flen
    x = _inputs(n, 710, wav_pcm)
    with mfcc_amd.MFCC(**kw) as m:
        assert m.kernel_name() == kernel
        assert m.num_frames(n) == fo.DENSE_FRAMES
        got = _far_equals_near(arena, x, m.process, form)
    ref, bound = reference(x[2:3], model)
    eb.check(got[2:3], ref, bound, "%s far channel" % form)


# ---------------------------------------------------------------------------------------------------- dense: spectrum
def _skw(cfg, **over):
    nfft, hop, flen = cfg
    kw = dict(nfft=nfft, hop=hop, nfilters=8, nceptrums=8, power_scale=sr.power_scale_of(nfft))
    if flen != nfft:
        kw["win_length"] = flen
    kw.update(over)
    return kw


SPECTRUM = {"spectrum512_h170": ((512, 170, 512), "mfcc_spectrum512_kernel"),
            "spectrum512_h160": ((512, 160, 400), "mfcc_spectrum512_kernel"),
            "spectrum_generic": ((256, 80, 200), "mfcc_spectrum_generic_kernel")}


@pytest.mark.parametrize("case", list(SPECTRUM))
def test_spectrum_kernel_reads_far_channels(mfcc_amd, arena, wav_pcm, case):
    cfg, kernel = SPECTRUM[case]
    n = SHAPES[case][0]
    x = _inputs(n, 720, wav_pcm)
    with mfcc_amd.MFCC(**_skw(cfg)) as m:
        assert m.spectrum_kernel_name() == kernel
        assert m.num_frames(n) == fo.DENSE_FRAMES
        got = _far_equals_near(arena, x, m.power_spectrum, case)
    ref = sr.reference(x[2], *cfg)
    sr.check(got[2], ref, sr.bound(ref), "%s far channel" % case)


FBANK = {"fbank512_f32_htk80": ((512, 170, 512), "mfcc_fbank512_kernel", lambda: fr.htk_weights(80), "f32"),
         "fbank512_mfma_dense128": ((512, 160, 400), "mfcc_fbank512_kernel", lambda: fr.dense_random(128), "bf16"),
         "fbank_generic": ((256, 80, 200), "mfcc_fbank_generic_kernel", lambda: fr.htk_weights(23, 256), "f32")}


@pytest.mark.parametrize("case", list(FBANK))
def test_filterbank_kernel_reads_far_channels(mfcc_amd, arena, wav_pcm, case):
    cfg, kernel, matrix, form = FBANK[case]
    W = matrix()
    assert fr.form_of(W, kernel) == form
    n = SHAPES[case][0]
    x = _inputs(n, 730, wav_pcm)
    with mfcc_amd.MFCC(**_skw(cfg)) as m:
        m.set_filterbank(W, "energy")
        assert m.filterbank_kernel_name() == kernel
        got = _far_equals_near(arena, x, m.filterbank, case)
    e_ref, b_e = fr.reference_and_bound(x[2], W, *cfg, form=form)
    _, aside = fr.check(got[2], e_ref, b_e, "energy", 0.0, "%s far channel" % case)
    assert aside == 0


# ---------------------------------------------------------------------------------------------------- decode, resample
def _format_inputs(fmt, n, nch):
    rng = np.random.default_rng(741)
    dtype = np.dtype({"s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8, "u8": np.uint8, "i2s32": np.int32, "s32": np.int32,
                      "f32": np.float32}[fmt])
    if dtype == np.float32:
        return (rng.standard_normal((nch, n)) * 0.1).astype(np.float32)
    if fmt == "i2s32":
        return (rng.integers(-3000, 3000, (nch, n)) << 10).astype(np.int32) | 0x155
    if fmt == "s32":
        return (rng.integers(-3000, 3000, (nch, n)) << 16).astype(np.int32) | 0x1234
    if fmt == "u8":
        return rng.integers(96, 160, (nch, n)).astype(np.uint8)
    if dtype == np.uint8:
        return rng.integers(0, 256, (nch, n)).astype(np.uint8)
    return np.clip(np.rint(rng.standard_normal((nch, n)) * 3000), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("fmt", ["s16", "ulaw", "alaw", "u8", "i2s32", "s32", "f32"])
def test_decode_stage_reads_far_rows(mfcc_amd, arena, fmt):
    fam = kf.FLOAT[0]
    n, esize = SHAPES["fmt_" + fmt]
    x = _format_inputs(fmt, n, 3 if esize == 4 else 4)
    assert x.dtype.itemsize == esize
    with open_handle(mfcc_amd, fam, sample_format=fmt) as m:
        got = _far_equals_near(arena, x, m.process, fmt)
    c = len(x) - 2 if esize != 4 else 2                            # the channel across its farthest line
    kf.check_oracle(fam, got[c], mfcc_amd.decode(x[c], fmt), what="far %s channel" % fmt)


def test_resample_stage_reads_far_rows(mfcc_amd, arena, wav_pcm):
    fam = kf.FLOAT[0]
    n = SHAPES["rate_8000"][0]
    x = _inputs(n, 750, wav_pcm)
    with open_handle(mfcc_amd, fam, input_rate=8000) as m:
        assert m.input_rate == 8000
        got = _far_equals_near(arena, x, m.process, "input_rate 8000")
        assert got.shape[1] == m.num_frames(n) >= fo.DENSE_FRAMES - 2
    kf.check_oracle(fam, got[2], mfcc_amd.resample(x[2], 8000, 16000), what="far resampled channel")


# ---------------------------------------------------------------------------------------------------- ragged
def _utterances(lens, wav_pcm, seed=760):
    return [kf.signal(KINDS[i % len(KINDS)], v, seed + i, wav_pcm) for i, v in enumerate(lens)]


def _ragged(arena, lens, wav_pcm, packed, dense, what):
    """``packed(flat, offsets)`` with ``offsets[0]`` just under 2^32 against ``dense(utterance)`` per utterance."""
    import torch
    utts = _utterances(lens, wav_pcm)
    offs, lay = fo.ragged_input(lens)
    flat = arena.flat(utts, offs, lay)
    try:
        rows, fro = packed(flat, np.asarray(offs, np.uint64))
        assert int(fro[0]) == 0
        for i, u in enumerate(utts):
            one = dense(torch.from_numpy(np.ascontiguousarray(u)).cuda())
            assert same(rows[int(fro[i]):int(fro[i + 1])], one), "%s: utterance %d at sample %d differs" % (what, i, offs[i])
        torch.cuda.synchronize()
    finally:
        arena.restore(lay)


RAGGED = [f for f in kf.ALL if f.id in fo.RAGGED_ROUTES]


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("fam", RAGGED, ids=[f.id for f in RAGGED])
def test_ragged_route_reads_far_utterances(mfcc_amd, arena, wav_pcm, fam, pad):
    with open_handle(mfcc_amd, fam, pad) as m:
        _ragged(arena, fo.ragged_lens(fam.nfft, fam.hop), wav_pcm, lambda f, o: m.process_packed(f, o, fixed=fam.fixed),
                lambda u: run(m, fam, u), "%s %s" % (fam.id, pad))


@pytest.mark.parametrize("fam", [kf.FLOAT[0], kf.FIXED[0]], ids=["f512", "x512"])
def test_uniform_route_reads_far_utterances(mfcc_amd, arena, wav_pcm, fam):
    with open_handle(mfcc_amd, fam) as m:
        _ragged(arena, fo.uniform_lens(fam.nfft, fam.hop), wav_pcm, lambda f, o: m.process_packed(f, o, fixed=fam.fixed),
                lambda u: run(m, fam, u), "%s uniform" % fam.id)


@pytest.mark.parametrize("case", ["spectrum512_h170", "spectrum_generic"])
def test_spectrum_packed_reads_far_utterances(mfcc_amd, arena, wav_pcm, case):
    cfg, kernel = SPECTRUM[case]
    with mfcc_amd.MFCC(**_skw(cfg)) as m:
        assert m.spectrum_kernel_name() == kernel
        _ragged(arena, fo.ragged_lens(cfg[2], cfg[1]), wav_pcm, m.power_spectrum_packed, m.power_spectrum, case)


@pytest.mark.parametrize("case", ["fbank512_f32_htk80", "fbank512_mfma_dense128", "fbank_generic"])
def test_filterbank_packed_reads_far_utterances(mfcc_amd, arena, wav_pcm, case):
    cfg, kernel, matrix, _ = FBANK[case]
    with mfcc_amd.MFCC(**_skw(cfg)) as m:
        m.set_filterbank(matrix(), "log2", 1e-10)
        assert m.filterbank_kernel_name() == kernel
        _ragged(arena, fo.ragged_lens(cfg[2], cfg[1]), wav_pcm, m.filterbank_packed, m.filterbank, case)
