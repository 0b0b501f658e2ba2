"""The front of a handle -- window function and pre-emphasis pair -- on the GPU: which kernel serves which front, every
output of every kernel family against the float64 reference of tests/front_ref.py under the bounds the project already
has (``oracle.error_bound`` / ``logmel_bound`` for cepstra and log-mel rows, ``spectrum_ref.bound`` for power rows,
tests/fbank_ref.py for band energies), the bit identities of the contract, and the fixed path's refusals.

Inputs are ``spectrum_ref.input_list`` (seven kinds x 33 frames) under the three framings of ``spectrum_ref.FRAMINGS``:
a workgroup's first tile, a steady tile, a partial tile and the ``halo`` path.  The hop-160 forms also get one
``spectrum_ref.steady_shape`` batch.  Every test asserts the kernel's name first, so that a handle rerouted to another
kernel fails loudly instead of testing the wrong code."""
import os

import numpy as np
import pytest

import fbank_ref as fb
import front_ref as fr
import kernel_families as kf
import melbank_ref as mr
import spectrum_ref as sr
from kernel_families import as_np, same
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu

GENERIC = "mfcc_float_generic_kernel"
H160, MB, W4, W12, F1K = ("mfcc_fused512_h160_kernel", "mfcc_fused512_h160_mb_kernel", "mfcc_fused512_kernel",
                          "mfcc_fused512_w12_kernel", "mfcc_fused1024_w12bf_kernel")
SPEC_FUSED, SPEC_GENERIC = "mfcc_spectrum512_kernel", "mfcc_spectrum_generic_kernel"
FB_FUSED, FB_GENERIC = "mfcc_fbank512_kernel", "mfcc_fbank_generic_kernel"
# the arithmetic of each kernel, read from its source (oracle/error_bound.py: MODELS)
MODEL = {GENERIC: "fp32/fp32", H160: "bf16x2/fp32", MB: "bf16x2/fp32", W4: "bf16x2/fp32", W12: "bf16x2/bf16x2",
         F1K: "bf16x2/fp32"}

# the shapes of the parity tests: handle arguments, and the kernel of (the default front, a non-default front whose pair
# the fused kernels serve); a pair beyond num + den = 127 runs the generic kernel everywhere
SHAPES = {
    "asr32": (dict(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=13), (H160, H160)),
    "htk40_logmel": (dict(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13, mel="htk", fmin=20.0,
                          output="logmel"), (MB, MB)),
    "cep170": (dict(nfft=512, hop=170, nfilters=32, nceptrums=13), (W12, W4)),
    "g200": (dict(nfft=256, hop=80, win_length=200, nfilters=20, nceptrums=13, power_scale=0), (GENERIC, GENERIC)),
    "g1024": (dict(nfft=1024, hop=341, nfilters=40, nceptrums=13, power_scale=0), (F1K, GENERIC)),
}
NONDEFAULT = [f for f in fr.FRONTS if not fr.is_default(f)]
HANN0 = ("hann", True, (0, 1))


def kernel_for(front, shape):
    if fr.is_default(front):
        return SHAPES[shape][1][0]
    return SHAPES[shape][1][1] if fr.fused_pair(front) else GENERIC


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _geom(kw):
    nfft = kw["nfft"]
    hop = kw.get("hop") or nfft // 3
    ps = kw.get("power_scale", 512.0)
    return nfft, hop, kw.get("win_length", nfft), float(ps) if ps else float(nfft)


def _open(mfcc_amd, kw, front, kernel=None, **over):
    m = mfcc_amd.MFCC(**dict(kw, **fr.front_kw(front)), **over)
    if kernel is not None and m.kernel_name() != kernel:
        name = m.kernel_name()
        m.close()
        raise AssertionError("%s %s: the handle runs %s, not %s" % (fr.front_id(front), kw, name, kernel))
    return m


def _filters(kw):
    nfft, _, _, _ = _geom(kw)
    if kw.get("mel") == "htk":
        return mr.matrix(nfft, kw["nfilters"], 16000, kw.get("fmin", 0.0), kw.get("fmax"))
    return None


_REFS = {}


def _reference(x, kw, front, model, pad, halo):
    """reference and bound of a batch; computed once per (samples, handle, front, model, framing) and left unchanged"""
    key = (x.tobytes(), x.shape, tuple(sorted(kw.items(), key=str)), front, model, pad, halo)
    if key not in _REFS:
        nfft, hop, L, ps = _geom(kw)
        ref, bound = fr.reference_and_bound(x, model, front, L, hop, nfft, kw["nfilters"], 16000, ps, kw["nceptrums"], pad,
                                            halo, kw.get("output", "cepstra"), _filters(kw))
        ref.setflags(write=False)
        bound.setflags(write=False)
        _REFS[key] = (ref, bound)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------- 1. kernel choice
def test_kernel_choice(mfcc_amd):
    U = mfcc_amd._lib.ERROR_UNSUPPORTED
    for front in fr.FRONTS:
        for shape, (kw, _) in SHAPES.items():
            with _open(mfcc_amd, kw, front) as m:
                assert m.kernel_name() == kernel_for(front, shape), (fr.front_id(front), shape, m.kernel_name())
                fused = fr.fused_pair(front) and kw["nfft"] == 512
                assert m.spectrum_kernel_name() == (SPEC_FUSED if fused else SPEC_GENERIC), (fr.front_id(front), shape)
                m.set_filterbank(np.ones((3, kw["nfft"] // 2 + 1), np.float32), "energy")
                assert m.filterbank_kernel_name() == (FB_FUSED if fused else FB_GENERIC), (fr.front_id(front), shape)
                assert m.front == (front[0], front[1], front[2])
    asr, htk, cep, _, big = (SHAPES[s][0] for s in SHAPES)
    with _open(mfcc_amd, asr, HANN0) as m:
        assert m.kernel_name() == H160
    with _open(mfcc_amd, htk, HANN0) as m:
        assert m.kernel_name() == MB
    with _open(mfcc_amd, dict(htk, output="cepstra"), HANN0) as m:
        assert m.kernel_name() == MB
    with _open(mfcc_amd, cep, HANN0) as m:
        assert m.kernel_name() == W4
    with _open(mfcc_amd, dict(cep, output="logmel"), HANN0) as m:         # the four-wave form has no log-mel tail
        assert m.kernel_name() == GENERIC
    with _open(mfcc_amd, big, HANN0) as m:
        assert m.kernel_name() == GENERIC
    with _open(mfcc_amd, dict(big, output="logmel"), HANN0) as m:
        assert m.kernel_name() == GENERIC
    # the fused limit num + den = 127 is served, 128 is not
    with _open(mfcc_amd, asr, ("hann", True, (63, 64))) as m:
        assert m.kernel_name() == H160 and m.spectrum_kernel_name() == SPEC_FUSED
    with _open(mfcc_amd, asr, ("hann", True, (63, 65))) as m:
        assert m.kernel_name() == GENERIC and m.spectrum_kernel_name() == SPEC_GENERIC
    # impl: GENERIC forces, FUSED512 means a fused 512 kernel or UNSUPPORTED
    for kw in (asr, htk, cep):
        with _open(mfcc_amd, kw, HANN0, impl="generic") as m:
            assert m.kernel_name() == GENERIC and m.spectrum_kernel_name() == SPEC_GENERIC
        with _open(mfcc_amd, kw, HANN0, impl="fused512") as m:
            assert m.kernel_name() == kernel_for(HANN0, [s for s in SHAPES if SHAPES[s][0] is kw][0])
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            _open(mfcc_amd, kw, ("hamming", False, (97, 100)), impl="fused512")
        assert e.value.code == U
    for kw in (dict(cep, output="logmel"), big):
        with pytest.raises(mfcc_amd.MfccHipError) as e:
            _open(mfcc_amd, kw, HANN0, impl="fused512")
        assert e.value.code == U
    # the default front written out is the plain handle
    for shape, (kw, _) in SHAPES.items():
        for front in (fr.DEFAULT, ("hamming", True, (62, 64))):
            with _open(mfcc_amd, kw, front) as m:
                assert m.kernel_name() == SHAPES[shape][1][0] and m.front == fr.DEFAULT


# ---------------------------------------------------------------------------------------------------- 2. parity
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("front", fr.FRONTS, ids=fr.front_id)
def test_rows_meet_the_fronted_reference(mfcc_amd, wav_pcm, front, shape):
    """Cepstra / log-mel rows of every kernel family: every value of every frame, all three framings."""
    kw, _ = SHAPES[shape]
    kernel = kernel_for(front, shape)
    nfft, hop, L, _ = _geom(kw)
    x = sr.input_list(nfft, hop, L, wav_pcm)
    got = {}
    for pad, halo in sr.FRAMINGS:
        with _open(mfcc_amd, kw, front, kernel, pad_mode=pad) as m:
            got[(pad, halo)] = as_np(m.process(_dev(x), halo=halo))
    worst = 0.0
    for (pad, halo), g in got.items():
        ref, bound = _reference(x, kw, front, MODEL[kernel], pad, halo)
        assert g.shape == ref.shape and g.dtype == np.float32
        # speech, noise, uniform: the reference bounds every frame
        assert not np.isposinf(bound[:3]).any(), (fr.front_id(front), shape, pad, halo)
        worst = max(worst, eb.check(g, ref, bound, "%s %s %s halo %d" % (fr.front_id(front), shape, pad, halo)))
    print("%s %s (%s): worst error / bound %.3f" % (fr.front_id(front), shape, kernel, worst))


POWER_CFGS = [(512, 160, 400), (512, 170, 512), (256, 80, 200), (1024, 341, 1024)]


def _power_kw(cfg, **over):
    nfft, hop, L = cfg
    kw = dict(nfft=nfft, hop=hop, nfilters=8, nceptrums=8, power_scale=sr.power_scale_of(nfft))
    if L != nfft:
        kw["win_length"] = L
    return dict(kw, **over)


_P_REFS = {}


def _power_ref(x, front, cfg, pad, halo):
    key = (x.tobytes(), x.shape, front, cfg, pad, halo)
    if key not in _P_REFS:
        nfft, hop, L = cfg
        ref = fr.power_reference(x, front, nfft, hop, L, pad_mode=pad, halo=halo)
        ref.setflags(write=False)
        _P_REFS[key] = (ref, fr.zero_frames(x, front, nfft, hop, L, pad, halo))
    return _P_REFS[key]


@pytest.mark.parametrize("cfg", POWER_CFGS, ids=lambda c: "%d_%d_%d" % c)
@pytest.mark.parametrize("front", fr.FRONTS, ids=fr.front_id)
def test_power_spectrum_meets_the_fronted_reference(mfcc_amd, wav_pcm, front, cfg):
    nfft, hop, L = cfg
    kernel = SPEC_FUSED if nfft == 512 and fr.fused_pair(front) else SPEC_GENERIC
    x = sr.input_list(nfft, hop, L, wav_pcm)
    worst = 0.0
    for pad, halo in sr.FRAMINGS:
        with _open(mfcc_amd, _power_kw(cfg), front, pad_mode=pad) as m:
            assert m.spectrum_kernel_name() == kernel
            got = as_np(m.power_spectrum(_dev(x), halo=halo))
        ref, zero = _power_ref(x, front, cfg, pad, halo)
        b = sr.bound(ref)
        sr.assert_not_blind(b, zero, fr.front_id(front))
        assert got.dtype == np.float32
        worst = max(worst, sr.check(got, ref, b, "%s %s %s halo %d" % (fr.front_id(front), cfg, pad, halo)))
    if nfft == 512 and kernel == SPEC_FUSED and not fr.is_default(front):       # the generic kernel on the same shape
        with _open(mfcc_amd, _power_kw(cfg, impl="generic"), front) as m:
            assert m.spectrum_kernel_name() == SPEC_GENERIC
            got = as_np(m.power_spectrum(_dev(x)))
        ref, _ = _power_ref(x, front, cfg, "notebook", 0)
        worst = max(worst, sr.check(got, ref, sr.bound(ref), "%s %s generic" % (fr.front_id(front), cfg)))
    print("%s %s (%s): worst error / bound %.3f" % (fr.front_id(front), cfg, kernel, worst))


_W = {}
BROADBAND = ("speech", "noise", "uniform", "silences")


def _matrices():
    if not _W:
        _W["htk80_ln"] = (fb.htk_weights(80), "ln", 1e-10)
        _W["htk80_energy"] = (fb.htk_weights(80), "energy", 0.0)
        _W["dense128"] = (fb.dense_random(128), "energy", 0.0)
    return _W


@pytest.mark.parametrize("cfg", POWER_CFGS[:2], ids=lambda c: "%d_%d_%d" % c)
@pytest.mark.parametrize("front", fr.FRONTS, ids=fr.front_id)
def test_filterbank_meets_the_fronted_reference(mfcc_amd, wav_pcm, front, cfg):
    """HTK 80 in ``ln`` scale and a dense 128 x 257 matrix (the fused kernel's MFMA form), on the fused kernel where the
    front's pair lets it run and on the generic one.

    fbank_ref's log comparison takes an element only when ``B_E <= E_ref / 4`` and counts the others.  On the broadband
    channels (speech, noise, uniform, noise with silences) that count must be 0 at every front, as in
    tests/test_gpu_fbank.py.  The line spectra (square, constant, sine) under a low-side-lobe window and without
    pre-emphasis leave most bands with nothing but the side lobes of a line, 100 dB and more below it: their logarithm is
    below what an fp32 FFT resolves (measured on the CPU, from the reference alone: up to 1980 of 2640 elements of such a
    channel under Blackman).  So the same matrix also runs in ENERGY scale, where EVERY element of every channel is held
    under ``B_E``."""
    nfft, hop, L = cfg
    x = sr.input_list(nfft, hop, L, wav_pcm)
    runs = [({}, FB_FUSED if fr.fused_pair(front) else FB_GENERIC)]
    if fr.fused_pair(front) and not fr.is_default(front):
        runs.append((dict(impl="generic"), FB_GENERIC))
    for over, kernel in runs:
        for pad, halo in (sr.FRAMINGS if not over else sr.FRAMINGS[:1]):
            with _open(mfcc_amd, _power_kw(cfg, **over), front, pad_mode=pad) as m:
                for name, (W, scale, floor) in _matrices().items():
                    m.set_filterbank(W, scale, floor)
                    assert m.filterbank_kernel_name() == kernel, (fr.front_id(front), cfg, over)
                    got = as_np(m.filterbank(_dev(x), halo=halo))
                    p_ref, zero = _power_ref(x, front, cfg, pad, halo)
                    e_ref, b_e = fb.energy_ref_and_bound(p_ref, W, fb.form_of(W, kernel))
                    fb.assert_not_blind(b_e, fb.pinned_mask(zero, W), name)
                    worst, aside = fb.check(got, e_ref, b_e, scale, floor,
                                            "%s %s %s %s %s halo %d" % (fr.front_id(front), cfg, name, kernel, pad, halo))
                    if scale != "energy":
                        live = [i for i, k in enumerate(sr.KINDS) if k in BROADBAND]
                        assert fb.check(got[live], e_ref[live], b_e[live], scale, floor, name)[1] == 0
                    print("%s %s %s (%s) %s halo %d: worst error / bound %.3f, %d set aside"
                          % (fr.front_id(front), cfg, name, kernel, pad, halo, worst, aside))


@pytest.mark.parametrize("shape", ["asr32", "htk40_logmel"])
@pytest.mark.parametrize("front", [HANN0, ("povey", False, (32, 33))], ids=fr.front_id)
def test_steady_state_of_the_hop160_forms(mfcc_amd, wav_pcm, front, shape):
    """The batch shape of tests/test_gpu_steady_state.py: workgroups that run a first, a middle and a last tile; rows,
    power and bands of the same batch."""
    import torch
    kw, _ = SHAPES[shape]
    kernel = kernel_for(front, shape)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    _, frames, nch = sr.steady_shape(cu)
    x = sr.batch_inputs(512, 160, 400, wav_pcm, nch, frames)
    with _open(mfcc_amd, kw, front, kernel) as m:
        assert m.spectrum_kernel_name() == SPEC_FUSED
        got = as_np(m.process(_dev(x)))
        power = as_np(m.power_spectrum(_dev(x)))
        W, scale, floor = _matrices()["htk80_ln"]
        m.set_filterbank(W, scale, floor)
        assert m.filterbank_kernel_name() == FB_FUSED
        bands = as_np(m.filterbank(_dev(x)))
    ref, bound = _reference(x, kw, front, MODEL[kernel], "notebook", 0)
    worst = eb.check(got, ref, bound, "steady %s %s" % (fr.front_id(front), shape))
    p_ref, zero = _power_ref(x, front, (512, 160, 400), "notebook", 0)
    worst_p = sr.check(power, p_ref, sr.bound(p_ref), "steady power %s" % fr.front_id(front))
    e_ref, b_e = fb.energy_ref_and_bound(p_ref, W, fb.form_of(W, FB_FUSED))
    worst_b, _ = fb.check(bands, e_ref, b_e, scale, floor, "steady bands %s" % fr.front_id(front))
    live = [i for i in range(nch) if sr.KINDS[i % len(sr.KINDS)] in BROADBAND]
    assert fb.check(bands[live], e_ref[live], b_e[live], scale, floor, "steady bands")[1] == 0
    print("steady %s %s: %d channels, worst error / bound rows %.3f, power %.3f, bands %.3f"
          % (fr.front_id(front), shape, nch, worst, worst_p, worst_b))


# ---------------------------------------------------------------------------------------------------- 3. bit identities
@pytest.mark.parametrize("shape", list(SHAPES))
def test_default_front_written_out_is_the_plain_handle(mfcc_amd, wav_pcm, shape):
    import torch
    kw, (kernel, _) = SHAPES[shape]
    nfft, hop, L, _ = _geom(kw)
    x = sr.input_list(nfft, hop, L, wav_pcm)
    utts = [x[1], x[0][: L + 5 * hop + 3], x[2][: L]]
    flat = np.concatenate(utts)
    offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint64)
    W = fb.htk_weights(80, nfft)

    def outputs(m):
        assert m.kernel_name() == kernel
        m.set_filterbank(W, "ln", 1e-10)
        out = [m.process(x), m.process(_dev(x)), m.process(_dev(x), halo=1), m.power_spectrum(_dev(x)),
               m.power_spectrum(x[:2]), m.filterbank(_dev(x)), m.filterbank(x[:2])]
        out += list(m.process_batch(utts)) + list(m.process_batch([_dev(u) for u in utts]))
        out += [m.process_packed(_dev(flat), offs)[0], m.power_spectrum_packed(_dev(flat), offs)[0],
                m.filterbank_packed(_dev(flat), offs)[0]]
        with m.stream() as s:
            out += [s.push(x[0][:1000]), s.push(x[0][1000:]), s.flush()]
        with m.stream_bank(2) as b:
            out += list(b.push([x[0], x[1][:999]])) + list(b.flush())
        torch.cuda.synchronize()
        return [as_np(o) for o in out]

    with mfcc_amd.MFCC(**kw) as plain:
        want = outputs(plain)
    for front in (fr.DEFAULT, ("hamming", True, (62, 64)), ("hamming", True, 0.96875)):
        with _open(mfcc_amd, kw, front) as m:
            got = outputs(m)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), (shape, front, i)


# Hann is 0 at sample 0, which hides the history sample's only product whatever the pair: the rectangular window does not
@pytest.mark.parametrize("front", [HANN0, ("rectangular", True, (0, 1))], ids=fr.front_id)
@pytest.mark.parametrize("shape", ["asr32", "htk40_logmel", "cep170", "g200"])
def test_without_preemphasis_the_history_sample_changes_no_bit(mfcc_amd, wav_pcm, shape, front):
    kw, _ = SHAPES[shape]
    nfft, hop, L, _ = _geom(kw)
    x = sr.input_list(nfft, hop, L, wav_pcm)
    y = x.copy()
    y[:, 0] = np.where(x[:, 0] > 0, -32768, 32767)                       # another history sample in every channel
    assert (x[:, 0] != y[:, 0]).all()
    with _open(mfcc_amd, kw, front, kernel_for(front, shape)) as m:
        m.set_filterbank(fb.htk_weights(80, nfft), "ln", 1e-10)
        for call in (m.process, m.power_spectrum, m.filterbank):
            assert same(as_np(call(_dev(x), halo=1)), as_np(call(_dev(y), halo=1))), (shape, call.__name__)
            # ... and equals the call without a history sample on the samples behind it
            assert same(as_np(call(_dev(x), halo=1)), as_np(call(_dev(x[:, 1:])))), (shape, call.__name__)
    # with pre-emphasis it does: the comparison above is not vacuous
    with _open(mfcc_amd, kw, ("rectangular", True, (32, 33))) as m:
        assert not same(as_np(m.power_spectrum(_dev(x), halo=1)), as_np(m.power_spectrum(_dev(y), halo=1)))


def _chunks(x, sizes):
    pos, out, i = 0, [], 0
    while pos < len(x):
        c = sizes[i % len(sizes)]
        out.append(x[pos:pos + c])
        pos += c
        i += 1
    return out


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("shape", ["asr32", "htk40_logmel", "cep170", "g1024"])
def test_sessions_and_banks_return_the_one_shot_rows(mfcc_amd, wav_pcm, shape, pad):
    kw, _ = SHAPES[shape]
    nfft, hop, L, _ = _geom(kw)
    n = 36 * hop + L + 7
    pcm = kf.channels(n, 11, wav_pcm, kinds=("speech", "noise", "silences", "uniform"))
    with _open(mfcc_amd, kw, HANN0, kernel_for(HANN0, shape), pad_mode=pad) as m:
        R = as_np(m.process(_dev(pcm)))
        assert R.shape[:2] == (4, m.num_frames(n))
        # the ragged route (utterances of different lengths: packed, one launch, gathered) and the host route
        cut = L + 20 * hop + 3
        for u, rows in zip((0, 1), m.process_batch([_dev(pcm[0]), _dev(pcm[1][:cut])])):
            assert same(as_np(rows), as_np(m.process(_dev(pcm[u][:len(pcm[u]) if u == 0 else cut]))[None][0])), (shape, pad, u)
        assert same(m.process(pcm[:2]), R[:2]), (shape, pad, "host")
        with m.stream() as s:
            rows = [s.push(c) for c in _chunks(pcm[0], (1, 159, 160, 161, 1000))]
            rows.append(s.flush())
            assert same(np.concatenate(rows), R[0]), (shape, pad, "session")
        sizes = [(1, 159, 160, 161, 1000), (0, 700, 0, 33), (2048,), (399, 0, 1, 160)]
        with m.stream_bank(4) as b:
            parts = [_chunks(pcm[u], sizes[u]) for u in range(4)]
            rows = [[] for _ in parts]
            while any(parts):
                for u, r in enumerate(b.push([p.pop(0) if p else np.zeros(0, np.int16) for p in parts])):
                    rows[u].append(r)
            for u, r in enumerate(b.flush()):
                rows[u].append(r)
            for u in range(4):
                assert same(np.concatenate(rows[u]), R[u]), (shape, pad, "bank", u)


@pytest.mark.parametrize("shape", ["asr32", "htk40_logmel"])
def test_post_passes_and_input_stages_see_the_fronted_rows(mfcc_amd, wav_pcm, shape):
    import torch
    kw, _ = SHAPES[shape]
    kernel = kernel_for(HANN0, shape)
    x = kf.channels(36 * 160 + 400, 5, wav_pcm, kinds=("speech", "noise", "uniform"))
    with _open(mfcc_amd, kw, HANN0, kernel) as raw:
        rows = raw.process(_dev(x))
        want = as_np(raw.deltas_rows(raw.normalize_rows(rows.clone(), mode="meanvar"), order=2, window=2))
        with _open(mfcc_amd, kw, HANN0, kernel, normalize="meanvar", deltas=2) as m:
            assert same(as_np(m.process(_dev(x))), want)
            assert same(m.process(x), want)
        ulaw = np.random.default_rng(5).integers(0, 256, 6000).astype(np.uint8)
        pcm16 = mfcc_amd.resample(mfcc_amd.decode(ulaw, "ulaw"), 8000, 16000)
        with _open(mfcc_amd, kw, HANN0, kernel, sample_format="ulaw", input_rate=8000) as m:
            assert same(as_np(m.process(torch.from_numpy(ulaw).cuda())), as_np(raw.process(_dev(pcm16))))
            assert same(m.process(ulaw), as_np(raw.process(_dev(pcm16))))
            assert same(as_np(m.power_spectrum(torch.from_numpy(ulaw).cuda())), as_np(raw.power_spectrum(_dev(pcm16))))


# ---------------------------------------------------------------------------------------------------- 4. fixed path
@pytest.mark.parametrize("front", [HANN0, ("hamming", False, (97, 100)), ("hamming", False, (31, 32)),
                                   ("hamming", True, (15, 16))], ids=fr.front_id)
def test_the_fixed_path_refuses_a_non_default_front(mfcc_amd, wav_pcm, golden_dir, tmp_path, front):
    import torch
    U = mfcc_amd._lib.ERROR_UNSUPPORTED
    x = kf.signal("speech", 4000, 1, wav_pcm)
    offs = np.array([0, 2000, 4000], np.uint64)
    wav = os.path.join(golden_dir, "f2bjrop1.0.wav")
    kw = dict(nfft=512, hop=170, nfilters=32, nceptrums=13)              # the fixed path's own shape
    with _open(mfcc_amd, kw, front) as m:
        out = torch.empty((1, 64, 13), device="cuda", dtype=torch.int16)
        calls = [lambda: m.process_fixed(x), lambda: m.process_fixed(_dev(x)), lambda: m.process_fixed(_dev(x), halo=1),
                 lambda: m.process_batch([x, x], fixed=True), lambda: m.process_batch([_dev(x), _dev(x[:3000])], fixed=True),
                 lambda: m.process_packed(_dev(x), offs, fixed=True),
                 lambda: m.time_launches(_dev(x), out, fixed=True), lambda: m.stream(fixed=True),
                 lambda: m.stream_bank(3, fixed=True),
                 lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=True),
                 lambda: m.convert_many([wav], [str(tmp_path / "b.mfcc")], fixed=True)]
        for i, call in enumerate(calls):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == U, (front, i)
        assert len(m.process(x)) == m.num_frames(len(x))                 # the float path of the same handle works
        assert m.convert(wav, str(tmp_path / "c.mfcc"), fixed=False) > 0


def test_the_fixed_path_keeps_the_default_front(mfcc_amd, wav_pcm):
    x = kf.signal("speech", 4000, 1, wav_pcm)
    kw = dict(nfft=512, hop=170, nfilters=32, nceptrums=13, pad_mode="stream")
    with mfcc_amd.MFCC(**kw) as plain, _open(mfcc_amd, kw, ("hamming", True, (62, 64))) as m:
        assert m.kernel_name(fixed=True) == plain.kernel_name(fixed=True)
        assert same(m.process_fixed(x), plain.process_fixed(x))
        assert same(as_np(m.process_fixed(_dev(x))), as_np(plain.process_fixed(_dev(x))))
