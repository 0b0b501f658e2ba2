"""Fronted handles -- a window function and a pre-emphasis pair other than (periodic Hamming, 31/32) -- where the
existing GPU tests never took them: the exact-DC paths, the routes that carry a history sample or an utterance boundary,
and the loud end of the pre-emphasis.

1. Every form the sample rate gives a kernel (tests/front_rate_cases.py: ``cases()``) under the five non-default fronts,
   against the float64 reference of tests/front_ref.py at that rate, 1.0 x the project's bounds; the not-blind condition
   (proven on the CPU by tests/test_front_rates_host.py) is asserted again before a kernel's output is looked at.
2. The bands with weight on bin 0 under the bound of the exact-DC arithmetic (``fc.dc_reference_and_bound``).
3. Sessions, banks, online banks, the ragged and packed routes, the host pipeline's frame-range chunks and the input
   stages, at fronts whose window is not 0 at sample 0 and whose pair is neither 0 nor 31/32: bit for bit the one-shot
   call of each utterance on its own.
4. Full-scale inputs that alternate sign every sample, at the pairs where ``|e|`` comes closest to the limit of the biased
   dot product (fused kernels) and of the fp32 fma (generic kernels).

Every test asserts the kernel's name before it compares anything and prints it with the worst error / bound."""
import numpy as np
import pytest

import fbank_ref as fb
import front_rate_cases as fc
import front_ref as fr
import kernel_families as kf
import spectrum_ref as sr
import test_gpu_front as tgf
from kernel_families import as_np, same
from oracle import error_bound as eb
from test_gpu_sample_rates import _strided

pytestmark = pytest.mark.gpu

GENERIC, W4, H160, MB = fc.GENERIC, fc.W4, fc.H160, fc.H160MB
SPEC_FUSED, SPEC_GENERIC, FB_FUSED, FB_GENERIC = tgf.SPEC_FUSED, tgf.SPEC_GENERIC, tgf.FB_FUSED, tgf.FB_GENERIC
CASES = fc.cases()


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()                          # a copy: some inputs are kept read-only


def _open(mfcc_amd, kw, front, kernel, **over):
    """A handle of ``kw`` under ``front``; fails unless the library reports ``kernel``."""
    m = mfcc_amd.MFCC(**dict(kw, **fr.front_kw(front)), **over)
    if m.kernel_name() != kernel:
        name = m.kernel_name()
        m.close()
        raise AssertionError("%s %s: the handle runs %s, not %s" % (fr.front_id(front), kw, name, kernel))
    return m


# ---------------------------------------------------------------------------------------------------- 1. parity
def _check(case, front, got, wav_pcm, pad="notebook", halo=0):
    fc.assert_not_blind(case, front, wav_pcm, pad, halo)               # before the kernel's output is looked at
    got = as_np(got)
    assert got.dtype == np.float32 and got.shape[0] == len(fc.KINDS) and got.shape[2] == case.width, (case.id, got.shape)
    worst = 0.0
    for c, kind in enumerate(fc.KINDS):
        ref, bound = fc.reference(case, front, wav_pcm, c, pad, halo)
        worst = max(worst, eb.check(got[c], ref, bound, "%s %s channel %s" % (case.id, fr.front_id(front), kind)))
    print("%s %s %s halo %d (%s): worst error / bound %.3f" % (case.id, fr.front_id(front), pad, halo, case.kernel(front), worst))
    return worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_fronted_rows_at_every_form_of_the_rate_map(mfcc_amd, wav_pcm, case):
    """37 frames x the five channels of tests/sample_rate_cases.py, notebook framing, channels on an odd stride."""
    dev = _strided(fc.pcm_of(case, wav_pcm))
    for front in fc.FRONTS:
        with _open(mfcc_amd, case.kw, front, case.kernel(front)) as m:
            assert m.num_frames(case.n_samples) == fc.NFR
            got = m.process(dev)
        assert as_np(got).shape == (len(fc.KINDS), fc.NFR, case.width)
        _check(case, front, got, wav_pcm)


@pytest.mark.parametrize("case", fc.stream_cases(), ids=lambda c: c.id)
def test_fronted_rows_in_stream_framing_behind_a_history_sample(mfcc_amd, wav_pcm, case):
    dev = _strided(fc.pcm_of(case, wav_pcm))
    for front in fc.FRONTS:
        with _open(mfcc_amd, case.kw, front, case.kernel(front), pad_mode="stream") as m:
            got = m.process(dev, halo=1)
        _check(case, front, got, wav_pcm, "stream", 1)


# ---------------------------------------------------------------------------------------------------- 2. the DC bin
@pytest.mark.parametrize("case", fc.dc_cases(), ids=lambda c: c.id)
def test_the_dc_bands_meet_the_bound_of_the_exact_sum(mfcc_amd, case):
    """``const_min`` under (povey, 32/33) and (rectangular, 63/64), ``dc_dither`` and ``dc_under_tone`` under every
    front: the log-mel value of every band with weight on bin 0 (cepstra of full width through the inverse DCT)."""
    x = fc.dc_channels(case.n_samples)
    bands = case.dc_bands()
    assert len(bands)
    for front in fc.FRONTS:
        with _open(mfcc_amd, case.kw, front, case.kernel(front)) as m:
            got = as_np(m.process(_dev(x)))
        assert got.shape == (len(fc.DC_KINDS), fc.NFR, case.width)
        for k, kind in enumerate(fc.DC_KINDS):
            if kind == "const_min" and front not in fc.DC_FRONTS:
                continue
            ref, bound, first = fc.dc_reference_and_bound(case, front, x[k])
            if case.logmel:
                assert np.isfinite(bound).all()
                rows = got[k][:, bands].astype(np.float64)
            else:
                with np.errstate(invalid="ignore"):
                    rows = fc.cepstra_to_logmel(got[k], case.kw["nfilters"])[:, bands]
            what = "%s %s %s" % (case.id, fr.front_id(front), kind)
            worst = eb.check(rows, ref, bound, what)
            fin = np.isfinite(bound)
            print("%s (%s): DC bands %s, worst error / section-2 bound %.3f (bound <= %.3g, %d of %d elements; section 1 <= %.3g where finite)"
                  % (what, case.kernel(front), bands.tolist(), worst, bound[fin].max(initial=0.0), int(fin.sum()), fin.size,
                     first[np.isfinite(first)].max(initial=0.0)))


# ---------------------------------------------------------------------------------------------------- 3. routes
ROUTE_SHAPES = {s: tgf.SHAPES[s][0] for s in ("asr32", "htk40_logmel", "cep170", "g200", "g1024")}
ROUTE_SHAPES["asr32_64k"] = dict(tgf.SHAPES["asr32"][0], samplerate=64000)        # a DCX form through the routes
FUSED_OF = {"asr32": H160, "htk40_logmel": MB, "cep170": W4, "g200": GENERIC, "g1024": GENERIC, "asr32_64k": H160}
ROUTES = [(s, f) for s in ROUTE_SHAPES for f in (fc.R, fc.G)] + [(s, fc.POVEY) for s in ("asr32", "htk40_logmel")]
ROUTE_IDS = ["%s-%s" % (s, fr.front_id(f)) for s, f in ROUTES]


def _route_handle(mfcc_amd, shape, front, **over):
    kernel = FUSED_OF[shape] if fr.fused_pair(front) else GENERIC
    return _open(mfcc_amd, ROUTE_SHAPES[shape], front, kernel, **over), kernel


def _cat(rows, width):
    rows = [as_np(r) for r in rows if len(r)]
    return np.concatenate(rows) if rows else np.zeros((0, width), np.float32)


@pytest.mark.parametrize("shape,front", ROUTES, ids=ROUTE_IDS)
def test_sessions_and_banks_return_the_one_shot_rows(mfcc_amd, wav_pcm, shape, front):
    nfft, hop, L, _ = tgf._geom(ROUTE_SHAPES[shape])
    n = 36 * hop + L + 7
    pcm = kf.channels(n, 11, wav_pcm, kinds=("speech", "noise", "silences", "uniform"))
    sizes = [(1, 159, 160, 161, 1000), (0, 700, 0, 33), (2048,), (399, 0, 1, 160)]
    for pad in ("notebook", "stream"):
        m, kernel = _route_handle(mfcc_amd, shape, front, pad_mode=pad)
        with m:
            R = as_np(m.process(_dev(pcm)))
            assert R.shape[:2] == (4, m.num_frames(n))
            with m.stream() as s:
                rows = [s.push(c) for c in tgf._chunks(pcm[0], sizes[0])]
                rows.append(s.flush())
                assert same(np.concatenate(rows), R[0]), (shape, pad, "session")
            with m.stream_bank(4) as b:
                parts = [tgf._chunks(pcm[u], sizes[u]) for u in range(4)]
                rows = [[] for _ in parts]
                while any(parts):
                    for u, r in enumerate(b.push([p.pop(0) if p else np.zeros(0, np.int16) for p in parts])):
                        rows[u].append(r)
                for u, r in enumerate(b.flush()):
                    rows[u].append(r)
                for u in range(4):
                    assert same(np.concatenate(rows[u]), R[u]), (shape, pad, "bank", u)
            # the online bank: causal CMVN over 40 rows and two orders of deltas of each stream's own rows
            raw = m.process(_dev(pcm))
            want = as_np(m.deltas_rows(m.normalize_rows(raw.clone(), mode="meanvar", window=40, min_window=1, center=False),
                                       order=2, window=2))
            with m.stream_bank(4, normalize="meanvar", normalize_window=40, deltas=2) as b:
                parts = [tgf._chunks(pcm[u], sizes[u]) for u in range(4)]
                rows = [[] for _ in parts]
                while any(parts):
                    for u, r in enumerate(b.push([p.pop(0) if p else np.zeros(0, np.int16) for p in parts])):
                        rows[u].append(r)
                for u, r in enumerate(b.flush()):
                    rows[u].append(r)
                for u in range(4):
                    assert same(_cat(rows[u], want.shape[-1]), want[u]), (shape, pad, "online bank", u)
    print("%s %s (%s): session, bank and online bank equal the one-shot rows" % (shape, fr.front_id(front), kernel))


@pytest.mark.parametrize("shape,front", ROUTES, ids=ROUTE_IDS)
def test_an_utterance_starts_on_history_zero_in_every_ragged_route(mfcc_amd, wav_pcm, shape, front):
    """Six utterances back to back, each ending on +32767 and starting on -32768: a predecessor read across a boundary
    moves ``e[0]`` by ``num 32767`` under a window whose first value is not 0."""
    kw = ROUTE_SHAPES[shape]
    nfft, hop, L, _ = tgf._geom(kw)
    utts = fc.boundary_utterances(L, hop, wav_pcm)
    assert len(utts) >= 5 and L in [len(u) for u in utts] and min(len(u) for u in utts) < L
    assert all(u[-1] == 32767 and v[0] == -32768 for u, v in zip(utts, utts[1:]))
    flat = np.concatenate(utts)
    offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint64)
    W = fb.htk_weights(80, nfft)
    m, kernel = _route_handle(mfcc_amd, shape, front)
    fused = kernel != GENERIC and nfft == 512
    with m:
        assert m.spectrum_kernel_name() == (SPEC_FUSED if fused else SPEC_GENERIC)
        m.set_filterbank(W, "ln", 1e-10)
        assert m.filterbank_kernel_name() == (FB_FUSED if fused else FB_GENERIC)
        calls = {"rows": m.process, "power": m.power_spectrum, "bands": m.filterbank}
        alone = {k: [as_np(f(_dev(u))) if len(u) >= L else None for u in utts] for k, f in calls.items()}
        nf = [0 if a is None else len(a) for a in alone["rows"]]
        assert nf[1] == 1 and nf[3] == 0 and [m.num_frames(len(u)) for u in utts] == nf
        width = {k: [a for a in v if a is not None][0].shape[-1] for k, v in alone.items()}
        want = {k: [np.zeros((0, width[k]), np.float32) if a is None else a for a in v] for k, v in alone.items()}
        for name, got in (("device list", m.process_batch([_dev(u) for u in utts])), ("host list", m.process_batch(utts))):
            assert len(got) == len(utts)
            for u, g in enumerate(got):
                assert same(as_np(g), want["rows"][u]), (shape, name, u)
        for k, call in (("rows", m.process_packed), ("power", m.power_spectrum_packed), ("bands", m.filterbank_packed)):
            out, fo = call(_dev(flat), offs)
            out = as_np(out)
            assert np.diff(fo.astype(np.int64)).tolist() == nf
            for u in range(len(utts)):
                assert same(out[int(fo[u]):int(fo[u + 1])], want[k][u]), (shape, k + " packed", u)
        # non-vacuity: the boundary shows.  The flat buffer as ONE stream differs in the first frame of utterance 2 ...
        if fr.window(front[0], L, front[1])[0] != 0:               # (povey, symmetric) is 0 at sample 0
            whole = as_np(m.power_spectrum(_dev(flat[int(offs[1]) - 1:int(offs[2])]), halo=1))
            assert not same(whole[:1], want["power"][1][:1]), (shape, "a leaked predecessor would not show")
    print("%s %s (%s): batch, packed, packed power and packed bands equal each utterance on its own"
          % (shape, fr.front_id(front), kernel))


@pytest.mark.parametrize("shape", list(ROUTE_SHAPES))
def test_the_history_sample_shows_at_these_fronts(mfcc_amd, wav_pcm, shape):
    """Non-vacuity of the route tests: under ``halo=1`` another history sample changes the rows at R and at G, and the
    call equals the one-shot call of the stream it stands for."""
    kw = ROUTE_SHAPES[shape]
    nfft, hop, L, _ = tgf._geom(kw)
    x = sr.input_list(nfft, hop, L, wav_pcm, frames=5)[:3]
    y = x.copy()
    y[:, 0] = np.where(x[:, 0] > 0, -32768, 32767)
    for front in (fc.R, fc.G):
        m, kernel = _route_handle(mfcc_amd, shape, front)
        with m:
            m.set_filterbank(fb.htk_weights(80, nfft), "ln", 1e-10)
            for call in (m.process, m.power_spectrum, m.filterbank):
                a, b = as_np(call(_dev(x), halo=1)), as_np(call(_dev(y), halo=1))
                assert a.shape == b.shape and not same(a[:, 0], b[:, 0]), (shape, fr.front_id(front), call.__name__)
                assert same(a[:, 1:], b[:, 1:])                    # no frame behind the first reads that sample
                assert not same(a, as_np(call(_dev(x[:, 1:])))), (shape, fr.front_id(front), call.__name__)


@pytest.mark.parametrize("shape,front", [("asr32_64k", fc.R), ("cep170", fc.R), ("g1024", fc.G), ("htk40_logmel", fc.POVEY)],
                         ids=lambda v: v if isinstance(v, str) else fr.front_id(v))
def test_host_arrays_in_frame_range_chunks(mfcc_amd, shape, front, monkeypatch):
    """1 MB chunks (524 288 samples): one long channel goes in frame ranges, each behind its own history sample."""
    n = 524_288 + 90_001
    long = np.random.default_rng(31).integers(-32768, 32768, n).astype(np.int16)
    m, kernel = _route_handle(mfcc_amd, shape, front)
    with m:
        want = as_np(m.process(_dev(long)))
        want_p = as_np(m.power_spectrum(_dev(long)))
        monkeypatch.setenv("MFCC_HIP_HOST_CHUNK_MB", "1")
        got, got_p = m.process(long), m.power_spectrum(long)
        monkeypatch.delenv("MFCC_HIP_HOST_CHUNK_MB")
        assert same(got, want) and same(got_p, want_p), (shape, fr.front_id(front))
        assert same(m.process(long), want)
    print("%s %s (%s): %d frames in frame-range chunks equal the device call" % (shape, fr.front_id(front), kernel, len(want)))


@pytest.mark.parametrize("shape", ["asr32", "htk40_logmel"])
def test_post_passes_and_input_stages_see_the_fronted_rows(mfcc_amd, wav_pcm, shape):
    import torch
    kw = ROUTE_SHAPES[shape]
    kernel = FUSED_OF[shape]
    x = kf.channels(36 * 160 + 400, 5, wav_pcm, kinds=("speech", "noise", "uniform"))
    with _open(mfcc_amd, kw, fc.R, kernel) as raw:
        rows = raw.process(_dev(x))
        want = as_np(raw.deltas_rows(raw.normalize_rows(rows.clone(), mode="meanvar"), order=2, window=2))
        with _open(mfcc_amd, kw, fc.R, kernel, normalize="meanvar", deltas=2) as m:
            assert same(as_np(m.process(_dev(x))), want)
            assert same(m.process(x), want)
        ulaw = np.random.default_rng(5).integers(0, 256, 6000).astype(np.uint8)
        pcm16 = mfcc_amd.resample(mfcc_amd.decode(ulaw, "ulaw"), 8000, 16000)
        with _open(mfcc_amd, kw, fc.R, kernel, sample_format="ulaw", input_rate=8000) as m:
            assert same(as_np(m.process(torch.from_numpy(ulaw).cuda())), as_np(raw.process(_dev(pcm16))))
            assert same(m.process(ulaw), as_np(raw.process(_dev(pcm16))))
            assert same(as_np(m.power_spectrum(torch.from_numpy(ulaw).cuda())), as_np(raw.power_spectrum(_dev(pcm16))))
    print("%s %s (%s): post passes and input stages" % (shape, fr.front_id(fc.R), kernel))


# ---------------------------------------------------------------------------------------------------- 4. loud inputs
LOUD = [("cep170", W4), ("asr32", H160), ("htk40_logmel", MB)]


def _loud_rows(mfcc_amd, wav_pcm, shape, kernel, front, what):
    kw = tgf.SHAPES[shape][0]
    nfft, hop, L, ps = tgf._geom(kw)
    x = fc.loud_channels(sr.samples_for(fc.LOUD_FRAMES, L, hop), wav_pcm)
    num, den = front[2]
    assert [fc.max_abs_e(c, num, den) == den * 32768 + num * 32767 for c in x] == [False, True, True, True]
    with _open(mfcc_amd, kw, front, kernel) as m:
        got = as_np(m.process(_dev(x)))
        power = as_np(m.power_spectrum(_dev(x)))
        spec = m.spectrum_kernel_name()
    model = "fp32/fp32" if kernel == GENERIC else "bf16x2/fp32"
    ref, bound = tgf._reference(x, kw, front, model, "notebook", 0)
    assert np.isfinite(bound[0]).all()                                # speech, the quiet neighbour, is bounded everywhere
    worst = eb.check(got, ref, bound, "%s %s rows" % (what, fr.front_id(front)))
    p_ref = fr.power_reference(x, front, nfft, hop, L, power_scale=sr.power_scale_of(nfft))
    b = sr.bound(p_ref)
    sr.assert_not_blind(b, fr.zero_frames(x, front, nfft, hop, L, "notebook", 0), what)
    assert not fr.zero_frames(x, front, nfft, hop, L, "notebook", 0).any()
    worst_p = sr.check(power, p_ref, b, "%s %s power" % (what, fr.front_id(front)))
    print("%s %s (%s, %s): worst error / bound rows %.3f, power %.3f" % (what, fr.front_id(front), kernel, spec, worst, worst_p))
    return spec


@pytest.mark.parametrize("shape,kernel", LOUD, ids=[s for s, _ in LOUD])
def test_the_biased_dot_product_at_its_loud_end(mfcc_amd, wav_pcm, monkeypatch, shape, kernel):
    """Rows and power of the three four-wave kernels and of mfcc_spectrum512_kernel under (63, 64), (1, 126) and the
    default pair, on speech, both phases of the Nyquist square and random full-scale signs."""
    for front in (fc.R, fc.QUIET, fr.DEFAULT):
        if kernel == W4 and fr.is_default(front):
            monkeypatch.setenv("MFCC_HIP_FUSED512", "w4")             # read when a handle is made: the default front's
        assert _loud_rows(mfcc_amd, wav_pcm, shape, kernel, front, shape) == SPEC_FUSED      # twelve-wave kernel otherwise
        monkeypatch.delenv("MFCC_HIP_FUSED512", raising=False)


@pytest.mark.parametrize("cfg", tgf.POWER_CFGS[:2], ids=lambda c: "%d_%d_%d" % c)
def test_band_energies_at_the_loud_end(mfcc_amd, wav_pcm, cfg):
    """mfcc_fbank512_kernel with HTK 80 (its fp32 form) and a dense 128 x 257 matrix (its MFMA form) in ENERGY scale, so
    that no element is set aside; the generic filterbank kernel under (127, 128)."""
    nfft, hop, L = cfg
    x = fc.loud_channels(sr.samples_for(fc.LOUD_FRAMES, L, hop), wav_pcm)
    mats = {"htk80_energy": fb.htk_weights(80), "dense128": fb.dense_random(128)}
    for front in (fc.R, fc.QUIET, fr.DEFAULT, fc.LOUD_GENERIC):
        kernel = FB_FUSED if fr.fused_pair(front) else FB_GENERIC
        p_ref = fr.power_reference(x, front, nfft, hop, L)
        zero = fr.zero_frames(x, front, nfft, hop, L, "notebook", 0)
        with tgf._open(mfcc_amd, tgf._power_kw(cfg), front) as m:
            for name, W in mats.items():
                m.set_filterbank(W, "energy", 0.0)
                assert m.filterbank_kernel_name() == kernel, (fr.front_id(front), cfg)
                got = as_np(m.filterbank(_dev(x)))
                e_ref, b_e = fb.energy_ref_and_bound(p_ref, W, fb.form_of(W, kernel))
                fb.assert_not_blind(b_e, fb.pinned_mask(zero, W), name)
                worst, aside = fb.check(got, e_ref, b_e, "energy", 0.0, "%s %s %s" % (fr.front_id(front), cfg, name))
                assert aside == 0
                print("%s %s %s (%s): worst error / bound %.3f" % (fr.front_id(front), cfg, name, kernel, worst))


@pytest.mark.parametrize("shape", ["cep170", "asr32", "g1024"])
def test_the_generic_fma_at_its_loud_end(mfcc_amd, wav_pcm, shape):
    """mfcc_float_generic_kernel and mfcc_spectrum_generic_kernel under (127, 128): ``|e|`` up to 255 x 2^15 - 127."""
    assert _loud_rows(mfcc_amd, wav_pcm, shape, GENERIC, fc.LOUD_GENERIC, shape) == SPEC_GENERIC
