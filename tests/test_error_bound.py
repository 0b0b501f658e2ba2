"""The per-coefficient error bound (oracle/error_bound.py) tested as an instrument, on the CPU.

Each declared kernel model is emulated in NumPy with the kernels' arithmetic: exact integer pre-emphasis, fp32
window and FFT, fp32 |X|^2, the mel contraction and the DCT either in fp32 or on bf16 x 2-split operands
(round to nearest even, products Wh Ph + Wh Pl + Wl Ph accumulated in fp32; frames with a silent band take the
fp32 DCT), fp32 log2.  The bound must be SOUND -- every emulation within half of it on speech, noise at three
levels, full-scale noise, clipped square, sine, DC with dither and noise with silent stretches, at 512/32 at
16 / 44.1 / 48 kHz and at 1024/40 -- and SHARP: the mutants a kernel can plausibly turn into (one coefficient
off in one tile column, a bf16 split term dropped in column 15, the wrong pre-emphasis history at a tile's
first frame) are flagged, although some of them pass the old global measure."""
import numpy as np
import pytest
import scipy.fft

from oracle import error_bound as eb
from oracle import mfcc_float as mf


def bf16(a):
    """float32 -> bf16 (round to nearest even, like v_cvt_pk_bf16_f32), returned as float32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def split(a):
    a = np.asarray(a, dtype=np.float32)
    hi = bf16(a)
    with np.errstate(invalid="ignore"):
        return hi, bf16(a - hi)


def emulate(pcm, model, n_cep=13, nfft=512, hop=170, n_mel=32, sample_rate=16000, power_scale=512.0, lifter=0.0,
            mutant=None, output="cepstra"):
    """fp32 / bf16 x 2 emulation of a kernel of ``model`` (notebook framing), optionally with a ``mutant``:
    ("coef", frame % 16, coef, delta), ("mel", term), ("dct", term) -- split term 0: Wh Ph, 1: Wh Pl (Dh Ll),
    2: Wl Ph (Dl Lh) dropped in tile column 15 -- or ("emphasis",): history 0 at the first frame of every tile.
    ``output="logmel"``: the fp32 log-mel rows (``n_cep`` is ignored; a "coef" mutant names a band)."""
    mel_kind, dct_kind = eb.MODELS[model]
    x = np.asarray(pcm, dtype=np.float64)
    emph = mf.pre_emphasis(x)                                   # exact in fp32: (32 x - 31 x') / 32
    framed = mf.frame_audio(emph, nfft, hop)
    nf = len(framed)
    tile0 = np.arange(nf) % 16 == 0
    col15 = np.arange(nf) % 16 == 15
    if mutant and mutant[0] == "emphasis":
        rows = np.flatnonzero(tile0)[1:]
        framed[rows, 0] = x[rows * hop]
    win = (mf.hamming_window(nfft) / power_scale).astype(np.float32)
    y = framed.astype(np.float32) * win[None, :]
    X = scipy.fft.rfft(y, axis=1)
    assert X.dtype == np.complex64
    P = (X.real * X.real + X.imag * X.imag).astype(np.float32)
    W = mf.mel_filterbank(nfft, n_mel, sample_rate).astype(np.float32)
    if mel_kind == "fp32":
        E = P @ W.T
    else:
        Wh, Wl = split(W)
        Ph, Pl = split(P)
        terms = [Ph @ Wh.T, Pl @ Wh.T, Ph @ Wl.T]
        if mutant and mutant[0] == "mel":
            terms[mutant[1]] = np.where(col15[:, None], np.float32(0), terms[mutant[1]])
        E = (terms[0] + terms[1]) + terms[2]
    with np.errstate(divide="ignore"):
        Lm = np.log2(E.astype(np.float32))
    if output == "logmel":
        n_cep, dct_kind, D = n_mel, "identity", None
    else:
        D = mf.dct_basis(n_mel, n_mel)[:n_cep].astype(np.float32)
    with np.errstate(invalid="ignore"):
        c = Lm.copy() if D is None else Lm @ D.T
        if dct_kind == "bf16x2":
            Dh, Dl = split(D)
            Lh, Ll = split(Lm)
            terms = [Lh @ Dh.T, Ll @ Dh.T, Lh @ Dl.T]
            if mutant and mutant[0] == "dct":
                terms[mutant[1]] = np.where(col15[:, None], np.float32(0), terms[mutant[1]])
            cb = (terms[0] + terms[1]) + terms[2]
            c = np.where(np.isfinite(Lm).all(axis=1)[:, None], cb, c)     # -inf frames: the fp32 chain
    if lifter:
        c = c * (1 + (lifter / 2.0) * np.sin(np.pi * np.arange(n_cep) / lifter)).astype(np.float32)
    c = c.astype(np.float32)
    if mutant and mutant[0] == "coef":
        _, col, k, delta = mutant
        c[np.arange(nf) % 16 == col, k] += np.float32(delta)
    return c


# ----------------------------------------------------------------------------- inputs

def signal(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise3000":
        x = rng.standard_normal(n) * 3000
    elif kind == "noise30":
        x = rng.standard_normal(n) * 30
    elif kind == "uniform":
        x = rng.integers(-32768, 32768, n).astype(np.float64)
    elif kind == "square":
        x = 40000 * np.sign(np.sin(t * 0.0731))                  # clipped
    elif kind == "sine":
        x = 20000 * np.sin(t * 0.2113)
    elif kind == "dc_dither":
        x = 1234 + rng.integers(-1, 2, n).astype(np.float64)
    elif kind == "silences":
        x = rng.standard_normal(n) * 3000
        x[n // 5:n // 5 + 3000] = 0
        x[n // 2:n // 2 + 700] = 0
    else:
        raise ValueError(kind)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


KINDS = ["wav", "noise3000", "noise30", "uniform", "square", "sine", "dc_dither", "silences"]
SHAPES = {"512/16k": dict(nfft=512, hop=170, n_mel=32, sample_rate=16000, power_scale=512.0),
          "512/44.1k": dict(nfft=512, hop=170, n_mel=32, sample_rate=44100, power_scale=512.0),
          "512/48k": dict(nfft=512, hop=170, n_mel=32, sample_rate=48000, power_scale=512.0),
          "1024/40": dict(nfft=1024, hop=341, n_mel=40, sample_rate=16000, power_scale=1024.0),
          # other hops: the generic kernel's (fp32 / fp32) shapes
          "256/20 hop 1": dict(nfft=256, hop=1, n_mel=20, sample_rate=16000, power_scale=256.0),
          "512/32 hop 160": dict(nfft=512, hop=160, n_mel=32, sample_rate=16000, power_scale=512.0)}


def _pcm(kind, kw, wav_pcm):
    n = 16 * 25 * kw["hop"] + kw["nfft"]                        # 401 frames: 25 tiles and one ragged frame
    if kind == "wav":
        return wav_pcm[:n]
    return signal(kind, n, seed=len(kind))


# ----------------------------------------------------------------------------- soundness

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("model", list(eb.MODELS))
def test_bound_is_sound_on_every_input_kind(wav_pcm, shape, model):
    kw = SHAPES[shape]
    n_cep = kw["n_mel"]
    worst = {}
    for kind in KINDS:
        pcm = _pcm(kind, kw, wav_pcm)
        ref, bound = eb.reference_and_bound(pcm, model, n_cep=n_cep, **kw)
        got = emulate(pcm, model, n_cep=n_cep, **kw)
        worst[kind] = eb.check(got, ref, bound, "%s %s %s" % (model, shape, kind))
    assert max(worst.values()) <= 0.5, worst


def test_silent_frames_are_held_to_the_oracle_pattern(wav_pcm):
    pcm = signal("silences", 170 * 200 + 512, seed=3)
    ref, bound = eb.reference_and_bound(pcm, "bf16x2/bf16x2", n_cep=32)
    silent = np.isnan(bound).all(axis=1)
    assert silent.sum() >= 10 and np.isneginf(ref[silent, 0]).all()
    got = emulate(pcm, "bf16x2/bf16x2", n_cep=32)
    eb.check(got, ref, bound)
    bad = got.copy()
    bad[np.flatnonzero(silent)[3], 0] = -1e30                   # a finite value where the oracle has -inf
    with pytest.raises(AssertionError, match="pattern"):
        eb.check(bad, ref, bound)
    bad = got.copy()
    bad[np.flatnonzero(silent)[3], 1] = np.nan if np.isinf(ref[np.flatnonzero(silent)[3], 1]) else -np.inf
    with pytest.raises(AssertionError, match="pattern"):
        eb.check(bad, ref, bound)


def test_bands_that_are_roundoff_of_an_exact_zero_are_left_free():
    """A constant input: after the first frame every band away from DC is float64 roundoff of an exact zero (and
    exactly 0 in some frames), so neither arithmetic determines its log: those frames are unconstrained, -inf or not.
    Noise at normal levels has no such frame, and neither do the frames of a silent stretch (held to the pattern)."""
    pcm = np.full(170 * 60 + 512, -1234, np.int16)
    ref, bound = eb.reference_and_bound(pcm, "bf16x2/bf16x2", n_cep=32)
    free = eb.unbounded_frames(bound)
    assert free[1:].all()
    eb.check(emulate(pcm, "bf16x2/bf16x2", n_cep=32), ref, bound)
    for kind in ("noise3000", "noise30", "silences"):
        _, b = eb.reference_and_bound(signal(kind, 170 * 200 + 512, seed=9), "bf16x2/bf16x2", n_cep=32)
        assert not eb.unbounded_frames(b).any(), kind


def test_lifter_and_halo_and_stream_framing(wav_pcm):
    """The bound's other arguments: lifter weights, a history halo, stream padding -- shapes and soundness."""
    pcm = wav_pcm[:170 * 100 + 512 + 55]
    ref, bound = eb.reference_and_bound(pcm, "fp32/fp32", n_cep=32, lifter=22.0)
    eb.check(emulate(pcm, "fp32/fp32", n_cep=32, lifter=22.0), ref, bound)
    assert np.allclose(ref, mf.lifter(mf.mfcc_float_ref(pcm, n_cep=32), 22))
    r1, b1 = eb.reference_and_bound(pcm, "fp32/fp32", n_cep=13, halo=1)
    assert r1.shape == b1.shape == (mf.num_frames_notebook(len(pcm) - 1), 13)
    np.testing.assert_array_equal(r1, mf.mfcc_float_ref(np.concatenate([np.zeros(169, np.int16), pcm]))[1:])
    rs, bs = eb.reference_and_bound(np.stack([pcm, pcm[::-1].copy()]), "fp32/fp32", n_cep=13, pad_mode="stream")
    assert rs.shape == bs.shape == (2, mf.num_frames_stream(len(pcm)), 13)
    np.testing.assert_array_equal(rs[1], mf.mfcc_float_ref(pcm[::-1].copy(), pad_mode="stream"))


@pytest.mark.parametrize("hop", [1, 2, 160, 511, 512])
def test_halo_and_stream_framing_at_other_hops(wav_pcm, hop):
    """halo=1 puts sample 0 hop - 1 zeros into a longer stream (none at hop 1) and drops that stream's frame 0; STREAM
    framing zero-pads to the end of its last frame: both against the oracle run directly on that stream."""
    kw = dict(nfft=512, hop=hop, n_mel=32, sample_rate=16000, power_scale=512.0)
    pcm = wav_pcm[5000:5000 + 512 + hop * (1500 // hop + 3) + hop // 2 + 1]
    n = len(pcm)
    r1, b1 = eb.reference_and_bound(pcm, "fp32/fp32", n_cep=13, halo=1, **kw)
    assert r1.shape == b1.shape == (mf.num_frames_notebook(n - 1, 512, hop), 13)
    longer = np.concatenate([np.zeros(hop - 1, np.int16), pcm])
    np.testing.assert_array_equal(r1, mf.mfcc_notebook(longer, **kw)[1:, :13])
    rs, bs = eb.reference_and_bound(pcm, "fp32/fp32", n_cep=13, pad_mode="stream", **kw)
    nf = mf.num_frames_stream(n, 512, hop)
    assert rs.shape == bs.shape == (nf, 13) and (nf - 1) * hop + 512 >= n
    padded = np.concatenate([pcm, np.zeros((nf - 1) * hop + 512 - n, np.int16)])
    np.testing.assert_array_equal(rs, mf.mfcc_notebook(padded, **kw)[:, :13])
    np.testing.assert_array_equal(rs, mf.mfcc_float_ref(pcm, pad_mode="stream", **kw))
    eb.check(emulate(padded, "fp32/fp32", n_cep=13, **kw), rs, bs)


# ----------------------------------------------------------------------------- sharpness

def _old_measure(got, ref):
    fin = np.isfinite(ref).all(axis=1)
    d = got[fin].astype(np.float64) - ref[fin]
    return np.abs(d).max() / np.abs(ref[fin]).max(), np.linalg.norm(d) / np.linalg.norm(ref[fin])


@pytest.mark.parametrize("kind", ["wav", "noise3000"])
def test_one_coefficient_off_in_one_tile_column_is_flagged(wav_pcm, kind):
    kw = SHAPES["512/16k"]
    pcm = _pcm(kind, kw, wav_pcm)
    model = "bf16x2/bf16x2"
    ref, bound = eb.reference_and_bound(pcm, model, n_cep=13)
    got = emulate(pcm, model, n_cep=13, mutant=("coef", 15, 5, 1e-3))
    e_max, e_l2 = _old_measure(got, ref)
    assert e_max <= 1e-4 and e_l2 <= 1e-4                       # the gap: the global contract does not see it
    with pytest.raises(AssertionError, match=r"frame % 16: \[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 25\]"):
        eb.check(got, ref, bound)


@pytest.mark.parametrize("shape", ["512/16k", "1024/40"])
@pytest.mark.parametrize("term", [1, 2])
def test_dropped_mel_split_term_in_column_15_is_flagged(wav_pcm, shape, term):
    kw = SHAPES[shape]
    pcm = _pcm("wav", kw, wav_pcm)
    ref, bound = eb.reference_and_bound(pcm, "bf16x2/fp32", n_cep=13, **kw)
    got = emulate(pcm, "bf16x2/fp32", n_cep=13, mutant=("mel", term), **kw)
    with pytest.raises(AssertionError, match=r"frame % 16: \[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, [1-9]"):
        eb.check(got, ref, bound)


@pytest.mark.parametrize("term", [0, 1, 2])
@pytest.mark.parametrize("kind", ["wav", "noise3000"])
def test_dropped_dct_split_term_in_column_15_is_flagged(wav_pcm, term, kind):
    pcm = _pcm(kind, SHAPES["512/16k"], wav_pcm)
    ref, bound = eb.reference_and_bound(pcm, "bf16x2/bf16x2", n_cep=32)
    got = emulate(pcm, "bf16x2/bf16x2", n_cep=32, mutant=("dct", term))
    with pytest.raises(AssertionError, match=r"frame % 16: \[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, [1-9]"):
        eb.check(got, ref, bound)


@pytest.mark.parametrize("model", list(eb.MODELS))
def test_wrong_emphasis_history_at_a_tile_start_is_flagged(wav_pcm, model):
    pcm = _pcm("wav", SHAPES["512/16k"], wav_pcm)
    ref, bound = eb.reference_and_bound(pcm, model, n_cep=13)
    got = emulate(pcm, model, n_cep=13, mutant=("emphasis",))
    with pytest.raises(AssertionError, match=r"frame % 16: \[[1-9][0-9]*, 0, 0,"):
        eb.check(got, ref, bound)


def test_models_of_the_kernels():
    assert eb.model_of("mfcc_fused512_w12_kernel") == "bf16x2/bf16x2"
    assert eb.model_of("mfcc_fused512_kernel") == "bf16x2/fp32"
    assert eb.model_of("mfcc_fused1024_w12bf_kernel") == "bf16x2/fp32"
    assert eb.model_of("mfcc_fused1024_kernel", "bf16") == "bf16x2/fp32"
    assert eb.model_of("mfcc_fused1024_w12_kernel") == eb.model_of("mfcc_fused1024_kernel", "f32") == "fp32/fp32"
    assert eb.model_of("mfcc_float_generic_kernel") == "fp32/fp32"
    with pytest.raises(ValueError):
        eb.model_of("mfcc_fused1024_kernel")
    with pytest.raises(KeyError):
        eb.model_of("mfcc_fixed512_kernel")
