"""The error bounds as instruments where the sample rate degenerates the mel bank, on the CPU.

From 88.2 kHz up the notebook's 512 / 32 bank has structurally empty filters (all weights zero: two integer filter
points coincide).  Such a band is -inf in every frame, so ``eb.bound_from_stages`` read every frame as "silent" and
the whole log-mel bound came back NaN: only the finite / non-finite pattern was checked and the 31 finite bands could
hold anything.  tests/logmel_bound.py now bounds per band.  Proven here:

* unchanged: on banks without an empty band the bounds of logmel_bound, framed_ref and melbank_ref are what the plain
  ``eb.bound_from_stages`` call gave, ``array_equal``;
* sound: the fp32 / bf16 x 2 emulation of tests/test_error_bound.py stays inside the bound at 12, 64, 96 and 192 kHz,
  512 / 32 (cepstra and log-mel) and 512 / 16, and reproduces the oracle's -inf / +-inf / NaN pattern;
* sharp: at 96 kHz log-mel the mutants of that file (one value off in one tile column, a split term dropped in column
  15), applied to a finite band of frames that have an empty band, fail -- and passed the whole-row bound;
* not blind: on speech, noise and uniform noise every element of every non-empty band has a finite bound and the
  elements without one are exactly frames x empty bands;
* cepstra with an empty band: the sign of an infinity is -sign(D[k, b]); the only elements set aside are those whose
  weight on an empty band is float64 roundoff of an exact zero, listed from the basis."""
import numpy as np
import pytest

import framed_ref as fr
import kernel_families as kf
import logmel_bound as lb
import melbank_ref as mr
import test_error_bound as teb
from oracle import error_bound as eb
from oracle import mfcc_float as mf

RATES = [12000, 64000, 96000, 192000]
EMPTY_512_32 = {12000: [], 64000: [], 96000: [1], 192000: [0, 2, 4]}
NFR = 16 * 4 + 5


def _kw(rate, n_mel=32):
    return dict(nfft=512, hop=170, n_mel=n_mel, sample_rate=rate, power_scale=512.0)


def _pcm(kind, wav_pcm, seed=5):
    return kf.signal(kind, 170 * (NFR - 1) + 512, seed, wav_pcm)


def _plain_logmel_bound(st, model):
    """What the three modules computed before: the whole-row bound, the identity as the basis."""
    n_mel = len(st["filters"])
    extra = lb.BF16X2_MEL_EXTRA if eb.MODELS[model][0] == "bf16x2" else 0.0
    with np.errstate(invalid="ignore"):
        return eb.bound_from_stages(dict(st, dct_basis=np.eye(n_mel)), model, n_mel) + lb.LOG2_ABS + extra


# ----------------------------------------------------------------------------- unchanged without an empty band

@pytest.mark.parametrize("model", ["bf16x2/fp32", "fp32/fp32"])
@pytest.mark.parametrize("shape", ["512/16k", "512/48k", "1024/40", "256/20 hop 1"])
def test_bounds_without_an_empty_band_are_what_they_were(wav_pcm, shape, model):
    kw = teb.SHAPES[shape]
    assert not lb.empty_bands(mf.mel_filterbank(kw["nfft"], kw["n_mel"], kw["sample_rate"])).any()
    for kind in teb.KINDS:                      # silences (NaN rows) and dc_dither (+inf rows) among them
        pcm = teb._pcm(kind, kw, wav_pcm)[:kw["hop"] * 40 + kw["nfft"]]
        _, st = mf.mfcc_notebook(pcm, return_stages=True, **kw)
        ref, bound = lb.reference_and_bound(pcm, model, **kw)
        assert np.array_equal(ref, st["logmel"], equal_nan=True)
        assert np.array_equal(bound, _plain_logmel_bound(st, model), equal_nan=True), (shape, kind)


@pytest.mark.parametrize("model", ["bf16x2/fp32", "fp32/fp32"])
def test_framed_and_banked_bounds_without_an_empty_band_are_what_they_were(wav_pcm, model):
    for kind in ("speech", "silences", "const_min"):
        pcm = kf.signal(kind, 160 * 36 + 400, 3, wav_pcm)
        _, st = fr.framed_notebook(pcm, 400, 160, 512, 32, 48000, 512.0)
        _, bound = fr.reference_and_bound(pcm, model, 400, 160, sample_rate=48000, output="logmel")
        assert np.array_equal(bound, _plain_logmel_bound(st, model), equal_nan=True), kind
        W = mr.matrix(512, 40, 16000, 20.0, None)
        assert not lb.empty_bands(W).any()
        _, st = mr.banked_notebook(pcm, W, 400, 160)
        _, bound = mr.reference_and_bound(pcm, model, 400, 160, n_mel=40, low=20.0, output="logmel")
        assert np.array_equal(bound, _plain_logmel_bound(st, model), equal_nan=True), kind


def test_an_empty_band_used_to_blind_the_whole_bound(wav_pcm):
    pcm = _pcm("noise", wav_pcm)
    _, st = mf.mfcc_notebook(pcm, return_stages=True, **_kw(96000))
    assert np.isnan(_plain_logmel_bound(st, "bf16x2/fp32")).all()
    _, bound = lb.reference_and_bound(pcm, "bf16x2/fp32", **_kw(96000))
    assert np.isnan(bound[:, 1]).all() and np.isfinite(np.delete(bound, 1, axis=1)).all()
    # the other bands keep the bound they have without the empty band, value for value
    live = np.arange(32) != 1
    sub = dict(st, filters=st["filters"][live], mel=st["mel"][:, live], logmel=st["logmel"][:, live])
    assert np.array_equal(bound[:, live], _plain_logmel_bound(sub, "bf16x2/fp32"))


def test_all_zero_frames_still_pin_the_whole_row(wav_pcm):
    pcm = _pcm("silences", wav_pcm)
    ref, bound = lb.reference_and_bound(pcm, "bf16x2/fp32", **_kw(96000))
    zero = np.isneginf(ref).all(axis=1)
    assert zero.sum() >= 3 and np.isnan(bound[zero]).all()
    assert np.isfinite(np.delete(bound[~zero], 1, axis=1)).all() and np.isnan(bound[~zero, 1]).all()


# ----------------------------------------------------------------------------- soundness

@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("model", sorted(set(lb.MODEL.values())))      # a log-mel row has no DCT: two models
def test_logmel_bound_is_sound(wav_pcm, rate, model):
    worst = {}
    for n_mel in (32, 16):
        kw = _kw(rate, n_mel)
        empty = lb.empty_bands(mf.mel_filterbank(512, n_mel, rate))
        assert np.flatnonzero(empty).tolist() == (EMPTY_512_32[rate] if n_mel == 32 else [])
        for kind in kf.KINDS:
            pcm = _pcm(kind, wav_pcm)
            ref, bound = lb.reference_and_bound(pcm, model, **kw)
            assert np.isneginf(ref[:, empty]).all()
            if kind in ("speech", "noise", "uniform"):
                lb.assert_not_blind(bound, mf.mel_filterbank(512, n_mel, rate), "%d / %d %s" % (rate, n_mel, kind))
            got = teb.emulate(pcm, model, output="logmel", **kw)
            assert np.isneginf(got[:, empty]).all()
            worst[n_mel, kind] = eb.check(got, ref, bound, "%s %d / %d %s" % (model, rate, n_mel, kind))
    print("%s at %d Hz: worst error / bound %.3f" % (model, rate, max(worst.values())))      # eb.check holds each to 1


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("model", list(eb.MODELS))
def test_cepstral_bound_is_sound_and_the_pattern_is_the_oracles(wav_pcm, rate, model):
    worst = {}
    for n_mel in (32, 16):
        kw = _kw(rate, n_mel)
        W = mf.mel_filterbank(512, n_mel, rate)
        empty = np.flatnonzero(lb.empty_bands(W))
        assert lb.roundoff_zero_weights(n_mel, n_mel) == []            # a power of two: nothing is set aside
        for kind in kf.KINDS:
            pcm = _pcm(kind, wav_pcm)
            with np.errstate(invalid="ignore"):
                ref, bound = eb.reference_and_bound(pcm, model, n_cep=n_mel, **kw)
            got = teb.emulate(pcm, model, n_cep=n_mel, **kw)
            worst[n_mel, kind] = eb.check(got, ref, bound, "%s %d / %d %s" % (model, rate, n_mel, kind))
            if len(empty):
                assert not np.isfinite(ref).any() and not np.isfinite(got).any()
                assert np.array_equal(got.astype(np.float64), ref, equal_nan=True)
            if len(empty) == 1 and kind in ("speech", "noise", "uniform"):
                sign = -np.sign(mf.dct_basis(n_mel, n_mel)[:, empty[0]])
                assert np.array_equal(ref, np.broadcast_to(sign * np.inf, ref.shape))
    print("%s at %d Hz: worst error / bound %.3f" % (model, rate, max(worst.values())))      # eb.check holds each to 1


def test_roundoff_zero_weights_of_the_dct_basis():
    """k (2 b + 1) = n_mel x odd has no solution with k < n_mel when n_mel is a power of two; at 40 filters the pairs are
    those with k (2 b + 1) in {40, 120, 200, ...}; only they are set aside, and only for an empty band."""
    for n in (16, 32, 64):
        assert lb.roundoff_zero_weights(n, n) == []
    pairs = lb.roundoff_zero_weights(40, 40)
    want = [(k, b) for k in range(40) for b in range(40) if (k * (2 * b + 1)) % 80 == 40]
    assert pairs == want and len(pairs) > 0 and all(k * (2 * b + 1) in range(40, 40 * 80, 80) for k, b in pairs)
    D = mf.dct_basis(40, 40)
    assert min(abs(D[k, b]) for k in range(40) for b in range(40) if (k, b) not in set(pairs)) > 1e-3
    W = mf.mel_filterbank(1024, 40, 192000)
    assert np.flatnonzero(lb.empty_bands(W)).tolist() == [1, 4]
    full = np.full((3, 40), np.nan)
    # bands 1 and 4 pair with no k < 40 (3 k and 9 k are never 40 x odd): the banks the GPU tests run set nothing aside
    assert not [p for p in pairs if p[1] in (1, 4)] and lb.free_roundoff_coefficients(full, W, 40) is full
    assert lb.free_roundoff_coefficients(full, mf.mel_filterbank(1024, 40, 16000), 40) is full
    W = W.copy()
    W[2] = 0                                                     # band 2: 5 k = 40, 120 -> k = 8, 24
    b = lb.free_roundoff_coefficients(full, W, 40)
    assert np.isposinf(b[:, [8, 24]]).all() and np.isnan(np.delete(b, [8, 24], axis=1)).all()
    assert np.isposinf(lb.free_roundoff_coefficients(full[:, :13], W, 13)[:, 8]).all()


# ----------------------------------------------------------------------------- sensitivity

COL15 = r"frame % 16: \[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, [1-9]"


@pytest.mark.parametrize("kind", ["speech", "noise"])
def test_one_value_off_in_one_tile_column_is_flagged_at_96_khz(wav_pcm, kind):
    kw, model = _kw(96000), "bf16x2/fp32"
    pcm = _pcm(kind, wav_pcm)
    ref, bound = lb.reference_and_bound(pcm, model, **kw)
    _, st = mf.mfcc_notebook(pcm, return_stages=True, **kw)
    for band in (0, 2, 17, 31):                                  # finite bands of frames whose band 1 is empty
        assert np.isfinite(ref[:, band]).all() and np.isneginf(ref[:, 1]).all()
        got = teb.emulate(pcm, model, output="logmel", mutant=("coef", 15, band, 1e-3), **kw)
        eb.check(got, ref, _plain_logmel_bound(st, model))      # the gap: the whole-row bound does not see it
        with pytest.raises(AssertionError, match=COL15):
            eb.check(got, ref, bound)


@pytest.mark.parametrize("term", [1, 2])
def test_dropped_mel_split_term_in_column_15_is_flagged_at_96_khz(wav_pcm, term):
    kw, model = _kw(96000), "bf16x2/fp32"
    pcm = _pcm("speech", wav_pcm)
    ref, bound = lb.reference_and_bound(pcm, model, **kw)
    _, st = mf.mfcc_notebook(pcm, return_stages=True, **kw)
    got = teb.emulate(pcm, model, output="logmel", mutant=("mel", term), **kw)
    assert np.isneginf(got[:, 1]).all()
    eb.check(got, ref, _plain_logmel_bound(st, model))
    with pytest.raises(AssertionError, match=COL15):
        eb.check(got, ref, bound)


def test_a_finite_value_in_the_empty_column_is_flagged(wav_pcm):
    kw, model = _kw(96000), "fp32/fp32"
    pcm = _pcm("noise", wav_pcm)
    ref, bound = lb.reference_and_bound(pcm, model, **kw)
    got = teb.emulate(pcm, model, output="logmel", **kw)
    got[20, 1] = -150.0
    with pytest.raises(AssertionError, match="pattern"):
        eb.check(got, ref, bound)


# ----------------------------------------------------------------------------- framed and HTK references

def test_framed_and_banked_references_bound_per_band(wav_pcm):
    for kind in ("speech", "noise", "uniform"):
        pcm = kf.signal(kind, 160 * 36 + 400, 3, wav_pcm)
        for model in ("bf16x2/fp32", "fp32/fp32"):
            ref, bound = fr.reference_and_bound(pcm, model, 400, 160, sample_rate=192000, output="logmel")
            lb.assert_not_blind(bound, mf.mel_filterbank(512, 32, 192000), kind)
            assert np.isneginf(ref[:, [0, 2, 4]]).all()
            for n_mel, lo, hi, rate, n_empty in ((64, 125.0, 7500.0, 48000, 3), (40, 20.0, None, 96000, 1),
                                                 (40, 0.0, None, 192000, 3)):
                W = mr.matrix(512, n_mel, rate, lo, hi)
                assert lb.empty_bands(W).sum() == n_empty
                ref, bound = mr.reference_and_bound(pcm, model, 400, 160, n_mel=n_mel, sample_rate=rate, low=lo,
                                                    high=hi, output="logmel")
                lb.assert_not_blind(bound, W, "%s htk %d at %d" % (kind, n_mel, rate))
                assert np.isneginf(ref[:, lb.empty_bands(W)]).all()


# ----------------------------------------------------------------------------- the GPU tests' own inputs

def test_the_gpu_cases_are_not_blind(wav_pcm):
    """Every float case of tests/test_gpu_sample_rates.py, on the channels it bounds: the condition the GPU tests assert
    again before they look at a kernel's output."""
    import sample_rate_cases as sc
    cases = sc.all_float_cases()
    assert len({c.id for c in cases}) == len(cases) > 150
    with_empty = 0
    for case in cases:
        sc.assert_not_blind(case, wav_pcm)
        with_empty += bool(lb.empty_bands(case.filters()).any())
    assert with_empty >= 40
