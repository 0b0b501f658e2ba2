"""The loud end of the fixed-point path's integer range, on the oracle alone (CPU only).

H1  the stimuli of tests/fixed_stimuli.py reach what the suite's older inputs do not: the top bits of the 30-bit power
    field, both FFT parts large in one bin, empty mel bands beside full ones, every mel bit, pre-emphasis wraps in both
    directions;
H2  the vectorised oracle and the structural model (the two independent readings of the RTL source) agree stage by
    stage on every stimulus;
H3  no butterfly output of the FFT-nfft or of the DCT's FFT leaves 16 bits on any stimulus;
H4  the fixed FFT, DCT and log2 stay within a few LSB of float64 on the stimuli.

Conditions on the reference alone: no kernel is involved."""
import numpy as np
import pytest

import fixed_stimuli as fs
from oracle import mfcc_fixed as mx
from oracle import mfcc_fixed_structural as ms
from oracle import mfcc_float as mf

SHAPES = [(512, 32), (64, 4), (256, 16), (512, 8), (512, 16), (1024, 64)]     # kernel_families.FIXED
STAGE_KEYS = ["framed", "windowed", "fft_re", "fft_im", "power", "mel", "log", "dct"]


def _show(tag, r):
    print("%-24s pow 2^%5.2f (read by a filter 2^%5.2f) |re| %5d |im| %5d both %5d  loud mel==0 %4d  mel OR %#06x  log %5d  "
          "preemph wraps +%d -%d  fft wraps %d dct wraps %d"
          % (tag, np.log2(max(r["pow_max"], 1)), np.log2(max(r["pow_max_read"], 1)), r["re_max"], r["im_max"], r["both_parts"],
                                         r["loud_zero_mel"], r["mel_or"], r["log_max"], r["preemph_over"],
                                         r["preemph_under"], r["fft_wraps"], r["dct_wraps"]))


# ------------------------------------------------------------------------------------------------ H1

def test_h1_inversion_is_exact():
    rng = np.random.default_rng(3)
    for y in (rng.integers(-32768, 32768, 3000), np.full(700, -32768), np.full(700, 32767), np.zeros(5)):
        x = fs.inv_preemph(y)
        assert x.dtype == np.int16 and np.array_equal(mx.preemph(x), y)


def test_h1_stimuli_reach_the_loud_end_at_512_32():
    per = fs.reach_of_stimuli(512, 32)
    for k, r in per.items():
        _show(k, r)
    u = fs.union(per.values())
    _show("UNION 512/32", u)
    assert u["pow_max"] >= 1 << 28
    # |X[k]| <= 32768 * sum(w |cos|) / 512 ~ 0.54 * 2 / pi * 32768 = 11 264 off DC, so the two parts cannot both pass
    # 10 000 in one frame; the square on bin 37 turns by 37 * 170 / 512 of a turn per frame and gives each its turn
    assert u["both_parts"] >= 10000
    assert u["loud_zero_mel"] >= 1
    assert u["mel_or"] == 0xFFFF
    assert u["preemph_over"] >= 1 and u["preemph_under"] >= 1


@pytest.mark.parametrize("nfft,nfil", SHAPES[1:], ids=lambda v: str(v))
def test_h1_same_power_mark_at_the_other_shapes(nfft, nfil):
    u = fs.union(fs.reach_of_stimuli(nfft, nfil).values())
    _show("UNION %d/%d" % (nfft, nfil), u)
    assert u["pow_max"] >= 1 << 28
    assert u["mel_or"] == 0xFFFF


@pytest.mark.parametrize("nfft,nfil", SHAPES, ids=lambda v: str(v))
def test_h1_the_loud_bins_are_bins_a_kernel_mistake_would_show_in(nfft, nfil):
    """The 2^28 mark is reached at bin 0 only (the constants), and no filter reads bin 0: off DC
    ``|X[k]| <= 0.54 * 2 / pi * 32768 = 11 264``, so the bins a filter reads stay below 2^26.92, and the squares get
    within 0.03 of that.  And the filterbank shows the top bits of a bin only through fractional weights (see
    ``observable_power_bits``).  So: the stimuli reach 2^26 at a bin that is read, and in every shape, for every bit of
    the power field up to the highest one reachable there (24 after the ``>> 2``), some stimulus changes a mel value
    when that bit alone is lost."""
    n = fs.n_samples(nfft, 9)
    seen = set()
    for f in fs.STIMULI.values():
        _, v = mx.mfcc_fixed_ref(f(n, nfft), nfft=nfft, nfilters=nfil, nceptrums=nfil, pad_mode="notebook",
                                 return_stages=True)
        assert v["power"][:, 1:-1].max() < 1 << 25                  # bit 24 is the highest a read bin can set
        seen |= set(fs.observable_power_bits(v, nfft, nfil, range(17, 25)))
    print("%d/%d: power bits that show in a mel value: %s" % (nfft, nfil, sorted(seen)))
    assert fs.union(fs.reach_of_stimuli(nfft, nfil).values())["pow_max_read"] >= 1 << 26
    assert seen == set(range(17, 25))


def test_h1_the_older_inputs_stay_below_2_22(wav_pcm):
    """Why this file exists: the golden wav, the suite's synthetic speech and the five channels of
    test_fixed_bit_exact_extremes_and_channels -- full-scale noise, a full-scale square, zeros, constant -32768, a sine --
    leave the top seven bits of the power field untouched."""
    rng = np.random.default_rng(5)
    old = {"golden wav": wav_pcm, "synth_pcm(5000, 5001)": mf.synth_pcm(5000, seed=5001),
           "uniform": rng.integers(-32768, 32768, 6000).astype(np.int16),
           "square % 7 < 3": np.where(np.arange(6000) % 7 < 3, 32767, -32768).astype(np.int16),
           "zeros": np.zeros(6000, np.int16), "const -32768": np.full(6000, -32768, np.int16),
           "sine 3000": (3000 * np.sin(np.arange(6000) * 0.3)).astype(np.int16)}
    rs = []
    for k, x in old.items():
        rs.append(fs.reach(mx.mfcc_fixed_ref(x, nceptrums=32, return_stages=True)[1]))
        _show(k, rs[-1])
    u = fs.union(rs)
    _show("UNION older inputs", u)
    assert u["pow_max"] < 1 << 22
    assert u["fft_wraps"] == 0 and u["dct_wraps"] == 0


# ------------------------------------------------------------------------------------------------ H2

H2_CASES = [(512, 32, k) for k in fs.NAMES] + [(512, 16, k) for k in fs.NAMES] + \
           [(nfft, nfil, k) for nfft, nfil in ((256, 16), (1024, 64)) for k in ("const_min", "noise")]


@pytest.mark.parametrize("nfft,nfil,name", H2_CASES, ids=["%d_%d_%s" % c for c in H2_CASES])
def test_h2_vectorised_equals_structural_model(nfft, nfil, name):
    """A stream of three frames (the structural model is scalar Python): every frame, every stage key that
    test_vectorised_equals_structural_model compares."""
    pcm = fs.STIMULI[name](fs.n_samples(nfft, 3), nfft)
    out, v = mx.mfcc_fixed_ref(pcm, nfft=nfft, nfilters=nfil, nceptrums=nfil, pad_mode="notebook", return_stages=True)
    assert len(out) == 3
    st = ms.mfcc_frames(pcm, 3, nfft=nfft, nfilters=nfil, nceptrums=nfil)
    for k in range(3):
        for key in STAGE_KEYS:
            assert np.array_equal(np.array(st[k][key]), v[key][k]), (name, k, key)
        assert np.array_equal(np.array(st[k]["curve"]), v["curve"])
        assert np.array_equal(np.array(st[k]["cep"]), out[k])


# ------------------------------------------------------------------------------------------------ H3

@pytest.mark.parametrize("nfft,nfil", SHAPES, ids=lambda v: str(v))
def test_h3_no_fft_stage_wraps(nfft, nfil):
    """``wrap16`` in fft.py's butterfly never acts, on any stimulus, so a kernel may keep or drop it -- and this says why
    it is unreachable.  A butterfly output is ``(x0 +- rot(x1)) >> 1``: a stage-s value is the 2^s-point DFT of loaded
    samples over 2^s, and what the integers add to that is below 3 LSB per stage (a rounded twiddle's modulus is at
    most 1 + 0.71 / 2^14, which is 1.4 LSB on a full-scale operand and is halved; the ``+ 8191 >> 14`` and the ``>> 1``
    round by less than one LSB each; twiddles 1 and -j are exact).

    * FFT-nfft: the loaded samples are ``(y * curve) >> 9`` with ``curve <= 510`` of 512, at most 32768 * 510 / 512 =
      32640 in magnitude; an average of them times unit phasors is no larger, and 32640 + 3 * 10 < 32767.
    * DCT FFT: the loaded words are log values in [0, 32766] (log.py's ten squarings never set bit 0 of the 15-bit
      result) at the odd addresses and zeros at the even ones.  Bin 0 of every sub-transform goes through twiddle 1
      only: exact floor averages, at most 32766.  Any other bin is unchanged by taking the constant 16383 off every
      word, which leaves words of magnitude at most 16383: at most 16383 + 3 * 8.  The last stage adds the all-zero
      even half to the odd half and halves again."""
    for k, r in fs.reach_of_stimuli(nfft, nfil).items():
        assert r["fft_wraps"] == 0 and r["dct_wraps"] == 0, (k, r)
    curve = mx.window_curve(nfft)
    assert curve.max() <= 510 and (32768 * 510 >> 9) + 3 * 10 < 32767


# ------------------------------------------------------------------------------------------------ H4

# LSB margins of test_bounded_against_float_model.  The log2's own bound is wider than that test's 4 LSB: log.py shifts
# a 16-bit mel down to a 12-bit mantissa (relative error below 2^-11: 1.4427 LSB of 2^-11), every one of the ten
# truncating squarings loses as much again at half the weight of the one before (1.4427 * (1 - 2^-10) LSB together),
# and the ten squarings resolve bits 2^10 .. 2^1 of the Q4.11 result only, which leaves up to 2 LSB: below 4.89 LSB
# in all, every term of one sign (the fixed value is never above the true one).  The stimuli named here come within
# 0.9 LSB of that; the others keep 4.
FFT_LSB, DCT_LSB, LOG_LSB = 6, 4, 4
LOG_LSB_WIDER = {(512, 32, "square_b1"): 1.4427 + 1.4427 * (1 - 2.0 ** -10) + 2}


@pytest.mark.parametrize("nfft,nfil", [(512, 32), (512, 16)], ids=lambda v: str(v))
def test_h4_bounded_against_float_model(nfft, nfil):
    n = fs.n_samples(nfft, 9)
    worst = dict(fft=0.0, dct=0.0, log=0.0)
    for name, f in fs.STIMULI.items():
        _, v = mx.mfcc_fixed_ref(f(n, nfft), nfft=nfft, nfilters=nfil, nceptrums=nfil, pad_mode="notebook",
                                 return_stages=True)
        X = np.fft.fft(v["windowed"].astype(np.float64), axis=1)[:, :nfft // 2] / nfft
        e_fft = max(np.abs(v["fft_re"] - X.real).max(), np.abs(v["fft_im"] - X.imag).max())
        lg = v["log"].astype(np.float64)
        i = np.arange(nfil)
        cosm = np.cos(np.pi * i[:, None] * (2 * i + 1) / (2 * nfil))
        e_dct = np.abs(v["dct"] - (lg[:, None, :] * cosm[None]).sum(-1) / (2 * nfil)).max()
        mel = v["mel"]
        nz = mel > 0
        d_log = v["log"][nz] - 2048.0 * np.log2(mel[nz])
        e_log = np.abs(d_log).max()
        print("%d/%d %-18s LSB from float64: fft %.2f  dct %.2f  log %.2f" % (nfft, nfil, name, e_fft, e_dct, e_log))
        assert e_fft < FFT_LSB, name
        assert e_dct < DCT_LSB, name
        assert e_log < LOG_LSB_WIDER.get((nfft, nfil, name), LOG_LSB), name
        assert d_log.max() < 1e-6, name                               # truncation only: never above the true log2
        assert (v["log"][~nz] == 0).all(), name
        worst = dict(fft=max(worst["fft"], e_fft), dct=max(worst["dct"], e_dct), log=max(worst["log"], e_log))
    print("%d/%d worst LSB from float64: fft %.2f  dct %.2f  log %.2f" % (nfft, nfil, worst["fft"], worst["dct"],
                                                                         worst["log"]))
