"""Loud inputs for the fixed-point path, and what they reach in its integer stages -- TEST INFRASTRUCTURE ONLY (a plain
module, no GPU).

Pre-emphasis (mfcc/core/preemph.py:18-28) takes most of a loud signal's low-frequency energy away before the FFT, and
the FFT divides by nfft, so full-scale PCM still gives the FFT quiet input: ``re^2 + im^2`` stays below 2^22 on speech,
noise, squares and constant inputs.  But pre-emphasis is a bijection modulo 2^16: for any int16 sequence ``y`` there is
PCM ``x`` with ``wrap16(x[n] + (x[n-1] >> 5) - x[n-1]) == y[n]``, namely

    x[n] = wrap16(y[n] - (x[n-1] >> 5) + x[n-1]),    x[-1] = 0  (the oracle's reset state).

``STIMULI`` are written on the pre-emphasised side and passed through that inversion, so the window, the FFT, the
power field, the filterbank sums, the log and the DCT see what was written: up to ``(511/512 * 0.54 * 32768)^2 =
2^28.2`` at the power stage in bin 0, and up to ``(0.54 * 2 / pi * 32768)^2 = 2^26.9`` in the bins a filter reads.
``reach`` measures, on the oracle's own stage outputs, how far an input gets.
"""
from __future__ import annotations

import numpy as np

from oracle import mfcc_fixed as mx


def inv_preemph(y):
    """int16 PCM whose pre-emphasised stream (``oracle.mfcc_fixed.preemph``, previous sample 0 at the start) is ``y``."""
    y = np.asarray(y, dtype=np.int64)
    x = np.zeros(len(y), dtype=np.int64)
    prev = 0
    for n, v in enumerate(y.tolist()):
        prev = ((v - (prev >> 5) + prev + 32768) & 0xFFFF) - 32768
        x[n] = prev
    return x.astype(np.int16)


# ------------------------------------------------------------------------------------------------ stimuli

def _freq(bin512, nfft):
    """Cycles per sample of "bin ``bin512`` of 512", or of bin nfft/2 - 1 for ``"top"``."""
    return (nfft // 2 - 1) / nfft if bin512 == "top" else bin512 / 512.0


def _phase(n, bin512, nfft):
    return 2 * np.pi * _freq(bin512, nfft) * np.arange(n) + np.pi / 4


def _square(bin512):
    def f(n, nfft):
        return inv_preemph(np.where(np.cos(_phase(n, bin512, nfft)) >= 0, 32767, -32767))
    return f


def _cosine(bin512):
    def f(n, nfft):
        return inv_preemph(np.rint(32767 * np.cos(_phase(n, bin512, nfft))))
    return f


def _tone_empty_bands(n, nfft):
    """A tone on a high bin, loud enough for ``mel >= 2^15`` in its own band and clean enough (an exact bin, so the
    window's leakage stays within three bins) for the narrow low bands to see ``(re^2 + im^2) >> 2 == 0`` only."""
    k = (nfft * 3) // 8 + 1
    return inv_preemph(np.rint(6000 * np.cos(2 * np.pi * k * np.arange(n) / nfft + 0.3)))


def _loud_silent(n, nfft):
    """One hop in four at -32768, the rest digital silence on the pre-emphasised side: of every four frames one sees
    zeros only and the others hold the loud hop at their start, middle or end."""
    hop = nfft // 3
    return inv_preemph(np.where((np.arange(n) // hop) % 4 == 0, -32768, 0))


def _noise(n, nfft):
    return inv_preemph(np.random.default_rng(nfft).integers(-32768, 32768, n))


def _nyquist(n, nfft):
    """NOT inverted: +32767 / -32768 alternating as PCM, every sample but the first wraps in pre-emphasis itself."""
    return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)


BINS = (1, 37, 100.5, "top")
_BIN_ID = {1: "b1", 37: "b37", 100.5: "b100h", "top": "top"}

STIMULI = {
    "const_min": lambda n, nfft: inv_preemph(np.full(n, -32768)),
    "const_max": lambda n, nfft: inv_preemph(np.full(n, 32767)),
}
STIMULI.update({"square_" + _BIN_ID[b]: _square(b) for b in BINS})
STIMULI.update({"cos_" + _BIN_ID[b]: _cosine(b) for b in BINS})
# between bins 123 and 124: with it, bit 24 of the power field shows in the output of every shape (observable_power_bits)
STIMULI["square_b123h"] = _square(123.5)
STIMULI.update({"tone_empty_bands": _tone_empty_bands, "loud_silent": _loud_silent, "noise": _noise,
                "nyquist": _nyquist})
NAMES = list(STIMULI)


def n_samples(nfft, n_frames, pad="notebook"):
    """Samples that give ``n_frames`` frames at hop nfft // 3 (STREAM: the last one zero-padded by half a hop)."""
    hop = nfft // 3
    if pad == "notebook":
        return hop * (n_frames - 1) + nfft
    return hop * (n_frames - 2) + nfft + hop // 2


def stack(n, nfft, names=None):
    """The stimuli as channels: int16 (len(names), n)."""
    return np.stack([STIMULI[k](n, nfft) for k in (NAMES if names is None else names)])


# ------------------------------------------------------------------------------------------------ reach

def fft_counting_wraps(xr, size, width=16):
    """``oracle.mfcc_fixed.fft_fixed`` restated with a counter: (re, im, per-stage count of butterfly outputs that did
    not fit 16 bits before ``wrap16``)."""
    L = size.bit_length() - 1
    bias = (1 << (width - 3)) - 1
    twr_rom, twi_rom = mx.twiddle_rom(size, width)
    xr = np.asarray(xr, dtype=np.int64)
    re = np.zeros_like(xr)
    re[..., mx._bitrev(L)] = xr
    im = np.zeros_like(re)
    t = np.arange(size // 2)
    wraps = []
    for s in range(L):
        j = t & ((1 << s) - 1)
        i0 = ((t >> s) << (s + 1)) | j
        i1 = i0 + (1 << s)
        ta = (j << (L - 1 - s)) & (size // 2 - 1)
        twr, twi = twr_rom[ta], twi_rom[ta]
        x0r, x0i, x1r, x1i = re[..., i0], im[..., i0], re[..., i1], im[..., i1]
        m0 = (x1r + x1i) * twr + bias
        a1 = (m0 - x1i * (twr + twi)) >> (width - 2)
        a2 = (m0 - x1r * (twr - twi)) >> (width - 2)
        outs = [(x0r + a1) >> 1, (x0i + a2) >> 1, (x0r - a1) >> 1, (x0i - a2) >> 1]
        wraps.append(int(sum(((o < -32768) | (o > 32767)).sum() for o in outs)))
        nr, ni = np.empty_like(re), np.empty_like(im)
        nr[..., i0], ni[..., i0], nr[..., i1], ni[..., i1] = [mx.wrap16(o) for o in outs]
        re, im = nr, ni
    return re[..., :size // 2], im[..., :size // 2], wraps


def reach(stages):
    """How far an input gets in the integer stages, from ``mfcc_fixed_ref(..., return_stages=True)[1]`` alone.

    pow_max          largest ``re^2 + im^2`` before pow2.py:32's shift, recomputed from fft_re / fft_im
    pow_max_read     the same over the bins a filter reads: not bin 0 (no filter starts before bin 1) and not the last
                     bin (filterbank.py:120-142 emits the last filter before that bin's product is added)
    re_max, im_max   largest magnitude of either FFT part
    both_parts       the best bin's smaller part: max over bins of min(max |re|, max |im|) taken over the frames
    loud_zero_mel    mel values equal to 0 in frames whose largest mel is at least 2^15
    mel_or           the OR of all mel values
    log_max          largest log value
    preemph_over / preemph_under   pre-emphasis sums above 32767 / below -32768 (the PCM is recovered from the
                     pre-emphasised stream: the inversion is exact)
    fft_wraps, dct_wraps           butterfly outputs of the FFT-nfft / DCT-FFT that did not fit 16 bits, all stages
    """
    re, im = np.asarray(stages["fft_re"], np.int64), np.asarray(stages["fft_im"], np.int64)
    mel = np.asarray(stages["mel"], np.int64)
    y = np.asarray(stages["preemph"], np.int64)
    x = inv_preemph(y).astype(np.int64)
    o = np.concatenate([np.zeros(1, np.int64), x[:-1]])
    v = x + (o >> 5) - o
    assert np.array_equal(mx.wrap16(v), y)
    nfft = stages["windowed"].shape[-1]
    r2, i2, fw = fft_counting_wraps(stages["windowed"], nfft)
    assert np.array_equal(r2, re) and np.array_equal(i2, im), "the restated FFT is not the oracle's"
    lg = np.asarray(stages["log"], np.int64)
    nfil = lg.shape[-1]
    z = np.zeros(lg.shape[:-1] + (4 * nfil,), dtype=np.int64)
    k = np.arange(nfil)
    z[..., 2 * k + 1] = lg
    z[..., 4 * nfil - 1 - 2 * k] = lg
    d2, _, dw = fft_counting_wraps(z, 4 * nfil)
    assert np.array_equal(d2[..., :nfil], stages["dct"]), "the restated DCT FFT is not the oracle's"
    empty = not len(re)
    loud = mel.max(axis=1) >= (1 << 15) if not empty else np.zeros(0, bool)
    return dict(
        pow_max=0 if empty else int((re * re + im * im).max()),
        pow_max_read=0 if empty else int((re * re + im * im)[:, 1:-1].max()),
        re_max=0 if empty else int(np.abs(re).max()),
        im_max=0 if empty else int(np.abs(im).max()),
        both_parts=0 if empty else int(np.minimum(np.abs(re).max(axis=0), np.abs(im).max(axis=0)).max()),
        loud_zero_mel=int((mel[loud] == 0).sum()),
        mel_or=0 if empty else int(np.bitwise_or.reduce(mel.reshape(-1))),
        log_max=0 if empty else int(lg.max()),
        preemph_over=int((v > 32767).sum()),
        preemph_under=int((v < -32768).sum()),
        fft_wraps=int(sum(fw)),
        dct_wraps=int(sum(dw)),
    )


def observable_power_bits(stages, nfft, nfilters, bits=range(17, 30)):
    """The bits of the 30-bit power field whose loss would change a mel value of this input.  The filterbank keeps bits
    31 .. 46 of ``sum(weight * power)`` with weights of up to 2^30 (filterbank.py:120-142), so at a bin of full weight
    -- a filter's peak -- bits 17 and up of the power never show; they show through the fractional weights of the
    slopes only.  A loud bin has to sit on a slope for a kernel's mistake in its top bits to reach the output."""
    p = np.asarray(stages["power"], np.int64)
    return [j for j in bits
            if (mx.filterbank(p & ~(1 << j), nfft, nfilters) != stages["mel"]).any()]


MARKS_MAX = ("pow_max", "pow_max_read", "re_max", "im_max", "both_parts", "log_max")
MARKS_SUM = ("loud_zero_mel", "preemph_over", "preemph_under", "fft_wraps", "dct_wraps")


def union(reaches):
    """The marks of several inputs together."""
    reaches = list(reaches)
    out = {k: max(r[k] for r in reaches) for k in MARKS_MAX}
    out.update({k: sum(r[k] for r in reaches) for k in MARKS_SUM})
    out["mel_or"] = int(np.bitwise_or.reduce([r["mel_or"] for r in reaches]))
    return out


_REACH = {}


def reach_of_stimuli(nfft, nfilters, n_frames=9):
    """name -> reach of every stimulus at ``nfft`` / ``nfilters``, 16 kHz, ``n_frames`` notebook frames; computed once."""
    key = (nfft, nfilters, n_frames)
    if key not in _REACH:
        n = n_samples(nfft, n_frames)
        _REACH[key] = {k: reach(mx.mfcc_fixed_ref(f(n, nfft), nfft=nfft, nfilters=nfilters, nceptrums=nfilters,
                                                  pad_mode="notebook", return_stages=True)[1])
                       for k, f in STIMULI.items()}
    return _REACH[key]
