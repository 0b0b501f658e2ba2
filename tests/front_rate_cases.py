"""The cases of tests/test_gpu_front_rates.py and tests/test_front_rates_host.py: fronted handles -- a window function
and a pre-emphasis pair other than (periodic Hamming, 31/32) -- at the sample rates where the mel bank changes the form of
a kernel, their inputs, and the float64 reference and bound of every channel -- TEST INFRASTRUCTURE ONLY (a plain
module, no GPU).

1.  Fronts x sample rates.  ``cases()`` is one handle per form (sparse, dense, dense + DCX, empty band, the generic
    kernel's ``window_d`` loop, the bank kernel's set masks), ``FRONTS`` the five non-default fronts of
    ``front_ref.FRONTS``.  The reference is ``front_ref.reference_and_bound`` at the case's rate; the limit is 1.0 x the
    project's bounds.  Inputs: ``sample_rate_cases.KINDS`` at 37 frames.

2.  The DC bin itself.  ``dc_reference_and_bound`` bounds the log-mel value of the bands with weight on bin 0 from the
    arithmetic the kernels state for that bin: the sum ``X[0] = sum (w / den) e`` in double (``N 2^-53 sum |w e|``), one
    fp32 rounding of its square, every other bin under ``spectrum_ref.bound``, the contraction and the log2 as
    ``oracle/error_bound.py`` and tests/logmel_bound.py model them.  The section-1 bound allows bin 0 the error of an
    fp32 FFT, ``e = u rms(X) log2(nfft)``, whatever ``|X[0]|`` is.

    What that gains over section 1 (tests/test_front_rates_host.py measures and prints both bounds for every case, front
    and channel).  ``const_min`` and ``dc_dither`` put the frame's energy INTO bin 0: there ``rms(X) <= |X[0]|``, the fp32
    FFT's allowance ``2 |X[0]| e`` is already below one fp32 rounding of ``P[0]``, and wherever both bounds are finite
    their ratio is between 0.994 and 1.02.  A factor of 8 between them is not to be had on such inputs.  Section 2 is a
    check of its own in two places: where section 1 gives the whole row up -- under a constant at ``L = nfft`` every band
    away from DC is roundoff of an exact zero, so ``eb.bound_from_stages`` returns +inf for the frame, and section 2 still
    pins its DC bands, to 1.1e-5 log2 units on the log-mel handles -- and where bin 0 is small against the frame: the
    ``dc_under_tone`` channel, a +-31000 square wave of period 8 (bins nfft / 8 and 3 nfft / 8) on a constant of
    ``TONE_CONST``.  There, on the log-mel handles under the fronts with pre-emphasis, section 1 is 19 (``(povey, 32/33)``
    on mfcc_fused512_h160_kernel) to 2600 times looser behind frame 0.  ``DC_RATIO`` = 8 is asserted on exactly those
    triples (``gains`` in the host test); every other triple is held to the section-2 bound all the same.

3.  Routes.  ``boundary_utterances`` builds utterances that end on +32767 and start on -32768.

4.  Loud inputs.  ``nyquist`` and ``corners`` reach ``max |e| = den 32768 + num 32767``.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import front_ref as fr
import kernel_families as kf
import logmel_bound as lb
import melbank_ref as mr
import sample_rate_cases as sc
import spectrum_ref as sr
import test_rate_map_host as rmap
from oracle import error_bound as eb
from oracle import mfcc_float as mf

NFR = sc.NFR
KINDS = sc.KINDS
BOUNDED = sc.BOUNDED
GENERIC, W4, H160, H160MB = sc.GENERIC, sc.W4, sc.H160, sc.H160MB

FRONTS = [f for f in fr.FRONTS if not fr.is_default(f)]
R = ("rectangular", True, (63, 64))              # w[0] = 1 at the fused limit num + den = 127
G = ("hamming", False, (97, 100))                # the generic kernels, w[0] = 0.08
POVEY = ("povey", False, (32, 33))
QUIET = ("rectangular", True, (1, 126))          # section 4: the fused limit with the weight on den
LOUD_GENERIC = ("rectangular", True, (127, 128))  # section 4: the generic kernels' limit num + den = 255
assert R in FRONTS and G in FRONTS and POVEY in FRONTS and len(FRONTS) == 5


@dataclass(frozen=True)
class Case:
    id: str
    fused: str                                   # the kernel of a front whose pair the fused kernels serve
    kw: dict = field(hash=False)                 # MFCC() arguments without the front

    def kernel(self, front):
        return self.fused if fr.fused_pair(front) else GENERIC

    def model(self, front):
        return "fp32/fp32" if self.kernel(front) == GENERIC else "bf16x2/fp32"

    @property
    def logmel(self):
        return self.kw.get("output") == "logmel"

    @property
    def frame_len(self):
        return self.kw.get("win_length") or self.kw["nfft"]

    @property
    def n_samples(self):
        return self.kw["hop"] * (NFR - 1) + self.frame_len

    @property
    def width(self):
        return self.kw["nfilters"] if self.logmel else self.kw["nceptrums"]

    @property
    def power_scale(self):
        return float(self.kw["power_scale"] or self.kw["nfft"])

    def filters(self):
        kw = self.kw
        if kw.get("mel") == "htk":
            return mr.matrix(kw["nfft"], kw["nfilters"], int(kw["samplerate"]), float(kw["fmin"]), kw["fmax"])
        return mf.mel_filterbank(kw["nfft"], kw["nfilters"], int(kw["samplerate"]))

    def dc_bands(self):
        return np.flatnonzero(self.filters()[:, 0] != 0)


def _with_outputs(name, kernel, kw, logmel=True):
    return [Case("%s %s at %d" % (name, tag, k["samplerate"]), kernel, k) for tag, k in sc._outputs(kw, logmel)]


def cases():
    """One handle per form (the forms are those of tests/test_rate_map_host.py)."""
    out = []
    for rate in (16001, 24000, 64000, 192000, 88200):          # sparse, dense, dense + DCX (twice), an empty band
        for n_cep in (13, 32):
            out += _with_outputs("512/170 32 filters", W4, sc._nb(512, 170, 32, n_cep, rate), logmel=False)
    for rate in (16001, 192000):                               # dense, DCX with block 1 masked
        out += _with_outputs("512/170 16 filters", W4, sc._nb(512, 170, 16, 16, rate), logmel=False)
    for rate in (64000, 88200):                                # the four-wave form has no log-mel tail: window_d
        out.append(Case("512/170 32 filters logmel at %d" % rate, GENERIC,
                        dict(sc._nb(512, 170, 32, 32, rate), output="logmel")))
    for rate, n_mel in ((16001, 32), (64000, 32), (96000, 32), (192000, 16)):
        out += _with_outputs("400/160/512 %d filters" % n_mel, H160, sc._nb(512, 160, n_mel, 13, rate, win_length=400))
    for bank in rmap.HTK_BANKS:
        out += [Case(c.id, H160MB, c.kw) for c in sc.cases_htk(bank, H160MB)]
    for rate in (16001, 96000, 192000):                        # no DC weight, DC_1024, DC weight and two empty bands
        for n_cep in (13, 40):
            out += _with_outputs("1024/341 40 filters", GENERIC, sc._nb(1024, 341, 40, n_cep, rate), logmel=n_cep == 40)
    assert len({c.id for c in out}) == len(out)
    return out


def stream_cases():
    """One case per kernel family for the ``stream`` framing with ``halo=1``: a DCX form where the family has one."""
    by_id = {c.id: c for c in cases()}
    return [by_id["512/170 32 filters cep32 at 64000"], by_id["400/160/512 32 filters logmel at 64000"],
            by_id["htk40_96k (set mask 53) cep13 on %s" % H160MB], by_id["1024/341 40 filters logmel at 96000"]]


# ------------------------------------------------------------------------------------------------ inputs, references

_REF = {}


def pcm_of(case, wav_pcm):
    """int16 (len(KINDS), n), read-only: the channels of tests/sample_rate_cases.py at the case's length."""
    return sc.pcm_of(case, wav_pcm)


def _ref_args(case, front):
    kw = case.kw
    return dict(model=case.model(front), front=front, L=case.frame_len, hop=kw["hop"], nfft=kw["nfft"],
                n_mel=kw["nfilters"], sample_rate=int(kw["samplerate"]), power_scale=case.power_scale,
                n_cep=kw["nceptrums"], output="logmel" if case.logmel else "cepstra",
                filters=case.filters() if kw.get("mel") == "htk" else None)


def reference_of(case, front, x, pad_mode="notebook", halo=0):
    """(ref, bound) of one channel ``x``: ``front_ref.reference_and_bound`` at the case's rate; cepstra on a bank with
    empty bands leave the roundoff-zero columns free, as ``sample_rate_cases.reference`` does."""
    args = _ref_args(case, front)
    with np.errstate(invalid="ignore"):
        ref, bound = fr.reference_and_bound(x, pad_mode=pad_mode, halo=halo, **args)
    if not case.logmel:
        bound = lb.free_roundoff_coefficients(bound, case.filters(), case.kw["nceptrums"])
        empty = lb.empty_bands(case.filters())
        if empty.any() and len(ref):
            # With an empty band ``eb.bound_from_stages`` pins every frame to the oracle's +-inf / NaN.  Whether a
            # coefficient is an infinity or NaN then depends on which OTHER bands are -inf too, and a band whose error
            # bound reaches its energy (float64 roundoff of an exact zero: every band away from DC of a constant under a
            # window without a pedestal) may be -inf in either arithmetic.  Without an empty band eb leaves such a frame
            # unconstrained (+inf); the same rule holds here, read from the per-band log-mel bound of the same stages.
            with np.errstate(invalid="ignore"):
                _, per_band = fr.reference_and_bound(x, pad_mode=pad_mode, halo=halo, **dict(args, output="logmel"))
            bound = np.array(bound, dtype=np.float64)
            bound[np.isposinf(per_band[:, ~empty]).any(axis=1)] = np.inf
    return ref, bound


def reference(case, front, wav_pcm, c, pad_mode="notebook", halo=0):
    """(ref, bound) of channel ``c`` of ``pcm_of``: float64, read-only, computed once."""
    key = (case.id, front, c, pad_mode, halo)
    if key not in _REF:
        ref, bound = reference_of(case, front, pcm_of(case, wav_pcm)[c], pad_mode, halo)
        if (pad_mode, halo) == ("notebook", 0):
            assert ref.shape == bound.shape == (NFR, case.width), (case.id, ref.shape)
        ref.setflags(write=False)
        bound.setflags(write=False)
        _REF[key] = (ref, bound)
    return _REF[key]


def assert_not_blind(case, front, wav_pcm, pad_mode="notebook", halo=0):
    """``sample_rate_cases.assert_not_blind`` with a front: on the three bounded channels a log-mel bound is finite
    exactly outside the empty bands, a cepstral bound is finite everywhere on a bank without an empty band, and with one
    every coefficient is pinned to the oracle's +-inf / NaN."""
    W = case.filters()
    empty = lb.empty_bands(W)
    for c, kind in enumerate(KINDS):
        if kind not in BOUNDED:
            continue
        ref, bound = reference(case, front, wav_pcm, c, pad_mode, halo)
        what = "%s %s channel %s" % (case.id, fr.front_id(front), kind)
        if case.logmel:
            lb.assert_not_blind(bound, W, what)
            assert np.isneginf(ref[:, empty]).all() and np.isfinite(ref[:, ~empty]).all(), what
        elif not empty.any():
            assert np.isfinite(bound).all() and np.isfinite(ref).all(), what
        else:
            free = sorted({k for k, b in lb.roundoff_zero_weights(len(empty), case.width) if empty[b]})
            assert np.isnan(np.delete(bound, free, axis=1)).all() and not np.isfinite(ref).any(), what


# ------------------------------------------------------------------------------------------------ 2. the DC bin

DC_FRONTS = [POVEY, R]                            # const_min: e is the constant -(den - num) 32768 behind sample 0
DC_RATIO = 8.0                                    # what section 2 must gain on section 1 to be a check of its own
DC_KINDS = ("const_min", "dc_dither", "dc_under_tone")
TONE_CONST = 150


def dc_channels(n, seed=3):
    """int16 (3, n): constant -32768; 1234 +- 1 (``dc_dither`` of tests/test_error_bound.py); a full-scale square wave of
    period 8 -- bins nfft / 8 and 3 nfft / 8 -- on a constant of ``TONE_CONST``: bin 0 far below the frame's rms."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    tone = np.where((i // 4) % 2 == 0, 31000, -31000) + TONE_CONST
    return np.stack([np.full(n, -32768), 1234 + rng.integers(-1, 2, n), tone]).astype(np.int16)


def dc_cases():
    """The handles of ``cases()`` whose bank has weight on bin 0 and whose output shows single bands: log-mel rows, or
    cepstra of full width (the DCT is then inverted on the CPU, see ``dc_reference_and_bound``) on a bank without an
    empty band."""
    out = []
    for c in cases():
        if not len(c.dc_bands()):
            continue
        if c.logmel or (c.width == c.kw["nfilters"] and not lb.empty_bands(c.filters()).any()):
            out.append(c)
    return out


def dc_reference_and_bound(case, front, x):
    """Of one channel: (log-mel reference (frames, dc bands), the section-2 bound, the section-1 bound), float64.

    Section 2, per band ``b`` with ``W[b, 0] != 0`` (``P`` the reference power, ``u = 2^-24``)::

        dX0  = N 2^-53 sum_i |w_i e_i| / (den power_scale)          the double sum: N fused multiply-adds
        dP0  = (2 sqrt(P_0) dX0 + dX0^2) (1 + u) + u P_0             ... and one fp32 rounding of the square
        dE_b = W_b0 dP0 + sum_{k > 0} W_bk B_spec(P)_k + s_mel E_b   spectrum_ref.bound on the other bins
        dL_b = -log2(1 - dE_b / E_b) + (s_dct + C_ACC u) |L_b| + LOG2_ABS (+ BF16X2_MEL_EXTRA)

    -- the last line is tests/logmel_bound.py's, term for term.  Section 1 is ``lb.bound_from_stages`` in the same
    columns.  A handle that returns cepstra of full width is read through the inverse of the DCT basis,
    ``L = D^-1 c``: ``cepstra_to_logmel`` and its own error term ``|D^-1| (s_dct + C_ACC u) |D| |L|`` in place of the
    ``|L_b|`` term, in both bounds alike."""
    kw = case.kw
    model = case.model(front)
    mel_kind, dct_kind = eb.MODELS[model]
    L_, hop, nfft = case.frame_len, kw["hop"], kw["nfft"]
    _, st = fr.fronted_notebook(np.asarray(x), front, L_, hop, nfft, kw["nfilters"], int(kw["samplerate"]), case.power_scale,
                                case.filters() if kw.get("mel") == "htk" else None)
    W, P, E, L = st["filters"], st["power"], st["mel"], st["logmel"]
    bands = case.dc_bands()
    den = front[2][1]
    e = fr.emphasised_frames(x, front, nfft, hop, L_, "notebook", 0)
    w = fr.window(front[0], L_, front[1])
    dx0 = nfft * 2.0 ** -53 * (np.abs(e) * w[None, :]).sum(axis=1) / (den * case.power_scale)
    dp0 = (2.0 * np.sqrt(P[:, 0]) * dx0 + dx0 * dx0) * (1.0 + eb.U) + eb.U * P[:, 0]
    bspec = sr.bound(P)
    dE = dp0[:, None] * W[bands, 0][None, :] + bspec[:, 1:] @ W[bands, 1:].T + eb._scale(mel_kind) * E[:, bands]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E[:, bands] > 0, dE / np.where(E[:, bands] > 0, E[:, bands], 1.0), np.inf)
        dL = np.where(r < 1.0, -np.log2(np.maximum(1.0 - r, 1e-300)), np.inf)
    extra = lb.LOG2_ABS + (lb.BF16X2_MEL_EXTRA if mel_kind == "bf16x2" else 0.0)
    acc = eb._scale(dct_kind) + eb.C_ACC * eb.U
    with np.errstate(invalid="ignore"):
        first = lb.bound_from_stages(st, model)[:, bands]
    if case.logmel:
        tail = acc * np.abs(L[:, bands])
    else:                                         # read through D^-1: the DCT's own rounding comes back through |D^-1|
        D = st["dct_basis"]
        absL = np.where(np.isfinite(L), np.abs(L), np.inf)
        with np.errstate(invalid="ignore"):
            tail = (acc * (absL @ np.abs(D).T)) @ np.abs(np.linalg.inv(D)).T[:, bands]
        first = first - acc * np.abs(L[:, bands]) + tail
    second = dL + tail + extra
    if not case.logmel:
        # ... and a cepstrum is finite only where every band is: a frame in which the model cannot tell some band from 0
        # (section 1's own rule, ``dE_b >= E_b``) may come back as -inf / NaN in every coefficient, and D^-1 reads nothing
        with np.errstate(invalid="ignore"):
            second[~np.isfinite(lb.bound_from_stages(st, model)).all(axis=1)] = np.inf
    # a frame with a silent band has no finite cepstrum to read a band from: unconstrained, like eb's +inf
    return L[:, bands], np.where(np.isnan(second), np.inf, second), np.where(np.isnan(first), np.inf, first)


def cepstra_to_logmel(cep, n_mel):
    """``D^-1 c`` in float64 of cepstra (..., n_mel) of full width."""
    return np.asarray(cep, np.float64) @ np.linalg.inv(mf.dct_basis(n_mel, n_mel)).T


# ------------------------------------------------------------------------------------------------ 3. routes

def boundary_utterances(L, hop, wav_pcm, seed=21):
    """Six int16 utterances, each ending on +32767 with its successor starting on -32768: a predecessor leaked across a
    boundary moves ``e[0]`` by ``num 32767``.  One is exactly ``L`` samples long, one is shorter than ``L`` (no frame)."""
    lengths = [L + 20 * hop + 3, L, L + 7 * hop, L - 1, L + 33 * hop + hop // 2, L + hop]
    kinds = ["speech", "noise", "uniform", "noise", "speech", "silences"]
    out = []
    for i, (n, k) in enumerate(zip(lengths, kinds)):
        u = kf.signal(k, n, seed + i, wav_pcm).copy()
        u[0], u[-1] = -32768, 32767
        out.append(u)
    return out


# ------------------------------------------------------------------------------------------------ 4. loud inputs

def nyquist(n, phase):
    """+32767, -32768, ... (``phase`` 0) or -32768, +32767, ... (1): ``e`` alternates between ``den 32767 + num 32768``
    and ``-(den 32768 + num 32767)``."""
    return np.where((np.arange(n) + phase) % 2 == 0, 32767, -32768).astype(np.int16)


def corners(n, seed):
    """Random signs at full scale: every pair ``(x[i], x[i-1])`` of ``{32767, -32768}^2``."""
    return np.where(np.random.default_rng(seed).integers(0, 2, n) == 0, 32767, -32768).astype(np.int16)


LOUD_KINDS = ("speech", "nyquist0", "nyquist1", "corners")
LOUD_FRAMES = 33


def loud_channels(n, wav_pcm):
    x = np.stack([kf.signal("speech", n, 11, wav_pcm), nyquist(n, 0), nyquist(n, 1), corners(n, 5)])
    x.setflags(write=False)
    return x


def max_abs_e(x, num, den):
    """``max |den x[i] - num x[i-1]|`` over a stream that starts with history 0."""
    x = np.asarray(x, np.int64)
    return int(np.abs(den * x - num * np.concatenate([[0], x[:-1]])).max())


def preemph8_restated(x0, x1, num, den):
    """``fused_common.hpp: preemph8`` in NumPy: the int32 dot product ``den x0 - num x1`` added to 0x4B400000, the bits
    viewed as float32, minus 12582912.0f."""
    acc = np.int64(0x4B400000) + den * np.asarray(x0, np.int64) - num * np.asarray(x1, np.int64)
    bits = (acc & 0xFFFFFFFF).astype(np.uint32)
    return bits.view(np.float32) - np.float32(12582912.0)


def fmaf_restated(x0, x1, num, den):
    """``kernels_generic.hpp: gen_stage_frame`` in NumPy: ``fmaf(-num, x1, den * x0)`` -- the product ``den x0`` rounded
    to fp32, then one fused multiply-add (every term is an integer below 2^53, so float64 holds the sum exactly and the
    conversion is the single rounding)."""
    prod = (np.float32(den) * np.asarray(x0, np.float32)).astype(np.float32)
    return (prod.astype(np.float64) - float(num) * np.asarray(x1, np.float64)).astype(np.float32)
