"""The cases of tests/test_gpu_sample_rates.py: handles at the sample rates where the mel bank degenerates, their
inputs, and the float64 reference and bound of every channel -- TEST INFRASTRUCTURE ONLY (a plain module, no GPU).

Which kernel a rate must run comes from the map that tests/test_rate_map_host.py proves on the CPU (``rmap``).  The
references are built here, once per (case, channel), so that tests/test_empty_band_bound_host.py can assert the
not-blind condition on exactly the inputs the GPU tests use, without a GPU.

One shape for every case: 37 frames per channel (two full tiles of 16 and a partial one of 5), notebook padding, the
channels ``KINDS``.  ``speech``, ``noise`` and ``uniform`` are bounded under the not-blind condition
(``assert_not_blind``); ``silences`` and ``const_min`` are held to the pattern and to whatever the bound still pins.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import framed_ref as fr
import kernel_families as kf
import logmel_bound as lb
import melbank_ref as mr
import test_rate_map_host as rmap
from oracle import error_bound as eb
from oracle import mfcc_float as mf

NFR = 37
BOUNDED = ("speech", "noise", "uniform")
KINDS = BOUNDED + ("silences", "const_min")

W12, W4 = "mfcc_fused512_w12_kernel", "mfcc_fused512_kernel"
H160, H160MB = "mfcc_fused512_h160_kernel", "mfcc_fused512_h160_mb_kernel"
K1024, K1024_W12, K1024_8 = "mfcc_fused1024_w12bf_kernel", "mfcc_fused1024_w12_kernel", "mfcc_fused1024_kernel"
GENERIC = "mfcc_float_generic_kernel"
# the two kernels eb.model_of does not name: bf16 x 2-split mel contraction, fp32 DCT (tests/test_gpu_framed.py,
# tests/test_gpu_melbank.py: read from their source)
_MODEL = {H160: "bf16x2/fp32", H160MB: "bf16x2/fp32"}


@dataclass(frozen=True)
class Case:
    id: str
    kernel: str
    kw: dict = field(hash=False)                 # MFCC() arguments
    form: str = ""                               # MFCC_HIP_FUSED1024 / MFCC_HIP_FUSED512 of the handle ("" : default)

    @property
    def logmel(self):
        return self.kw.get("output") == "logmel"

    @property
    def model(self):
        if self.logmel and self.kernel in lb.MODEL:
            return lb.MODEL[self.kernel]
        return _MODEL.get(self.kernel) or eb.model_of(self.kernel, self.form or None)

    @property
    def frame_len(self):
        return self.kw.get("win_length") or self.kw["nfft"]

    @property
    def n_samples(self):
        return self.kw["hop"] * (NFR - 1) + self.frame_len

    @property
    def width(self):
        return self.kw["nfilters"] if self.logmel else self.kw["nceptrums"]

    def filters(self):
        kw = self.kw
        if kw.get("mel") == "htk":
            return mr.matrix(kw["nfft"], kw["nfilters"], int(kw["samplerate"]), float(kw["fmin"]), kw["fmax"])
        return mf.mel_filterbank(kw["nfft"], kw["nfilters"], int(kw["samplerate"]))


def _nb(nfft, hop, n_mel, n_cep, rate, **over):
    return dict(nfft=nfft, hop=hop, nfilters=n_mel, nceptrums=n_cep, samplerate=rate,
                power_scale=512.0 if nfft == 512 else 0, **over)


def _outputs(kw, logmel=True):
    return [("cep%d" % kw["nceptrums"], kw)] + ([("logmel", dict(kw, output="logmel"))] if logmel else [])


def cases_512(rate, kernel=W12):
    """512 / hop 170: 32 filters with 13 and 32 cepstra, 16 filters with 16; log-mel rows on the twelve-wave form (the
    four-wave form has no log-mel tail)."""
    out = []
    for n_mel, n_cep in ((32, 13), (32, 32), (16, 16)):
        for tag, kw in _outputs(_nb(512, 170, n_mel, n_cep, rate), logmel=kernel == W12 and n_cep != 13):
            out.append(Case("%s %d/%d %s at %d" % ("w4" if kernel == W4 else "w12", 512, n_mel, tag, rate), kernel, kw,
                            "w4" if kernel == W4 else ""))
    return out


FRAMED = [(12000, 32), (16001, 32), (64000, 32), (96000, 32), (192000, 32), (192000, 16)]


def cases_framed(rate, n_mel):
    kw = _nb(512, 160, n_mel, 13, rate, win_length=400)
    return [Case("h160 %d filters %s at %d" % (n_mel, tag, rate), H160, k) for tag, k in _outputs(kw)]


def cases_htk(bank, kernel):
    n_mel, lo, hi, rate, mask, _ = rmap.HTK_BANKS[bank]
    kw = _nb(512, 160, n_mel, 13, rate, win_length=400, mel="htk", fmin=lo, fmax=hi or None)
    if kernel == GENERIC:
        kw["impl"] = "generic"
    return [Case("%s (set mask %d) %s on %s" % (bank, mask, tag, kernel), kernel, k) for tag, k in _outputs(kw)]


FORMS_1024 = ([("", r) for r in (1000, 12000, 24000, 64000)] + [(f, r) for f in ("w12", "f32") for r in sorted(rmap.F32_1024)]
              + [("generic", r) for r in (37800, 88200, 96000, 192000)])


def cases_1024(form, rate):
    """1024 / 341 / 40 with 13 and 40 cepstra; log-mel on the default form and on the generic kernel the handle falls
    to where every fused builder refuses the rate (``form`` "generic" is what the handle must report, not an argument)."""
    kernel = {"": K1024, "w12": K1024_W12, "f32": K1024_8, "generic": GENERIC}[form]
    env = "" if form == "generic" else form
    out = []
    for n_cep in (13, 40):
        for tag, kw in _outputs(_nb(1024, 341, 40, n_cep, rate), logmel=form in ("", "generic") and n_cep == 40):
            out.append(Case("1024 %s %s at %d" % (form or "default", tag, rate), kernel, kw, env))
    return out


def cases_generic(rate):
    out = []
    for kw in (_nb(256, 85, 20, 13, rate, impl="generic"), _nb(512, 257, 32, 32, rate, impl="generic")):
        out += [Case("generic %d/%d hop %d %s at %d" % (kw["nfft"], kw["nfilters"], kw["hop"], tag, rate), GENERIC, k)
                for tag, k in _outputs(kw)]
    return out


def all_float_cases():
    out = []
    for r in rmap.RATES:
        out += cases_512(r, W12) + cases_512(r, W4)
    for r, n_mel in FRAMED:
        out += cases_framed(r, n_mel)
    for b in rmap.HTK_BANKS:
        out += cases_htk(b, H160MB) + cases_htk(b, GENERIC)
    for form, r in FORMS_1024:
        out += cases_1024(form, r)
    for r in (96000, 384000):
        out += cases_generic(r)
    return out


# ------------------------------------------------------------------------------------------------ inputs, references

_PCM, _REF = {}, {}


def pcm_of(case: Case, wav_pcm):
    """int16 (len(KINDS), n): read-only, one array per length."""
    n = case.n_samples
    if n not in _PCM:
        x = kf.channels(n, 11 + n % 7, wav_pcm, kinds=KINDS)
        x.setflags(write=False)
        _PCM[n] = x
    return _PCM[n]


def reference(case: Case, wav_pcm, c):
    """(ref, bound) of channel ``c``, float64 (NFR, width), read-only; computed once.  Cepstra on a bank with empty
    bands: the columns with a roundoff-zero DCT weight on an empty band are left free (``lb.free_roundoff_coefficients``)."""
    kw = case.kw
    ps = float(kw["power_scale"] or kw["nfft"])
    key = (c, case.model, case.logmel, case.width, ps, tuple(sorted((k, str(v)) for k, v in kw.items()
                                                                   if k not in ("impl", "output", "nceptrums", "power_scale"))))
    if key not in _REF:
        x = pcm_of(case, wav_pcm)[c]
        nb = dict(nfft=kw["nfft"], hop=kw["hop"], n_mel=kw["nfilters"], sample_rate=int(kw["samplerate"]), power_scale=ps)
        with np.errstate(invalid="ignore"):
            if kw.get("mel") == "htk":
                ref, bound = mr.reference_and_bound(x, case.model, case.frame_len, n_cep=kw["nceptrums"], low=float(kw["fmin"]),
                                                    high=kw["fmax"], output="logmel" if case.logmel else "cepstra", **nb)
            elif "win_length" in kw:
                ref, bound = fr.reference_and_bound(x, case.model, case.frame_len, n_cep=kw["nceptrums"],
                                                    output="logmel" if case.logmel else "cepstra", **nb)
            elif case.logmel:
                ref, bound = lb.reference_and_bound(x, case.model, **nb)
            else:
                ref, bound = eb.reference_and_bound(x, case.model, n_cep=kw["nceptrums"], **nb)
        if not case.logmel:
            bound = lb.free_roundoff_coefficients(bound, case.filters(), kw["nceptrums"])
        assert ref.shape == bound.shape == (NFR, case.width), (case.id, ref.shape)
        ref.setflags(write=False)
        bound.setflags(write=False)
        _REF[key] = (ref, bound)
    return _REF[key]


def assert_not_blind(case: Case, wav_pcm):
    """The cap on what the bound may give up, on the three bounded channels.  Log-mel: ``lb.assert_not_blind``.  Cepstra:
    without an empty band every coefficient has a finite bound; with one every coefficient is pinned to the oracle's
    +-inf / NaN (bound NaN), the roundoff-zero columns -- none on the banks here -- apart."""
    W = case.filters()
    empty = lb.empty_bands(W)
    for c, kind in enumerate(KINDS):
        if kind not in BOUNDED:
            continue
        ref, bound = reference(case, wav_pcm, c)
        what = "%s channel %s" % (case.id, kind)
        if case.logmel:
            lb.assert_not_blind(bound, W, what)
            assert np.isneginf(ref[:, empty]).all() and np.isfinite(ref[:, ~empty]).all(), what
        elif not empty.any():
            assert np.isfinite(bound).all() and np.isfinite(ref).all(), what
        else:
            free = sorted({k for k, b in lb.roundoff_zero_weights(len(empty), case.width) if empty[b]})
            assert np.isnan(np.delete(bound, free, axis=1)).all() and not np.isfinite(ref).any(), what
