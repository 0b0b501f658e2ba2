"""Every instantiation of the four fused 1024/341/40 kernels, by name, in one place: the 3 + 3 of
mfcc_fused1024_w12bf_kernel<VAR, LOGMEL> (the default), the 5 of mfcc_fused1024_w12_kernel<R> (MFCC_HIP_FUSED1024=w12) and
the 5 + 3 of the two mfcc_fused1024_kernel (=f32, =bf16).  The four share their helpers and table code
(fused1024_common.hpp) and the two twelve-wave ones are two copies of one loop, so a change made
to one copy and not to the other shows here.

Shape: 2 channels of 37 frames at an odd channel stride behind an odd base offset -- three 16-frame tiles per channel, the
last one partial.  The six tiles go to three twelve-wave workgroups (one tile for group A, one for group B each) or to six
eight-wave ones.  The steady state of the loops needs more tiles than the launch has workgroups:
tests/test_gpu_steady_state.py runs the forms that way.

Sample rates -> instantiation (proved on the CPU by tests/test_fused1024_tables_host.py):
  bf16 set lists  Sets<0>: 8000, 11025, 16000, 22050    Sets<2>: 32000    Sets<1>: 44100, 48000
  fp32 lists      one Sched<R> each for 8000, 11025, 16000, 22050, 32000; 44100 and 48000 are refused

Nothing here is new arithmetic: every value is held to oracle/error_bound.py under the kernel's declared model
(eb.model_of), log-mel rows through tests/logmel_bound.py, and the reference must bound every frame (speech and noise:
no band of any frame is empty; checked on the CPU when the cases were chosen)."""
import numpy as np
import pytest

import kernel_families as kf
import logmel_bound as lb
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu
NCH, NFR = 2, 37
N = 341 * (NFR - 1) + 1024
SEED = 11
BF_RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000]
F32_RATES = BF_RATES[:5]
# form (the value of MFCC_HIP_FUSED1024, None: unset) -> the kernel the handle must report, its rates
FORMS = {
    None: ("mfcc_fused1024_w12bf_kernel", BF_RATES),
    "w12": ("mfcc_fused1024_w12_kernel", F32_RATES),
    "f32": ("mfcc_fused1024_kernel", F32_RATES),
    "bf16": ("mfcc_fused1024_kernel", BF_RATES),
}
CASES = [(form, rate, 32) for form, (_, rates) in FORMS.items() for rate in rates] + [(form, 16000, 13) for form in FORMS]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


_PCM, _REF = {}, {}


def _pcm(wav_pcm):
    if "x" not in _PCM:
        x = kf.channels(N, SEED, wav_pcm, kinds=["speech", "noise"])
        x.setflags(write=False)
        _PCM["x"] = x
    return _PCM["x"]


def _nb(rate):
    """the oracle's arguments; power_scale = nfft is what a handle made with power_scale=0 divides by"""
    return dict(nfft=1024, hop=341, n_mel=40, sample_rate=rate, power_scale=1024.0)


def _reference(pcm, model, rate, n_cep):
    """(ref, bound) of both channels, computed once per (model, rate, n_cep) and left unchanged"""
    key = (model, rate, n_cep)
    if key not in _REF:
        ref, bound = eb.reference_and_bound(pcm, model, n_cep=n_cep, **_nb(rate))
        assert not np.isposinf(bound).any(), "the reference leaves frames unbounded at %d Hz" % rate
        _REF[key] = (ref, bound)
    return _REF[key]


def _view(pcm):
    """``pcm`` (channels, n) on the device at an odd channel stride behind an odd base offset"""
    import torch
    nch, n = pcm.shape
    off, stride = 3, n + 5 + n % 2
    assert stride % 2 == 1
    flat = np.zeros(off + stride * nch + 16, np.int16)
    for c in range(nch):
        flat[off + c * stride: off + c * stride + n] = pcm[c]
    return torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (stride, 1), storage_offset=off)


def _env(monkeypatch, form):
    monkeypatch.delenv("MFCC_HIP_FUSED1024", raising=False)     # read when a handle is made
    if form:
        monkeypatch.setenv("MFCC_HIP_FUSED1024", form)


@pytest.mark.parametrize("form,rate,n_cep", CASES, ids=["%s-%d-%dc" % (f or "default", r, c) for f, r, c in CASES])
def test_cepstra_every_form_and_rate(mfcc_amd, wav_pcm, monkeypatch, form, rate, n_cep):
    kernel = FORMS[form][0]
    _env(monkeypatch, form)
    pcm = _pcm(wav_pcm)
    with mfcc_amd.MFCC(nfft=1024, hop=341, nfilters=40, nceptrums=n_cep, samplerate=rate, power_scale=0) as m:
        assert m.kernel_name() == kernel
        got = kf.as_np(m.process(_view(pcm)))
    assert got.shape == (NCH, NFR, n_cep)
    ref, bound = _reference(pcm, eb.model_of(kernel, form), rate, n_cep)
    worst = eb.check(got, ref, bound, "%s at %d Hz, %d coefficients" % (kernel, rate, n_cep))
    print("%s (%s) at %d Hz, n_cep %d: worst error / bound %.3f" % (kernel, form or "default", rate, n_cep, worst))


@pytest.mark.parametrize("rate", [16000, 32000, 48000])
def test_logmel_default_form_three_set_lists(mfcc_amd, wav_pcm, monkeypatch, rate):
    kernel = FORMS[None][0]
    _env(monkeypatch, None)
    pcm = _pcm(wav_pcm)
    with mfcc_amd.MFCC(nfft=1024, hop=341, nfilters=40, nceptrums=13, samplerate=rate, power_scale=0,
                       output="logmel") as m:
        assert m.kernel_name() == kernel and m.num_features == 40
        got = kf.as_np(m.process(_view(pcm)))
    assert got.shape == (NCH, NFR, 40)
    worst = 0.0
    for c in range(NCH):
        _, bound = lb.reference_and_bound(pcm[c], lb.MODEL[kernel], **_nb(rate))
        assert not np.isposinf(bound).any(), "the reference leaves frames unbounded at %d Hz, channel %d" % (rate, c)
        worst = max(worst, lb.check(got[c], pcm[c], kernel, "log-mel at %d Hz, channel %d" % (rate, c), **_nb(rate)))
    print("%s log-mel at %d Hz: worst error / bound %.3f" % (kernel, rate, worst))
