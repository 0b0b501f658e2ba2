"""Every kernel where the sample rate degenerates the mel bank, on the GPU.

``sample_rate`` is a free integer; the mel matrix built from it picks the instantiation of each fused kernel and, in
places, whether a fused kernel runs at all.  The other GPU tests use seven common rates.  Here the rates of
``test_rate_map_host.RATES`` run -- 1 kHz to 384 kHz -- and with them what only uncommon rates reach: structurally
empty filters (log-mel -inf in that column of every frame, cepstra +-inf or NaN by the DCT's signs: from 88.2 kHz at
512 / 32, in VGGish's bank on 48 kHz audio), the exact-DC path of the 16-filter instantiation (from 176.4 kHz), the
sparse 512 tables on matrices other than the 16 kHz one, every set list and schedule of the 1024 builders, and the
generic kernel where every fused 1024 builder refuses the rate (its double-precision DC sum at 1024 points).

Which kernel a rate must run is imported from tests/test_rate_map_host.py, which proves the map on the CPU; every test
asserts ``kernel_name()`` before anything else.  Float results are held value by value to the float64 reference under
the kernel's declared model (``eb.check`` / ``lb.check`` / ``fr.check`` / ``mr.check``), with the per-band log-mel
bound of tests/logmel_bound.py; before a test looks at a kernel's output it asserts that the bound is not blind
(tests/sample_rate_cases.py).  Fixed results are the RTL oracle's bit for bit.

One shape: 37 frames per channel (two tiles of 16 and one of 5), notebook padding, channels on an odd stride behind an
odd base offset."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fixed_stimuli as fs
import framed_ref as fr
import logmel_bound as lb
import melbank_ref as mr
import sample_rate_cases as sc
import test_rate_map_host as rmap
from kernel_families import as_np, same
from oracle import error_bound as eb
from oracle import mfcc_fixed as mx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCH = len(sc.KINDS)


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _strided(pcm):
    """The channels of ``pcm`` on an odd stride behind an odd base offset, as a device view."""
    import torch
    nch, n = pcm.shape
    off, stride = 3, n + 5 + (n % 2 == 0)
    flat = np.zeros(off + stride * nch + 8, pcm.dtype)
    for c in range(nch):
        flat[off + c * stride: off + c * stride + n] = pcm[c]
    return torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (stride, 1), storage_offset=off)


def _check(case, got, wav_pcm):
    """``got`` (channels, 37, width) against the case's reference; returns the worst error / bound ratio."""
    sc.assert_not_blind(case, wav_pcm)                      # before the kernel's output is looked at
    got = as_np(got)
    assert got.shape == (NCH, sc.NFR, case.width) and got.dtype == np.float32, (case.id, got.shape)
    check = mr.check if case.kw.get("mel") == "htk" else fr.check if "win_length" in case.kw else eb.check
    worst = 0.0
    for c, kind in enumerate(sc.KINDS):
        ref, bound = sc.reference(case, wav_pcm, c)
        worst = max(worst, check(got[c], ref, bound, "%s channel %s" % (case.id, kind)))
    print("%s: worst error / bound %.3f" % (case.id, worst))
    return worst


def _run(mfcc_amd, case, wav_pcm):
    with mfcc_amd.MFCC(**case.kw) as m:
        assert m.kernel_name() == case.kernel, (case.id, m.kernel_name())
        assert m.num_frames(case.n_samples) == sc.NFR
        got = m.process(_strided(sc.pcm_of(case, wav_pcm)))
        return _check(case, got, wav_pcm)


# ------------------------------------------------------------------------------------------------ float, 512 / hop 170

@pytest.mark.parametrize("rate", rmap.RATES)
def test_fused512_twelve_wave_form_at_every_rate(mfcc_amd, wav_pcm, rate):
    """mfcc_fused512_w12_kernel: sparse tables at 12000 / 16001, dense elsewhere, the exact-DC path from 64 kHz (32
    filters) and from 176.4 kHz (16 filters: DENSE + DCX with block 1 masked), empty bands from 88.2 kHz -- there every
    tile takes the fp32 DCT chain in frames whose other bands are finite."""
    for case in sc.cases_512(rate, sc.W12):
        _run(mfcc_amd, case, wav_pcm)


def test_fused512_four_wave_form_at_every_rate(mfcc_amd, wav_pcm, tmp_path):
    """mfcc_fused512_kernel through MFCC_HIP_FUSED512=w4 (read when a handle is made), in one child process."""
    cases = [c for r in rmap.RATES for c in sc.cases_512(r, sc.W4)]
    pcm = sc.pcm_of(cases[0], wav_pcm)
    np.save(tmp_path / "in.npy", pcm)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import mfcc_amd\n"
            "x = np.load(%r)\n"
            "out = {}\n"
            "for i, kw in enumerate(%r):\n"
            "    with mfcc_amd.MFCC(**kw) as m:\n"
            "        assert m.kernel_name() == 'mfcc_fused512_kernel', (kw, m.kernel_name())\n"
            "        out['c%%d' %% i] = m.process(x)\n"
            "np.savez(%r, **out)\n"
            % (ROOT, str(tmp_path / "in.npy"), [c.kw for c in cases], str(tmp_path / "out.npz")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MFCC_HIP_FUSED512="w4"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    for i, case in enumerate(cases):
        _check(case, out["c%d" % i], wav_pcm)


# ------------------------------------------------------------------------------------------------ float, 400 / 160 / 512

@pytest.mark.parametrize("rate,n_mel", sc.FRAMED)
def test_fused512_hop160_form(mfcc_amd, wav_pcm, rate, n_mel):
    """mfcc_fused512_h160_kernel: sparse at 12000 / 16001, DCX at 64 kHz, DCX and empty bands at 96 / 192 kHz."""
    assert (rate in rmap.SPARSE_512) == (rate in (12000, 16001)) and (rate in rmap.DC_EXACT[n_mel]) == (rate >= 64000)
    for case in sc.cases_framed(rate, n_mel):
        _run(mfcc_amd, case, wav_pcm)


@pytest.mark.parametrize("kernel", [sc.H160MB, sc.GENERIC])
@pytest.mark.parametrize("bank", list(rmap.HTK_BANKS))
def test_htk_banks_with_empty_filters(mfcc_amd, wav_pcm, bank, kernel):
    """VGGish's 64 bands over 125 - 7500 Hz on 48 kHz audio (three empty filters), 40 bands from 20 Hz at 96 kHz (one),
    40 from 0 Hz at 192 kHz (three): the bank kernel under the set mask the host map gives, and the generic kernel."""
    assert len(rmap.HTK_BANKS[bank][5]) == int(lb.empty_bands(sc.cases_htk(bank, kernel)[0].filters()).sum()) > 0
    for case in sc.cases_htk(bank, kernel):
        _run(mfcc_amd, case, wav_pcm)


# ------------------------------------------------------------------------------------------------ float, 1024 / 341 / 40

@pytest.mark.parametrize("form,rate", sc.FORMS_1024)
def test_fused1024_forms_and_the_generic_fallback(mfcc_amd, wav_pcm, monkeypatch, form, rate):
    """Default form: set list 0 at 1000 / 12000 / 24000, set list 1 at 64000.  MFCC_HIP_FUSED1024=w12 / f32: schedules 1,
    2, 0 at 7999 / 12000 / 16001.  At 37800 (no set list fits) and from 88.2 kHz (DC weight) every fused builder
    refuses: the handle must report the generic kernel and meet the fp32 model."""
    if form in ("w12", "f32"):
        monkeypatch.setenv("MFCC_HIP_FUSED1024", form)
        assert rate in rmap.F32_1024
    else:
        monkeypatch.delenv("MFCC_HIP_FUSED1024", raising=False)
        assert (rate in rmap.GENERIC_1024) == (form == "generic") and (rate in rmap.BF16_1024) == (form == "")
    for case in sc.cases_1024(form, rate):
        _run(mfcc_amd, case, wav_pcm)


# ------------------------------------------------------------------------------------------------ generic float kernel

@pytest.mark.parametrize("rate", [96000, 384000])
def test_generic_float_kernel(mfcc_amd, wav_pcm, rate):
    """impl="generic" at 256 / 20 and at 512 / 32 hop 257: DC weight and empty bands in both."""
    for case in sc.cases_generic(rate):
        assert lb.empty_bands(case.filters()).any() and (case.filters()[:, 0] != 0).any()
        _run(mfcc_amd, case, wav_pcm)


# ------------------------------------------------------------------------------------------------ fixed

FIXED = [("mfcc_fixed512_kernel", 512, 32, 13), ("mfcc_fixed512_kernel", 512, 16, 16),
         ("mfcc_fixed_kernel", 256, 16, 16), ("mfcc_fixed_kernel", 1024, 64, 32)]
STIMULI = ["noise", "square_b100h", "const_min", "loud_silent"]


@pytest.mark.parametrize("kernel,nfft,nfil,ncep", FIXED)
def test_fixed_kernels_at_every_rate(mfcc_amd, kernel, nfft, nfil, ncep):
    """Bit for bit against the RTL oracle at every rate, on four loud stimuli; where the oracle's filterbank asserts the
    library must answer UNSUPPORTED (the rule of test_fixed_fused_kernel_other_sample_rates).  The fused kernel deals
    its filterbank products out by filter width: the rates whose float bank has an empty filter must run, not be
    refused, at 512 / 32."""
    pcm = fs.stack(fs.n_samples(nfft, sc.NFR), nfft, STIMULI)
    dev = _strided(pcm)
    ran = []
    for rate in rmap.RATES:
        with mfcc_amd.MFCC(nfft=nfft, nfilters=nfil, nceptrums=ncep, samplerate=rate) as m:
            try:
                ref = mx.mfcc_fixed_ref(pcm, nfft=nfft, nfilters=nfil, nceptrums=ncep, sample_rate=float(rate),
                                        pad_mode="notebook")
            except AssertionError:
                with pytest.raises(mfcc_amd.MfccHipError) as e:
                    m.process_fixed(pcm)
                assert e.value.code == -105, rate
                continue
            assert m.kernel_name(fixed=True) == kernel, (rate, m.kernel_name(fixed=True))
            got = as_np(m.process_fixed(dev))
            assert got.shape == ref.shape == (len(STIMULI), sc.NFR, ncep) and got.dtype == np.int16
            bad = np.argwhere(got != ref)
            assert not len(bad), "%d Hz: %d value(s) differ, first at (stimulus, frame, coef) %s" % (rate, len(bad), bad[0])
            ran.append(rate)
    assert len(ran) >= 10
    if (nfft, nfil) == (512, 32):
        assert len([r for r in ran if rmap.empty_bands(512, 32, r)]) == 5        # 88.2, 96, 176.4, 192, 384 kHz all run


# ------------------------------------------------------------------------------------------------ routes

def test_the_empty_column_survives_the_ragged_and_session_routes(mfcc_amd, wav_pcm):
    """96 kHz / 32 filters, log-mel: ``process_batch`` and ``stream()`` equal the dense call bit for bit."""
    case = [c for c in sc.cases_512(96000) if c.logmel and c.kw["nfilters"] == 32][0]
    pcm = sc.pcm_of(case, wav_pcm)
    n = pcm.shape[1]
    with mfcc_amd.MFCC(**case.kw) as m:
        assert m.kernel_name() == sc.W12
        dense = as_np(m.process(_strided(pcm)))
        _check(case, dense, wav_pcm)
        assert np.isneginf(dense[:, :, 1]).all() and np.isfinite(dense[:3, :, 2:]).all()
        utts = [pcm[c][:n - 170 * 3 * c - c] for c in range(NCH)]
        for c, rows in enumerate(m.process_batch(utts)):
            assert same(rows, dense[c][:sc.NFR - 3 * c - (c > 0)]), c
        rng = np.random.default_rng(4)
        for c in (1, 3):
            with m.stream() as s:
                rows, i = [], 0
                while i < n:
                    k = int(rng.integers(1, 1500))
                    rows.append(s.push(pcm[c][i:i + k]))
                    i += k
                rows.append(s.flush())
            assert same(np.concatenate(rows), dense[c]), c
