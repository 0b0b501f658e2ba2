"""Every float kernel against the per-coefficient error bound of its declared arithmetic (oracle/error_bound.py).

The global measure of the float contract (max|d| / max|ref| <= 1e-4, tests/test_gpu_parity.py) lets each
coefficient of each frame drift by ~5e-3: a kernel wrong in one frame per 16-frame tile passes it.  Here every
coefficient of every frame is held to its own bound, carried from the float64 oracle's stages through the
kernel's declared model (fp32 or bf16 x 2-split mel / DCT), and frames with a silent band to the oracle's exact
-inf / NaN pattern.  Inputs: speech, noise at three levels, full-scale noise, clipped square, sine, DC with dither,
noise with silent stretches.  Shapes: frame counts at every tile residue that matters, odd channel strides and base
offsets, a history halo, stream padding, every n_cep band of both fused kernels, a lifter, the 16-filter constructor
default, every sample rate, the generic kernel at each FFT size, and a whole one-hour config-4 channel (the whole
config-2 stream is checked in tests/test_gpu_parity.py::test_float_linearity_property_full_size)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import error_bound as eb
from oracle import mfcc_float as mf

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ["wav", "noise3000", "noise30", "uniform", "square", "sine", "dc_dither", "silences"]
RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def signal(kind, n, seed, wav_pcm):
    """The input kinds of tests/test_error_bound.py (the soundness set of the instrument)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "wav":
        return np.resize(wav_pcm[seed % 5000:], n).astype(np.int16)
    if kind == "noise3000":
        x = rng.standard_normal(n) * 3000
    elif kind == "noise30":
        x = rng.standard_normal(n) * 30
    elif kind == "uniform":
        x = rng.integers(-32768, 32768, n).astype(np.float64)
    elif kind == "square":
        x = 40000 * np.sign(np.sin(t * rng.uniform(0.01, 0.3)))
    elif kind == "sine":
        x = 20000 * np.sin(t * rng.uniform(0.01, 3.0))
    elif kind == "dc_dither":
        x = rng.integers(-20000, 20000) + rng.integers(-1, 2, n).astype(np.float64)
    elif kind == "silences":
        x = rng.standard_normal(n) * 3000
        for a in rng.integers(0, max(n - 3000, 1), 2):
            x[a:a + int(rng.integers(300, 3000))] = 0
    else:
        raise ValueError(kind)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def all_kinds(n, seed, wav_pcm):
    return np.stack([signal(k, n, seed + i, wav_pcm) for i, k in enumerate(KINDS)])


def strided(flat_np, nch, n, stride, off):
    """(nch, n) view of a device copy of ``flat_np`` at channel stride ``stride`` and base offset ``off``."""
    import torch
    assert off + stride * (nch - 1) + n <= flat_np.size
    return torch.as_strided(torch.from_numpy(flat_np).cuda(), (nch, n), (stride, 1), storage_offset=off)


def check_channels(got, pcm, model, what, halo=0, **kw):
    """check() per channel (channel index in the message); returns the worst ratio."""
    worst = 0.0
    for c in range(len(pcm)):
        ref, bound = eb.reference_and_bound(pcm[c], model, halo=halo, **kw)
        worst = max(worst, eb.check(got[c], ref, bound, "%s channel %d" % (what, c)))
    return worst


def report(name, worst):
    print("error-bound %s: worst ratio %.3f" % (name, worst))


# ----------------------------------------------------------------------------- fused 512 (twelve-wave form)

@pytest.mark.parametrize("sr", RATES)
def test_fused512_every_input_kind_and_rate(mfcc_amd, wav_pcm, sr):
    pcm = all_kinds(170 * (16 * 12 + 14) + 512, 10 + sr % 97, wav_pcm)          # 207 frames: 12 tiles + 15
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=32, samplerate=sr) as m:
        assert m.kernel_name() == "mfcc_fused512_w12_kernel"
        got = m.process(pcm)
    report("w12 sr %d" % sr, check_channels(got, pcm, "bf16x2/bf16x2", "w12 sr %d" % sr, n_cep=32, sample_rate=sr))


@pytest.mark.parametrize("extra", [0, 1, 15, 16 * 9 + 7])
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("pad", ["notebook", "stream"])
def test_fused512_tile_residues_strides_halo_and_padding(mfcc_amd, wav_pcm, extra, halo, pad):
    """Frame counts 0, 1, 15 (mod 16) and a ragged tile count; channels at odd strides from every base residue."""
    nfr = 16 * 6 + extra
    n = 170 * (nfr - 1) + 512 + (60 if pad == "stream" else 0)
    nch = len(KINDS)
    pcm = all_kinds(n + halo, 300 + extra, wav_pcm)
    worst = 0.0
    for off in (0, 3, 5):
        stride = n + halo + 2 * off + 1
        flat = np.zeros(off + stride * nch + 16, np.int16)
        for c in range(nch):
            flat[off + c * stride: off + c * stride + n + halo] = pcm[c]
        view = strided(flat, nch, n + halo, stride, off)
        with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode=pad) as m:
            assert m.kernel_name() == "mfcc_fused512_w12_kernel"
            got = m.process(view, halo=halo).cpu().numpy()
        if pad == "notebook":
            assert got.shape[1] == nfr
        worst = max(worst, check_channels(got, pcm, "bf16x2/bf16x2", "w12 nfr %d halo %d %s off %d" % (nfr, halo, pad, off),
                                          halo=halo, n_cep=13, pad_mode=pad))
    report("w12 nfr %d halo %d %s" % (nfr, halo, pad), worst)


@pytest.mark.parametrize("ncep", [1, 13, 16, 17, 32])
def test_fused512_ncep_bands_and_lifter(mfcc_amd, wav_pcm, ncep):
    pcm = all_kinds(170 * (16 * 8 + 15) + 512 + 99, 40 + ncep, wav_pcm)
    for lifter in ((0.0, 22.0) if ncep in (13, 32) else (0.0,)):
        with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=ncep, pad_mode="stream", lifter=lifter) as m:
            assert m.kernel_name() == "mfcc_fused512_w12_kernel"
            got = m.process(pcm)
        report("w12 ncep %d lifter %g" % (ncep, lifter),
               check_channels(got, pcm, "bf16x2/bf16x2", "w12 ncep %d lifter %g" % (ncep, lifter), n_cep=ncep,
                              pad_mode="stream", lifter=lifter))


@pytest.mark.parametrize("ncep", [16, 5])
def test_fused512_constructor_default_of_16_filters(mfcc_amd, wav_pcm, ncep):
    pcm = all_kinds(170 * (16 * 5 + 1) + 512, 60 + ncep, wav_pcm)
    with mfcc_amd.MFCC(nceptrums=ncep) as m:
        assert m.nfilters == 16 and m.kernel_name() == "mfcc_fused512_w12_kernel"
        got = m.process(pcm)
    report("w12 16 filters ncep %d" % ncep,
           check_channels(got, pcm, "bf16x2/bf16x2", "w12 16 filters", n_cep=ncep, n_mel=16))


def test_fused512_four_wave_form(mfcc_amd, wav_pcm, tmp_path):
    """MFCC_HIP_FUSED512=w4 (read when a handle is made) in a child process: the four-wave form, bf16 x 2 mel and fp32
    DCT, on every input kind, at 16 kHz with 32 and 16 filters and at 44.1 / 48 kHz."""
    pcm = all_kinds(170 * (16 * 7 + 15) + 512 + 33, 77, wav_pcm)
    np.save(tmp_path / "in.npy", pcm)
    cases = [dict(nfilters=32, nceptrums=32, samplerate=16000), dict(nfilters=16, nceptrums=16, samplerate=16000),
             dict(nfilters=32, nceptrums=17, samplerate=44100), dict(nfilters=32, nceptrums=13, samplerate=48000)]
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import mfcc_amd\n"
            "x = np.load(%r)\n"
            "for i, kw in enumerate(%r):\n"
            "    with mfcc_amd.MFCC(nfft=512, pad_mode='stream', **kw) as m:\n"
            "        assert m.kernel_name() == 'mfcc_fused512_kernel', m.kernel_name()\n"
            "        np.save(%r %% i, m.process(x))\n"
            % (ROOT, str(tmp_path / "in.npy"), cases, str(tmp_path / "out%d.npy")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MFCC_HIP_FUSED512="w4"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for i, kw in enumerate(cases):
        got = np.load(tmp_path / ("out%d.npy" % i))
        what = "w4 %s" % kw
        report(what, check_channels(got, pcm, "bf16x2/fp32", what, n_cep=kw["nceptrums"], n_mel=kw["nfilters"],
                                    sample_rate=kw["samplerate"], pad_mode="stream"))


# ----------------------------------------------------------------------------- fused 1024

K1 = dict(nfft=1024, hop=341, n_mel=40, power_scale=1024.0)


@pytest.mark.parametrize("form,name,model", [(None, "mfcc_fused1024_w12bf_kernel", "bf16x2/fp32"),
                                             ("w12", "mfcc_fused1024_w12_kernel", "fp32/fp32"),
                                             ("f32", "mfcc_fused1024_kernel", "fp32/fp32"),
                                             ("bf16", "mfcc_fused1024_kernel", "bf16x2/fp32")])
def test_fused1024_every_form_and_input_kind(mfcc_amd, wav_pcm, monkeypatch, form, name, model):
    if form:
        monkeypatch.setenv("MFCC_HIP_FUSED1024", form)
    else:
        monkeypatch.delenv("MFCC_HIP_FUSED1024", raising=False)
    assert eb.model_of(name, form) == model
    pcm = all_kinds(341 * (16 * 9 + 15) + 1024 + 77, 90, wav_pcm)
    for ncep in (13, 40):
        with mfcc_amd.MFCC(nfft=1024, nfilters=40, nceptrums=ncep, power_scale=0) as m:
            assert m.kernel_name() == name and m.hop == 341
            got = m.process(pcm)
        report("1024 %s ncep %d" % (form or "default", ncep),
               check_channels(got, pcm, model, "1024 %s ncep %d" % (form, ncep), n_cep=ncep, **K1))


@pytest.mark.parametrize("sr", RATES)
def test_fused1024_every_rate(mfcc_amd, wav_pcm, sr):
    pcm = all_kinds(341 * (16 * 4 + 1) + 1024, 120 + sr % 89, wav_pcm)
    with mfcc_amd.MFCC(nfft=1024, nfilters=40, nceptrums=32, samplerate=sr, power_scale=0) as m:
        assert m.kernel_name() == "mfcc_fused1024_w12bf_kernel", sr
        got = m.process(pcm)
    report("1024 sr %d" % sr, check_channels(got, pcm, "bf16x2/fp32", "1024 sr %d" % sr, n_cep=32,
                                             **dict(K1, sample_rate=sr)))


@pytest.mark.parametrize("extra,halo,pad", [(0, 1, "notebook"), (1, 0, "stream"), (15, 1, "stream"), (16 * 3 + 9, 0, "notebook")])
@pytest.mark.parametrize("ncep,lifter", [(13, 0.0), (17, 0.0), (32, 22.0), (40, 0.0)])
def test_fused1024_tile_residues_strides_halo_ncep_lifter(mfcc_amd, wav_pcm, extra, halo, pad, ncep, lifter):
    nfr = 16 * 5 + extra
    n = 341 * (nfr - 1) + 1024 + (200 if pad == "stream" else 0)
    nch = len(KINDS)
    pcm = all_kinds(n + halo, 400 + extra + ncep, wav_pcm)
    off = 1 + ncep % 7
    stride = n + halo + 2 * off + 3
    flat = np.zeros(off + stride * nch + 16, np.int16)
    for c in range(nch):
        flat[off + c * stride: off + c * stride + n + halo] = pcm[c]
    view = strided(flat, nch, n + halo, stride, off)
    with mfcc_amd.MFCC(nfft=1024, nfilters=40, nceptrums=ncep, power_scale=0, pad_mode=pad, lifter=lifter) as m:
        assert m.kernel_name() == "mfcc_fused1024_w12bf_kernel"
        got = m.process(view, halo=halo).cpu().numpy()
    what = "1024 nfr %d halo %d %s ncep %d lifter %g" % (nfr, halo, pad, ncep, lifter)
    report(what, check_channels(got, pcm, "bf16x2/fp32", what, halo=halo, n_cep=ncep, pad_mode=pad, lifter=lifter, **K1))


# ----------------------------------------------------------------------------- generic

@pytest.mark.parametrize("nfft,nmel,ncep", [(64, 8, 8), (128, 16, 13), (256, 32, 13), (512, 32, 32), (1024, 40, 17)])
def test_generic_kernel_at_every_fft_size(mfcc_amd, wav_pcm, nfft, nmel, ncep):
    hop = nfft // 3
    pcm = all_kinds(hop * (16 * 6 + 15) + nfft + 11, nfft, wav_pcm)
    for sr in (16000, 48000):
        with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=ncep, samplerate=sr, power_scale=float(nfft),
                           pad_mode="stream", impl="generic") as m:
            assert m.kernel_name() == "mfcc_float_generic_kernel"
            got = m.process(pcm)
        what = "generic %d/%d sr %d" % (nfft, nmel, sr)
        report(what, check_channels(got, pcm, "fp32/fp32", what, n_cep=ncep, nfft=nfft, hop=hop, n_mel=nmel,
                                    sample_rate=sr, power_scale=float(nfft), pad_mode="stream"))


# ----------------------------------------------------------------------------- whole streams

def test_fused1024_whole_one_hour_channel(mfcc_amd):
    """One whole one-hour channel (168 912 frames) on the config-4 kernel, next to three other channels."""
    import torch
    n = 16000 * 3600
    x = mf.synth_pcm(n, seed=4)
    xs = torch.from_numpy(np.stack([x[::-1].copy(), x, x // 3, x])).cuda()
    with mfcc_amd.MFCC(nfft=1024, nfilters=40, nceptrums=13, power_scale=0) as m:
        assert m.kernel_name() == "mfcc_fused1024_w12bf_kernel"
        out = m.process(xs)
        got = out[1].cpu().numpy()
        assert torch.equal(out[1], out[3])
    del xs, out
    assert got.shape == (168912, 13)
    report("1024 one hour", eb.check_stream(got, x, "bf16x2/fp32", n_cep=13, chunk=12000, what="1024 one hour", **K1))
