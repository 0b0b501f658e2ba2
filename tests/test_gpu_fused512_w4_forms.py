"""Every instantiation of the four-wave tile loop, by name, in one place: the three of mfcc_fused512_kernel, the six of
mfcc_fused512_h160_kernel (both tile_loop_w4 of kernel_fused512.hpp) and the two of mfcc_fused512_h160_mb_kernel (its
own copy of that loop), so a change made to one copy and not to the other shows here.

Shape: 2 channels of 37 frames at an odd channel stride -- three 16-frame tiles per channel, the last one partial.  The
six tiles go to six workgroups: each runs one tile (an edge-path one, an aligned one, a partial one) and the epilogue
behind the loop.  The steady state of the loop -- a previous tile to finish, a next one to fetch -- needs more tiles than
the launch has workgroups: tests/test_gpu_steady_state.py runs every instantiation listed here that way.

Sample rates (mfcc_fused::needs_dc_exact and the banded test of mfcc_fused::build_tables):
  16000  the banded set list                                    <DENSE, DCX> = <false, false>
   8000  the dense list, no filter on bin 0                                    <true, false>
  48000  the dense list and the double-precision DC bin                        <true, true>

Nothing here is new arithmetic: every value is held to oracle/error_bound.py under the kernels' model (bf16 x 2-split
mel, fp32 DCT), through tests/framed_ref.py and tests/melbank_ref.py for the framed and the HTK handles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import framed_ref as fr
import kernel_families as kf
import melbank_ref as mr
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = "bf16x2/fp32"
RATES = [16000, 8000, 48000]
NCH, NFR = 2, 37


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _flat(pcm):
    """``pcm`` (channels, n) laid out at an odd channel stride behind an odd base offset: (flat, stride, offset)"""
    nch, n = pcm.shape
    off, stride = 3, n + 5 + n % 2
    assert stride % 2 == 1
    flat = np.zeros(off + stride * nch + 16, np.int16)
    for c in range(nch):
        flat[off + c * stride: off + c * stride + n] = pcm[c]
    return flat, stride, off


def _view(flat, n, stride, off):
    import torch
    return torch.as_strided(torch.from_numpy(flat).cuda(), (NCH, n), (stride, 1), storage_offset=off)


def _check(check, got, refs, what):
    got = kf.as_np(got)
    assert got.shape == (NCH,) + refs[0][0].shape, what
    worst = 0.0
    for c, (ref, bound) in enumerate(refs):
        assert not np.isposinf(bound).any(), "%s channel %d: the reference leaves frames unbounded" % (what, c)
        worst = max(worst, check(got[c], ref, bound, "%s channel %d" % (what, c)))
    print("%s: worst error / bound %.3f" % (what, worst))


def test_hop_170_kernel_three_instantiations(mfcc_amd, wav_pcm, tmp_path):
    """MFCC_HIP_FUSED512=w4 is read when a handle is made: a child process, as tests/test_gpu_error_bound.py does."""
    n = 170 * (NFR - 1) + 512
    pcm = kf.channels(n, 5, wav_pcm, kinds=["speech", "noise"])
    flat, stride, off = _flat(pcm)
    np.save(tmp_path / "in.npy", flat)
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); import mfcc_amd\n"
            "flat = torch.from_numpy(np.load(%r)).cuda()\n"
            "x = torch.as_strided(flat, (%d, %d), (%d, 1), storage_offset=%d)\n"
            "for sr in %r:\n"
            "    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, samplerate=sr) as m:\n"
            "        assert m.kernel_name() == 'mfcc_fused512_kernel', m.kernel_name()\n"
            "        np.save(%r %% sr, m.process(x).cpu().numpy())\n"
            % (ROOT, str(tmp_path / "in.npy"), NCH, n, stride, off, RATES, str(tmp_path / "out%d.npy")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MFCC_HIP_FUSED512="w4"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for sr in RATES:
        refs = [eb.reference_and_bound(pcm[c], MODEL, n_cep=13, sample_rate=sr) for c in range(NCH)]
        _check(eb.check, np.load(tmp_path / ("out%d.npy" % sr)), refs, "w4 hop 170 at %d Hz" % sr)


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
@pytest.mark.parametrize("sr", RATES)
def test_framed_kernel_six_instantiations(mfcc_amd, wav_pcm, sr, output):
    n = 160 * (NFR - 1) + 400
    pcm = kf.channels(n, 6, wav_pcm, kinds=["speech", "noise"])
    flat, stride, off = _flat(pcm)
    with mfcc_amd.MFCC(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=13, samplerate=sr, output=output) as m:
        assert m.kernel_name() == "mfcc_fused512_h160_kernel"
        got = m.process(_view(flat, n, stride, off))
    refs = [fr.reference_and_bound(pcm[c], MODEL, L=400, hop=160, nfft=512, n_mel=32, sample_rate=sr, power_scale=512.0,
                                   n_cep=13, output=output) for c in range(NCH)]
    _check(fr.check, got, refs, "framed 400/160 at %d Hz, %s" % (sr, output))


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
def test_bank_kernel_two_instantiations(mfcc_amd, wav_pcm, output):
    n = 160 * (NFR - 1) + 400
    pcm = kf.channels(n, 7, wav_pcm, kinds=["speech", "noise"])
    flat, stride, off = _flat(pcm)
    with mfcc_amd.MFCC(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13, mel="htk", fmin=20, fmax=8000,
                       output=output) as m:
        assert m.kernel_name() == "mfcc_fused512_h160_mb_kernel"
        got = m.process(_view(flat, n, stride, off))
    refs = [mr.reference_and_bound(pcm[c], MODEL, L=400, hop=160, nfft=512, n_mel=40, sample_rate=16000, power_scale=512.0,
                                   n_cep=13, output=output, low=20.0, high=8000) for c in range(NCH)]
    _check(mr.check, got, refs, "HTK 40, %s" % output)
