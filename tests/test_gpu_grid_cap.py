"""More tiles than the grid of each fused float kernel: workgroups walk their tile cursor a grid stride at a time, and
the stride is no multiple of a channel's tiles, so many of those advances carry into the next channel (fused_common.hpp:
advance; the geometry is launch_geom.hpp's).  The other GPU tests run the non-default forms on inputs of a few tiles only.

One batch per form: channels of three tiles (37 frames) on an odd channel stride, about 2.5 x CUs tiles, so that for
every grid rule (a stride of 2 x CUs tiles, or of CUs for the eight-wave 1024 forms) a good part of the workgroups own
a second tile and reach it by a carried advance; the test counts those advances before it runs anything.  The batch must
equal, bit for bit, the same handle run on slices of channels small enough that no workgroup sees a second tile
(n_tiles <= CUs / 2), and six of its channels, one of them reached by a carried advance, are held to the float64
reference under the bound of the kernel's model.  The diagnostic forms are reached through the environment variables a
handle reads when it is made (tests/test_gpu_error_bound.py)."""
import numpy as np
import pytest

import framed_ref as fr
import kernel_families as kf
import melbank_ref as mr
from kernel_families import as_np, same
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu

K512 = dict(nfft=512, nfilters=32, nceptrums=13)
K1024 = dict(nfft=1024, nfilters=40, nceptrums=13, power_scale=0)
FRAMED = dict(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=13)
HTK = dict(nfft=512, hop=160, win_length=400, nfilters=40, nceptrums=13, mel="htk", fmin=20, fmax=8000)
R1024 = dict(nfft=1024, hop=341, n_mel=40, power_scale=1024.0)
RFRAMED = dict(L=400, hop=160, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0)

# id -> (MFCC arguments, environment, kernel, cursor stride in tiles per CU, samples of a frame, hop, model,
#        reference_and_bound of (channels, n) samples)
FORMS = {
    "512_w12": (K512, {}, "mfcc_fused512_w12_kernel", 2, 512, 170, "bf16x2/bf16x2",
                lambda x, model: eb.reference_and_bound(x, model, n_cep=13)),
    "512_w4": (K512, {"MFCC_HIP_FUSED512": "w4"}, "mfcc_fused512_kernel", 2, 512, 170, "bf16x2/fp32",
               lambda x, model: eb.reference_and_bound(x, model, n_cep=13)),
    "512_h160": (FRAMED, {}, "mfcc_fused512_h160_kernel", 2, 400, 160, "bf16x2/fp32",
                 lambda x, model: fr.reference_and_bound(x, model, n_cep=13, **RFRAMED)),
    "512_h160_mb": (HTK, {}, "mfcc_fused512_h160_mb_kernel", 2, 400, 160, "bf16x2/fp32",
                    lambda x, model: mr.reference_and_bound(x, model, n_cep=13, low=20.0, high=8000, **dict(RFRAMED, n_mel=40))),
    "1024_w12bf": (K1024, {}, "mfcc_fused1024_w12bf_kernel", 2, 1024, 341, "bf16x2/fp32",
                   lambda x, model: eb.reference_and_bound(x, model, n_cep=13, **R1024)),
    "1024_w12": (K1024, {"MFCC_HIP_FUSED1024": "w12"}, "mfcc_fused1024_w12_kernel", 2, 1024, 341, "fp32/fp32",
                 lambda x, model: eb.reference_and_bound(x, model, n_cep=13, **R1024)),
    "1024_f32": (K1024, {"MFCC_HIP_FUSED1024": "f32"}, "mfcc_fused1024_kernel", 1, 1024, 341, "fp32/fp32",
                 lambda x, model: eb.reference_and_bound(x, model, n_cep=13, **R1024)),
    "1024_bf16": (K1024, {"MFCC_HIP_FUSED1024": "bf16"}, "mfcc_fused1024_kernel", 1, 1024, 341, "bf16x2/fp32",
                  lambda x, model: eb.reference_and_bound(x, model, n_cep=13, **R1024)),
}


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


@pytest.mark.parametrize("form", list(FORMS))
def test_more_tiles_than_the_grid(mfcc_amd, wav_pcm, monkeypatch, form):
    import torch
    kw, env, kernel, stride_per_cu, flen, hop, model, reference = FORMS[form]
    for var in ("MFCC_HIP_FUSED512", "MFCC_HIP_FUSED1024"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    tpc = next(t for t in (3, 5, 7) if cu % t)          # tiles per channel: the grid (CUs or 2 x CUs) is no multiple of it
    frames = 16 * (tpc - 1) + 5                         # 37 frames on a device whose CU count is no multiple of 3
    nch = 5 * cu // (2 * tpc) + 1                       # about 2.5 CUs tiles: 214 channels on 256 CUs, under 3 M samples
    n_tiles = nch * tpc
    per_slice = max(1, (cu // 2) // tpc)                # channels of a slice: n_tiles <= CUs / 2
    assert n_tiles > 2 * cu and per_slice * tpc <= max(tpc, cu // 2)
    # (virtual) workgroup v starts on tile v and advances by the stride; the advance carries when t_in + grid_mod
    # reaches tiles_per_ch.  Those whose carried advance lands on a tile of the batch:
    stride = stride_per_cu * cu
    assert stride % tpc and n_tiles > stride
    carried = [v for v in range(min(stride, n_tiles - stride)) if v % tpc + stride % tpc >= tpc]
    assert len(carried) >= cu // 8, (form, len(carried))
    n = hop * (frames - 1) + flen
    ch_stride = (n | 1) + 2                             # odd, so channels start at every alignment of a 16-byte load
    pcm = np.stack([kf.signal(kf.KINDS[c % len(kf.KINDS)], n, 500 + c, wav_pcm) for c in range(nch)])
    flat = np.zeros(5 + nch * ch_stride + 16, np.int16)
    for c in range(nch):
        flat[5 + c * ch_stride: 5 + c * ch_stride + n] = pcm[c]
    view = torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (ch_stride, 1), storage_offset=5)
    with mfcc_amd.MFCC(**kw) as m:
        assert m.kernel_name() == kernel
        assert m.num_frames(n) == frames
        whole = m.process(view)
        assert tuple(whole.shape) == (nch, frames, 13)
        parts = [m.process(view[a:a + per_slice]) for a in range(0, nch, per_slice)]
        torch.cuda.synchronize()
    assert same(whole, torch.cat(parts)), "%s: the batch differs from its slices" % form
    # six channels: the first two, two with a tile that a carried advance reaches, the last two
    idx = [0, 1, (carried[0] + stride) // tpc, (carried[len(carried) // 2] + stride) // tpc, nch - 2, nch - 1]
    assert len(set(idx)) == 6, idx
    ref, bound = reference(pcm[idx], model)
    worst = eb.check(as_np(whole)[idx], ref, bound, "%s channels %s" % (form, idx))
    print("grid cap %s: %d channels, %d carried advances, worst error / bound %.3f" % (form, nch, len(carried), worst))
