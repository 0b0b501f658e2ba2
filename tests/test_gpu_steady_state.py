"""The steady state of every fused float kernel's tile loop: what a workgroup runs on every tile but its last.

A fused kernel finishes tile t (log2, DCT or log-mel store) while it transforms tile t + 1, and fetches and parks the
samples of tile t + 2 on the way: the ``have_prev`` branches inside ``while (cur.ch < g.n_ch)`` and the
fetch_window / park_window / ``shift = next_shift`` hand-over.  A launch has at most 2 x CUs workgroups (CUs for the
eight-wave 1024 forms; launch_geom.hpp), so on an input of a few dozen tiles every workgroup runs one tile and the
epilogue behind the loop, and none of that code runs.  tests/test_gpu_grid_cap.py gives a workgroup a second tile in one
configuration per form; here every form, instantiation and option of the fused kernels gets workgroups of three tiles.

One batch shape for all cases (``_batch``): channels of ``tpc`` tiles (3 unless the CU count is a multiple of 3; 37
frames, the last tile partial) on an odd channel stride behind an odd base offset, the six input kinds cycled over the
channels, about 4.5 x CUs tiles.  With a cursor stride of S tiles, (virtual) workgroup v owns tiles v, v + S, v + 2 S:
for v < n_tiles - 2 S it has a first tile, a middle tile -- a previous tile to finish and a next one to fetch -- and a
last one.  Before anything runs, a case counts the workgroups of three tiles, the advances that carry into the next
channel, and the edge-path and aligned tiles among the second and third ones.  Then

1. the handle reports the expected kernel;
2. the batch equals, bit for bit, the same handle run on slices of channels of at most CUs / 2 tiles, where no workgroup
   has a second tile: the epilogue path that the other tests pin;
3. every channel is held to the float64 reference under the kernel's declared model (oracle/error_bound.py,
   tests/framed_ref.py, tests/melbank_ref.py; the terms of tests/logmel_bound.py for log-mel rows), and the reference
   must bound every frame or pin its -inf / NaN pattern.

The diagnostic forms are reached through the environment variables a handle reads when it is made."""
import numpy as np
import pytest

import framed_ref as fr
import kernel_families as kf
import logmel_bound as lb
import melbank_ref as mr
from kernel_families import as_np, same
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu

W4, H160, MB = "mfcc_fused512_kernel", "mfcc_fused512_h160_kernel", "mfcc_fused512_h160_mb_kernel"
W12, W12BF = "mfcc_fused512_w12_kernel", "mfcc_fused1024_w12bf_kernel"
S512, S1024 = 3072, 6152                     # samples of a tile's parked span (kSUsed of the 512 and the 1024 kernels)
SEED = 7
# A constant input under the full-length periodic Hamming window has energy in bins 0 and 1 only: every other band is
# float64 roundoff of an exact zero and the model leaves the frame open.  (Under a window shorter than nfft the
# zero-padding spreads it over every bin, so the hop-160 cases keep the kind.)  The hop-170 and 1024 cases run a second
# full-scale square in its place.  A square whose period divides nfft (half periods 1, 2, 4, 8, 16) is as sparse, at its
# harmonics only: those cases draw the square of the next seed whose period does not (_square_seed).
KINDS_FULL_FRAME = ["speech", "noise", "uniform", "square", "square", "silences"]


def _square_seed(seed):
    """the first of seed, seed + 1000, ... for which kf.signal("square", ...) draws a half period that is no power of two"""
    while True:
        half = max(1, int(np.random.default_rng(seed).integers(2, 40)) // 2)
        if half & (half - 1):
            return seed
        seed += 1000


class Case:
    def __init__(self, kernel, kw, model, reference, flen, s_used, env=None, stride_per_cu=2, kinds=kf.KINDS, seed=SEED):
        self.kernel, self.kw, self.model, self.reference = kernel, kw, model, reference
        self.flen, self.hop, self.s_used = flen, kw["hop"], s_used
        self.env, self.stride_per_cu, self.kinds = env or {}, stride_per_cu, kinds
        self.pad, self.halo, self.seed = kw["pad_mode"], kw.pop("halo", 0), seed


def _plain(kernel, nfft=512, n_mel=32, n_cep=13, rate=16000, lifter=0.0, output="cepstra", pad="notebook", halo=0,
           env=None, stride_per_cu=2, model=None):
    """the 512 / 170 and 1024 / 341 forms: oracle/error_bound.py, log-mel rows by tests/logmel_bound.py"""
    hop = nfft // 3
    kw = dict(nfft=nfft, hop=hop, nfilters=n_mel, nceptrums=n_cep, samplerate=rate, lifter=lifter, output=output,
              pad_mode=pad, halo=halo, power_scale=512.0 if nfft == 512 else 0)
    nb = dict(nfft=nfft, hop=hop, n_mel=n_mel, sample_rate=rate, power_scale=float(nfft))
    model = model or eb.model_of(kernel)
    if output == "logmel":
        model = lb.MODEL[kernel]
        ref = lambda x: lb.reference_and_bound(x, model, pad_mode=pad, halo=halo, **nb)
    else:
        ref = lambda x: eb.reference_and_bound(x, model, n_cep=n_cep, pad_mode=pad, lifter=lifter, halo=halo, **nb)
    return Case(kernel, kw, model, ref, nfft, S512 if nfft == 512 else S1024, env, stride_per_cu, KINDS_FULL_FRAME)


def _w4(**kw):
    return _plain(W4, env={"MFCC_HIP_FUSED512": "w4"}, **kw)


def _framed(L=400, n_mel=32, n_cep=13, rate=16000, lifter=0.0, output="cepstra", pad="notebook", halo=0, seed=SEED):
    kw = dict(nfft=512, hop=160, win_length=L, nfilters=n_mel, nceptrums=n_cep, samplerate=rate, lifter=lifter,
              output=output, pad_mode=pad, halo=halo)
    ref = lambda x: fr.reference_and_bound(x, "bf16x2/fp32", L=L, hop=160, nfft=512, n_mel=n_mel, sample_rate=rate,
                                           power_scale=512.0, n_cep=n_cep, pad_mode=pad, halo=halo, output=output,
                                           lifter=lifter)
    return Case(H160, kw, "bf16x2/fp32", ref, L, S512, seed=seed)


def _bank(bank, n_cep=13, lifter=0.0, output="cepstra", pad="notebook", halo=0):
    n_mel, low, high, rate = bank
    kw = dict(nfft=512, hop=160, win_length=400, nfilters=n_mel, nceptrums=n_cep, samplerate=rate, lifter=lifter,
              output=output, pad_mode=pad, halo=halo, mel="htk", fmin=low, fmax=high)
    ref = lambda x: mr.reference_and_bound(x, "bf16x2/fp32", L=400, hop=160, nfft=512, n_mel=n_mel, sample_rate=rate,
                                           power_scale=512.0, n_cep=n_cep, pad_mode=pad, halo=halo, output=output,
                                           low=float(low), high=high, lifter=lifter)
    return Case(MB, kw, "bf16x2/fp32", ref, 400, S512)


HTK23, HTK40, HTK64V, HTK64 = (23, 20, 8000, 16000), (40, 20, 8000, 16000), (64, 125, 7500, 16000), (64, 0, 8000, 16000)
M21, M170 = kf.MASK_BANKS["m21_40f_telephone"][:4], kf.MASK_BANKS["m170_64f_high"][:4]

CASES = {
    # tile_loop_w4<170>: <DENSE, DCX> = <false, false>, <true, false>, <true, true> at 16, 8 and 48 kHz
    "w4_16k": _w4(), "w4_8k": _w4(rate=8000), "w4_48k": _w4(rate=48000),
    "w4_32c_lifter": _w4(n_cep=32, lifter=22.0), "w4_44k_17c": _w4(rate=44100, n_cep=17),
    "w4_16f": _w4(n_mel=16, n_cep=16),
    # mfcc_fused512_h160_kernel: its six <DENSE, DCX, LOGMEL>
    # (48 kHz: band 0 is the DC bin alone, and with seed 7 one frame of one `uniform` channel of the 385 on 256 CUs has
    # it at 4e-7 of the frame's rms, under its own error bound; seed 8 leaves no frame open)
    "h160_16k": _framed(), "h160_8k": _framed(rate=8000), "h160_48k": _framed(rate=48000, seed=8),
    "h160_16k_logmel": _framed(output="logmel"), "h160_8k_logmel": _framed(rate=8000, output="logmel"),
    "h160_48k_logmel": _framed(rate=48000, output="logmel", seed=8),
    "h160_32c_lifter": _framed(n_cep=32, lifter=22.0),
    "h160_16f": _framed(n_mel=16), "h160_16f_logmel": _framed(n_mel=16, output="logmel"),
    "h160_L511_stream_halo": _framed(L=511, pad="stream", halo=1), "h160_L160": _framed(L=160),
    # mfcc_fused512_h160_mb_kernel: both <LOGMEL>, two to four blocks, one K group only
    "mb_htk23": _bank(HTK23), "mb_htk40": _bank(HTK40), "mb_htk64_vggish": _bank(HTK64V),
    "mb_mask21": _bank(M21), "mb_mask170": _bank(M170),
    "mb_htk23_logmel": _bank(HTK23, output="logmel"), "mb_htk40_logmel": _bank(HTK40, output="logmel"),
    "mb_htk64_vggish_logmel": _bank(HTK64V, output="logmel"),
    "mb_mask21_logmel": _bank(M21, output="logmel"), "mb_mask170_logmel": _bank(M170, output="logmel"),
    "mb_htk64_16c_lifter": _bank(HTK64, n_cep=16, lifter=22.0),
    "mb_htk40_stream_halo": _bank(HTK40, pad="stream", halo=1),
    # mfcc_fused512_w12_kernel
    "w12_16k": _plain(W12), "w12_8k": _plain(W12, rate=8000), "w12_48k": _plain(W12, rate=48000),
    "w12_32c_lifter": _plain(W12, n_cep=32, lifter=22.0), "w12_16f": _plain(W12, n_mel=16, n_cep=16),
    "w12_16k_logmel": _plain(W12, output="logmel"), "w12_48k_logmel": _plain(W12, rate=48000, output="logmel"),
    "w12_stream_halo": _plain(W12, pad="stream", halo=1),
    # mfcc_fused1024_w12bf_kernel
    "1024_16k": _plain(W12BF, 1024, 40), "1024_44k": _plain(W12BF, 1024, 40, rate=44100),
    "1024_48k": _plain(W12BF, 1024, 40, rate=48000), "1024_40c": _plain(W12BF, 1024, 40, n_cep=40),
    "1024_32c_lifter": _plain(W12BF, 1024, 40, n_cep=32, lifter=22.0),
    "1024_logmel": _plain(W12BF, 1024, 40, output="logmel"),
    "1024_stream_halo": _plain(W12BF, 1024, 40, pad="stream", halo=1),
    # the other 1024 forms; the eight-wave ones stride by CUs, so their workgroups see four or five tiles
    "1024_w12_40c": _plain("mfcc_fused1024_w12_kernel", 1024, 40, n_cep=40, env={"MFCC_HIP_FUSED1024": "w12"}),
    "1024_f32_40c": _plain("mfcc_fused1024_kernel", 1024, 40, n_cep=40, env={"MFCC_HIP_FUSED1024": "f32"},
                           stride_per_cu=1, model="fp32/fp32"),
    "1024_bf16_40c": _plain("mfcc_fused1024_kernel", 1024, 40, n_cep=40, env={"MFCC_HIP_FUSED1024": "bf16"},
                            stride_per_cu=1, model="bf16x2/fp32"),
    # the four forms at 32 kHz: Sets<2>, whose five sets change the waits and the register pressure of the bf16 forms,
    # and the fp32 list with the most MFMAs
    "1024_32k_40c": _plain(W12BF, 1024, 40, rate=32000, n_cep=40),
    "1024_w12_32k_40c": _plain("mfcc_fused1024_w12_kernel", 1024, 40, rate=32000, n_cep=40,
                               env={"MFCC_HIP_FUSED1024": "w12"}),
    "1024_f32_32k_40c": _plain("mfcc_fused1024_kernel", 1024, 40, rate=32000, n_cep=40,
                               env={"MFCC_HIP_FUSED1024": "f32"}, stride_per_cu=1, model="fp32/fp32"),
    "1024_bf16_32k_40c": _plain("mfcc_fused1024_kernel", 1024, 40, rate=32000, n_cep=40,
                                env={"MFCC_HIP_FUSED1024": "bf16"}, stride_per_cu=1, model="bf16x2/fp32"),
}


def _batch(case, cu):
    """The geometry of a case's batch on ``cu`` compute units, asserted to reach the steady state, as a dict."""
    tpc = next(t for t in (3, 5, 7) if cu % t)          # tiles per channel: the stride (CUs or 2 x CUs) is no multiple of it
    frames = 16 * (tpc - 1) + 5                         # 37 frames on a device whose CU count is no multiple of 3
    nch = 9 * cu // (2 * tpc) + 1                       # about 4.5 CUs tiles: 385 channels on 256 CUs, under 6 M samples
    n_tiles = nch * tpc
    stride = case.stride_per_cu * cu                    # of the cursor, in tiles: every workgroup is in flight
    assert stride % tpc and n_tiles > 2 * stride
    # samples that give ``frames`` frames (tests/test_gpu_framed.py: _length), and the halo sample in front of them
    n = case.hop * (frames - 1) + case.flen if case.pad == "notebook" else \
        case.hop * (frames - 2) + case.flen + case.hop // 2
    # (virtual) workgroup v starts on tile v and advances by the stride.  Three tiles or more:
    three = list(range(min(stride, n_tiles - 2 * stride)))
    assert len(three) >= cu // 8, len(three)
    # second and later tiles, and those reached by an advance that carries (fused_common.hpp: t_in + grid_mod reaches
    # tiles_per_ch), as tests/test_gpu_grid_cap.py counts them
    later = list(range(stride, n_tiles))
    carried = [t for t in later if (t - stride) % tpc + stride % tpc >= tpc]
    assert len(carried) >= cu // 8, len(carried)
    # launch_geom.hpp: tiles t_lo <= t_in <= t_hi load their span with aligned 16-byte loads, every other one goes
    # sample by sample
    tile_hop = 16 * case.hop
    t_lo = max(0, (9 - case.halo + tile_hop - 1) // tile_hop)
    t_hi = -1 if n < case.s_used else min((n - case.s_used) // tile_hop, tpc)
    edge = [t for t in later if not t_lo <= t % tpc <= t_hi]
    assert edge and len(edge) < len(later), (t_lo, t_hi)
    per_slice = max(1, (cu // 2) // tpc)                # channels of a slice: n_tiles <= CUs / 2
    assert per_slice * tpc <= max(tpc, cu // 2)
    # channels that must be among the checked ones: the first and the last, one of each kind, and those holding the middle
    # and the last tile of the first, a middle and the last three-tile workgroup.  (All channels are checked.)
    named = set(range(len(case.kinds))) | {nch - 1}
    for v in (three[0], three[len(three) // 2], three[-1]):
        named |= {(v + stride) // tpc, (v + 2 * stride) // tpc}
    assert len(named) >= 12 and max(named) < nch, sorted(named)
    return dict(tpc=tpc, frames=frames, nch=nch, n=n, stride=stride, three=len(three), carried=len(carried),
                edge=len(edge), later=len(later), per_slice=per_slice, named=sorted(named))


_PCM = {}


def _pcm(case, b, wav_pcm):
    """(channels, n + halo) int16, the kinds cycled over the channels; shared by the cases of one length, left unchanged"""
    n = b["n"] + case.halo
    key = (n, b["nch"], tuple(case.kinds), case.seed)
    if key not in _PCM:
        def seed(c, kind):
            return _square_seed(case.seed + c) if kind == "square" and case.kinds is KINDS_FULL_FRAME else case.seed + c
        kinds = [case.kinds[c % len(case.kinds)] for c in range(b["nch"])]
        x = np.stack([kf.signal(k, n, seed(c, k), wav_pcm) for c, k in enumerate(kinds)])
        x.setflags(write=False)
        _PCM[key] = x
    return _PCM[key]


def _reference(case, pcm):
    """reference and bound of every channel; every frame bounded, or an all-zero frame with its pattern pinned"""
    ref, bound = case.reference(pcm)
    assert not np.isposinf(bound).any(), "the reference leaves %d frame(s) unbounded" % np.isposinf(bound).any(axis=2).sum()
    return ref, bound


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def test_the_matrix_holds_every_instantiation_of_the_four_wave_loop():
    """<DENSE, DCX> by sample rate (tests/test_gpu_fused512_w4_forms.py): three of mfcc_fused512_kernel, times LOGMEL
    six of mfcc_fused512_h160_kernel, and the two <LOGMEL> of mfcc_fused512_h160_mb_kernel."""
    def forms(kernel):
        return {(c.kw["samplerate"], c.kw["output"]) for c in CASES.values()
                if c.kernel == kernel and c.kw["nfilters"] == 32 and not c.kw["lifter"]}
    rates = (16000, 8000, 48000)
    assert forms(W4) >= {(r, "cepstra") for r in rates}
    assert forms(H160) >= {(r, o) for r in rates for o in ("cepstra", "logmel")}
    assert {c.kw["output"] for c in CASES.values() if c.kernel == MB} == {"cepstra", "logmel"}


@pytest.mark.parametrize("name", list(CASES))
def test_steady_state(mfcc_amd, wav_pcm, monkeypatch, name):
    import torch
    case = CASES[name]
    for var in ("MFCC_HIP_FUSED512", "MFCC_HIP_FUSED1024"):
        monkeypatch.delenv(var, raising=False)
    for var, value in case.env.items():
        monkeypatch.setenv(var, value)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    b = _batch(case, cu)
    nch, halo = b["nch"], case.halo
    pcm = _pcm(case, b, wav_pcm)
    n = pcm.shape[1]                                    # with the halo sample
    ch_stride = (n | 1) + 2                             # odd, so channels start at every alignment of a 16-byte load
    flat = np.zeros(5 + nch * ch_stride + 16, np.int16)
    for c in range(nch):
        flat[5 + c * ch_stride: 5 + c * ch_stride + n] = pcm[c]
    view = torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (ch_stride, 1), storage_offset=5)
    with mfcc_amd.MFCC(**case.kw) as m:
        assert m.kernel_name() == case.kernel
        assert m.num_frames(n - halo) == b["frames"]
        whole = m.process(view, halo=halo)
        assert tuple(whole.shape) == (nch, b["frames"], m.num_features)
        parts = [m.process(view[a:a + b["per_slice"]], halo=halo) for a in range(0, nch, b["per_slice"])]
        torch.cuda.synchronize()
    assert same(whole, torch.cat(parts)), "%s: the batch differs from its slices" % name
    ref, bound = _reference(case, pcm)
    worst = eb.check(as_np(whole), ref, bound, name)
    print("steady state %s: %s, %d channels, %d three-tile workgroups, %d carried advances, %d of %d later tiles on the "
          "edge path, worst error / bound %.3f" % (name, case.kernel, nch, b["three"], b["carried"], b["edge"],
                                                   b["later"], worst))
