"""The twelve-wave 512 kernel after its non-FFT instruction diet, at the smallest shapes where each changed
piece can go wrong: the conversion-free pre-emphasis of the parkers, the CEP16 tail (no second M tile, coefficient masks
computed once, the Q slots summed and the log-mel values split on register pairs) and column 16's fixed addresses.

Every case is held to the float64 oracle through the per-coefficient bound of oracle/error_bound.py (log-mel:
tests/logmel_bound.py) and to the generic kernel on the device with the measure and tolerance of
tests/test_gpu_parity.py's fused-against-generic tests (max|d| / max|ref| and rel-L2 <= 2e-5).  The generic comparison
runs over the frames the oracle's model constrains (finite bound): where a band's energy is roundoff of an exact zero, two
correct fp32 kernels differ by tens of log2 units and neither is wrong (oracle/error_bound.py's docstring).
"""
import numpy as np
import pytest

import logmel_bound as lb
from oracle import error_bound as eb

pytestmark = pytest.mark.gpu

W12 = "mfcc_fused512_w12_kernel"
MODEL = "bf16x2/bf16x2"
GENERIC_TOL = 2e-5                       # tests/test_gpu_parity.py::test_fused_kernel_alignment_shifts_and_edges
FRAME_COUNTS = [1, 15, 16, 17, 33]       # below / at / above one tile; 33: an inside tile between two edge tiles
NCH = 3


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def n_samples(nfr):
    return 170 * (nfr - 1) + 512


def noise(nch, n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(nch, n)).astype(np.int16)


def strided(pcm, base_off, halo=0):
    """Device view of ``pcm`` (channels, n) at a channel stride of 3 (mod 8) samples from ``base_off``."""
    import torch
    nch, n = pcm.shape
    stride = (n + 7) // 8 * 8 + 3
    flat = np.full(base_off + stride * nch + 64, 1234, np.int16)
    for c in range(nch):
        flat[base_off + c * stride: base_off + c * stride + n] = pcm[c]
    dev = torch.from_numpy(flat).cuda()
    return torch.as_strided(dev, (nch, n), (stride, 1), storage_offset=base_off)


def against_generic(a, b, bound, what):
    """max|d| / max|ref| and rel-L2 over the frames the model constrains, generic kernel as reference."""
    keep = np.isfinite(bound).all(axis=-1)
    if not keep.any():
        return 0.0
    a = np.asarray(a, np.float64)[keep]
    b = np.asarray(b, np.float64)[keep]
    assert np.isfinite(a).all() and np.isfinite(b).all(), what
    e_max = np.abs(a - b).max() / np.abs(b).max()
    e_l2 = np.linalg.norm(a - b) / np.linalg.norm(b)
    print("w12-diet %s: vs generic e_max %.3g e_l2 %.3g" % (what, e_max, e_l2))
    assert e_max <= GENERIC_TOL and e_l2 <= GENERIC_TOL, (what, e_max, e_l2)
    return e_max


def run_pair(mfcc_amd, view, halo, kernel=W12, **kw):
    with mfcc_amd.MFCC(nfft=512, **kw) as mfu, mfcc_amd.MFCC(nfft=512, impl="generic", **kw) as mge:
        assert mfu.kernel_name() == kernel, mfu.kernel_name()
        assert mge.kernel_name().endswith("generic_kernel")
        a = mfu.process(view, halo=halo).cpu().numpy()
        b = mge.process(view, halo=halo).cpu().numpy()
    assert a.shape == b.shape
    return a, b


def check_cepstra(a, b, pcm, what, halo=0, n_cep=13, **okw):
    worst = 0.0
    bounds = []
    for c in range(len(pcm)):
        ref, bound = eb.reference_and_bound(pcm[c], MODEL, n_cep=n_cep, halo=halo, **okw)
        worst = max(worst, eb.check(a[c], ref, bound, "%s channel %d" % (what, c)))
        bounds.append(bound)
    print("w12-diet %s: worst oracle ratio %.3f" % (what, worst))
    against_generic(a, b, np.stack(bounds), what)


# ----------------------------------------------------------------------------- frame counts, shifts, edges

@pytest.mark.parametrize("nfr", FRAME_COUNTS)
def test_frame_counts_shifts_and_edge_tiles(mfcc_amd, nfr):
    """Three channels at a stride of 3 (mod 8) samples from base offsets 0, 1, 2: every alignment shift 0..7 of the window
    fetch occurs; 33 frames have an inside tile (the parkers' 16-byte loads and predecessor dwords, lane 0 and the wave
    boundary at lane 64) between a first tile whose predecessor is the history sample 0 and a zero-padded last one."""
    n = n_samples(nfr)
    seen = set()
    for base_off in (0, 1, 2):
        pcm = noise(NCH, n, 100 * nfr + base_off)
        view = strided(pcm, base_off)
        seen |= {((view.data_ptr() // 2 + c * view.stride(0) + 2720) % 8) for c in range(NCH)}
        a, b = run_pair(mfcc_amd, view, 0, nfilters=32, nceptrums=13)
        assert a.shape == (NCH, nfr, 13)
        check_cepstra(a, b, pcm, "nfr %d off %d" % (nfr, base_off))
    assert seen == set(range(8)), seen


def test_history_halo_at_the_channel_start(mfcc_amd):
    """halo = 1: the first frame's predecessor is a real sample in front of the channel, not 0."""
    pcm = noise(NCH, n_samples(33) + 1, 7)
    view = strided(pcm, 3)
    a, b = run_pair(mfcc_amd, view, 1, nfilters=32, nceptrums=13)
    assert a.shape == (NCH, 33, 13)
    check_cepstra(a, b, pcm, "halo", halo=1)


# ----------------------------------------------------------------------------- n_cep: both tail forms, nothing written outside

@pytest.mark.parametrize("ncep", [1, 4, 13, 16, 17, 32])
def test_ncep_on_both_tail_forms_writes_only_its_rows(mfcc_amd, ncep):
    """n_cep <= 16 runs the tail without the second M tile, 17 and 32 the tail with it.  17 frames: a full tile and a tile
    with one row.  The output lies between two guard areas of a sentinel value that must come back untouched."""
    import torch
    nfr, guard = 17, 4096
    pcm = noise(NCH, n_samples(nfr), 900 + ncep)
    view = strided(pcm, 5)
    sentinel = -12345.678
    big = torch.full((guard + NCH * nfr * ncep + guard,), sentinel, dtype=torch.float32, device="cuda")
    out = big[guard:guard + NCH * nfr * ncep].view(NCH, nfr, ncep)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=ncep) as mfu, \
            mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=ncep, impl="generic") as mge:
        assert mfu.kernel_name() == W12
        got = mfu.process(view, out=out)
        b = mge.process(view).cpu().numpy()
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    want = torch.full((guard,), sentinel, dtype=torch.float32, device="cuda")
    assert torch.equal(big[:guard].view(torch.int32), want.view(torch.int32)), "written in front of the output"
    assert torch.equal(big[guard + NCH * nfr * ncep:].view(torch.int32), want.view(torch.int32)), "written behind the output"
    a = out.cpu().numpy()
    assert not (a == np.float32(sentinel)).any(), "an output element was not written"
    check_cepstra(a, b, pcm, "ncep %d" % ncep, n_cep=ncep)


# ----------------------------------------------------------------------------- silent frames: the fp32 `special` chain

@pytest.mark.parametrize("ncep", [13, 32])
def test_silent_frames_inside_a_tile(mfcc_amd, ncep):
    """Channel 1 has a stretch of zeros that makes frames 5..10 of its first tile all-zero: the tile runs the fp32 chain
    as well and those frames take its results.  eb.check holds their -inf / NaN pattern to the oracle's exactly."""
    nfr = 33
    pcm = noise(NCH, n_samples(nfr), 55 + ncep)
    pcm[1, 800:2300] = 0
    view = strided(pcm, 2)
    a, b = run_pair(mfcc_amd, view, 0, nfilters=32, nceptrums=ncep)
    ref, bound = eb.reference_and_bound(pcm[1], MODEL, n_cep=ncep)
    silent = np.isnan(bound).all(axis=1)
    assert silent[5:11].all() and silent.sum() == 6, np.flatnonzero(silent)
    assert np.isneginf(ref[5, 0]) and np.isneginf(a[1, 5, 0])
    check_cepstra(a, b, pcm, "silent ncep %d" % ncep, n_cep=ncep)


# ----------------------------------------------------------------------------- the other instantiations

@pytest.mark.parametrize("nfr", FRAME_COUNTS)
def test_dense_instantiation_16_filters(mfcc_amd, nfr):
    pcm = noise(NCH, n_samples(nfr), 300 + nfr)
    a, b = run_pair(mfcc_amd, strided(pcm, 1), 0, nfilters=16, nceptrums=13)
    check_cepstra(a, b, pcm, "dense nfr %d" % nfr, n_mel=16)


@pytest.mark.parametrize("nfr", FRAME_COUNTS)
def test_dc_instantiation_48_khz(mfcc_amd, nfr):
    pcm = noise(NCH, n_samples(nfr), 400 + nfr)
    a, b = run_pair(mfcc_amd, strided(pcm, 1), 0, nfilters=32, nceptrums=13, samplerate=48000)
    check_cepstra(a, b, pcm, "48 kHz nfr %d" % nfr, sample_rate=48000)


@pytest.mark.parametrize("nfr", FRAME_COUNTS)
def test_logmel_mode(mfcc_amd, nfr):
    pcm = noise(NCH, n_samples(nfr), 500 + nfr)
    a, b = run_pair(mfcc_amd, strided(pcm, 1), 0, nfilters=32, nceptrums=13, output="logmel")
    assert a.shape == (NCH, nfr, 32)
    bounds = []
    for c in range(NCH):
        ref, bound = lb.reference_and_bound(pcm[c], lb.MODEL[W12])
        eb.check(a[c], ref, bound, "logmel nfr %d channel %d" % (nfr, c))
        bounds.append(bound)
    against_generic(a, b, np.stack(bounds), "logmel nfr %d" % nfr)


def test_ragged_call_of_1_16_and_17_frames(mfcc_amd):
    """process_packed: three utterances of 1, 16 and 17 frames straight out of one buffer (the RAGGED instantiation)."""
    import torch
    rng = np.random.default_rng(61)
    utts = [rng.integers(-32768, 32768, size=n_samples(f) + extra).astype(np.int16) for f, extra in ((1, 3), (16, 0), (17, 5))]
    offsets = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.uint64)
    flat = torch.from_numpy(np.concatenate(utts)).cuda()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as mfu, \
            mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, impl="generic") as mge:
        assert mfu.kernel_name() == W12
        out, fo = mfu.process_packed(flat, offsets)
        outg, fog = mge.process_packed(flat, offsets)
        torch.cuda.synchronize()
        out, outg = out.cpu().numpy(), outg.cpu().numpy()
        single = [mfu.process(torch.from_numpy(u).cuda()).cpu().numpy() for u in utts]
    assert fo.tolist() == fog.tolist() == [0, 1, 17, 34]
    for i, u in enumerate(utts):
        a = out[int(fo[i]):int(fo[i + 1])]
        assert np.array_equal(a, single[i]), "utterance %d differs from its own call" % i
        check_cepstra(a[None], outg[None, int(fo[i]):int(fo[i + 1])], u[None], "ragged utterance %d" % i)


# ----------------------------------------------------------------------------- pre-emphasis at the extremes

def test_full_scale_samples(mfcc_amd):
    """32 x - 31 x' at its extremes (+2 064 352 and -2 064 353: both inside the 2^22 the biased dot product holds exactly).
    Channel 0 alternates -32768 / 32767; channel 1 takes the two extremes in a random order, which reaches the same
    pre-emphasis values with energy in every band; channel 2 is noise.  The alternating channel's energy sits in three FFT
    bins: the model leaves bands without them open (bound +inf), the rest is checked like everything else."""
    nfr = 17
    n = n_samples(nfr)
    rng = np.random.default_rng(3)
    pcm = noise(NCH, n, 33)
    pcm[0] = np.where(np.arange(n) & 1, 32767, -32768)
    pcm[1] = np.where(rng.integers(0, 2, n) == 1, 32767, -32768)
    a, b = run_pair(mfcc_amd, strided(pcm, 6), 0, nfilters=32, nceptrums=13)
    check_cepstra(a, b, pcm, "full scale")
    ref1, bound1 = eb.reference_and_bound(pcm[1], MODEL, n_cep=13)
    assert np.isfinite(bound1).all()                   # the random-order channel is constrained in every frame
