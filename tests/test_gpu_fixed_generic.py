"""The fixed-point contract over the RTL's whole parameter space: every nfft 64..1024, every n_mel in {4, 8, 16, 32, 64}
with a (4 n_mel)-point DCT FFT no longer than the frame, every rate 8 .. 48 kHz.  Where the oracle's streaming filterbank
asserts, ``process_fixed`` fails with UNSUPPORTED (-105) and nothing else; everywhere else the output is the oracle's, bit
for bit, on the kernel the routing rule names.  Then the generic fixed kernel's frame cursor at its two extremes: more
channels than the grid has waves, and one channel of more than 100 k frames.  (The host tables of the same grid are
checked without a GPU in tests/test_cabi_host.py.)"""
import numpy as np
import pytest

from oracle import mfcc_fixed as mx
from oracle import mfcc_float as mf

pytestmark = pytest.mark.gpu
NFFTS = (64, 128, 256, 512, 1024)
NMELS = (4, 8, 16, 32, 64)
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)
PAIRS = [(nfft, nmel) for nfft in NFFTS for nmel in NMELS if 4 * nmel <= nfft]
MEL_CHUNK = 12          # taps per lane the fused fixed-point kernel is unrolled for (kernel_fixed512.hpp: kMelChunk)


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _oracle(pcm, nfft, nmel, sr, pad):
    """The RTL oracle with every coefficient (n_cep = n_mel), or None where it asserts."""
    try:
        return mx.mfcc_fixed_ref(pcm, nfft=nfft, nfilters=nmel, nceptrums=nmel, sample_rate=float(sr), pad_mode=pad)
    except AssertionError:
        return None


def _expected_kernel(mfcc_amd, nfft, nmel, sr):
    """mfcc_fixed512_kernel where mfcc_fixed512::supported holds (512 with 16 or 32 filters) and every filter's taps
    can be dealt out to the 64 lanes in pieces of at most MEL_CHUNK (build_mel_lanes); mfcc_fixed_kernel elsewhere."""
    if nfft != 512 or nmel not in (16, 32):
        return "mfcc_fixed_kernel"
    from mfcc_amd import _lib
    W = mfcc_amd.get_table(_lib.TABLE_FX_MEL_DENSE_U32, nfft=nfft, nfilters=nmel, nceptrums=1, samplerate=sr)[1:]
    W = W.reshape(nmel, nfft // 2)
    counts = []
    for row in W:
        nz = np.flatnonzero(row)
        counts.append(int(nz[-1] - nz[0] + 1) if len(nz) else 0)
    fits = any(sum(-(-c // chunk) if c else 1 for c in counts) <= 64 for chunk in range(1, MEL_CHUNK + 1))
    return "mfcc_fixed512_kernel" if fits else "mfcc_fixed_kernel"


def _inputs(wav_pcm, n, seed):
    """Speech, full-scale uniform noise and sample-by-sample alternating extremes."""
    rng = np.random.default_rng(seed)
    return np.stack([np.resize(wav_pcm[(seed * 131) % 50000:], n).astype(np.int16),
                     rng.integers(-32768, 32768, n).astype(np.int16),
                     np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)])


@pytest.mark.parametrize("pad", ["stream", "notebook"])
@pytest.mark.parametrize("nfft,nmel", PAIRS)
def test_every_rtl_parameter_set_is_bit_exact_or_refused(mfcc_amd, wav_pcm, nfft, nmel, pad):
    refused = ran = 0
    for i, sr in enumerate(RATES):
        nfr = 20 + (7 * i + nfft // 64 + nmel) % 21                     # 20 .. 40 frames
        n = (nfft // 3) * (nfr - 1) + nfft + (nfft // 6 if pad == "stream" else 0)
        pcm = _inputs(wav_pcm, n, nfft + nmel + i)
        ref = _oracle(pcm, nfft, nmel, sr, pad)
        for ncep in sorted({1, nmel}):
            with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=ncep, samplerate=sr, pad_mode=pad) as m:
                if ref is None:
                    with pytest.raises(mfcc_amd.MfccHipError) as e:
                        m.process_fixed(pcm)
                    assert e.value.code == -105, (nfft, nmel, sr)
                    refused += 1
                    continue
                assert m.kernel_name(fixed=True) == _expected_kernel(mfcc_amd, nfft, nmel, sr), (nfft, nmel, sr)
                got = m.process_fixed(pcm)
            assert got.shape == ref[..., :ncep].shape, (nfft, nmel, sr, ncep)
            if not np.array_equal(got, ref[..., :ncep]):
                c, f, k = np.argwhere(got != ref[..., :ncep])[0]
                raise AssertionError("nfft %d n_mel %d %d Hz n_cep %d %s: channel %d frame %d coef %d: got %d, oracle %d"
                                     % (nfft, nmel, sr, ncep, pad, c, f, k, got[c, f, k], ref[c, f, k]))
            ran += 1
    assert ran + refused == 7 * len({1, nmel})
    assert ran or nfft == 4 * nmel                                      # such a dense bank streams at no rate


def _batched_oracle(pcm, nfft, nmel, ncep, pad, block=16384):
    """mfcc_fixed_ref of many short channels at once: each channel padded, pre-emphasised and framed on its own exactly
    as mfcc_fixed_ref does, then the stages of oracle/mfcc_fixed.py on all frames together, ``block`` frames at a time."""
    hop = nfft // 3
    n = pcm.shape[1]
    nf = mf.num_frames_stream(n, nfft, hop) if pad == "stream" else mf.num_frames_notebook(n, nfft, hop)
    need = (nf - 1) * hop + nfft
    x = np.zeros((len(pcm), max(n, need)), np.int64)
    x[:, :n] = pcm
    y = mx.wrap16(x + (np.concatenate([np.zeros((len(x), 1), np.int64), x[:, :-1]], axis=1) >> 5)
                  - np.concatenate([np.zeros((len(x), 1), np.int64), x[:, :-1]], axis=1))
    idx = hop * np.arange(nf)[:, None] + np.arange(nfft)[None, :]
    frames = y[:, idx].reshape(-1, nfft)
    curve = mx.window_curve(nfft)
    out = []
    for a in range(0, len(frames), block):
        re, im = mx.fft_fixed(mx.window_apply(frames[a:a + block], curve), nfft)
        lg = mx.log2_fix(mx.filterbank(mx.power_spectrum(re, im), nfft, nmel))
        out.append(mx.dct_fixed(lg, nmel)[:, :ncep].astype(np.int16))
    return np.concatenate(out).reshape(len(pcm), nf, ncep)


@pytest.mark.parametrize("frames", [1, 3])
def test_more_channels_than_the_grid_has_waves(mfcc_amd, frames):
    """40 000 channels of `frames` frames: more frames than the capped grid has waves (n_cu * 32 workgroups of 4 waves,
    32 768 on MI355X), so the (channel, frame) cursor steps by whole channels (step_ch > 0) and, at 3 frames, carries
    the frame remainder (step_f = 2) across a channel boundary."""
    import torch
    nfft, nmel, ncep, nch = 64, 8, 8, 40_000
    n = (nfft // 3) * (frames - 1) + nfft + 5
    rng = np.random.default_rng(frames)
    pcm = rng.integers(-32768, 32768, (nch, n)).astype(np.int16)
    pcm[::7] = (rng.standard_normal((len(pcm[::7]), n)) * 2000).astype(np.int16)
    pcm[3::11, :n // 2] = 0
    with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=ncep, pad_mode="notebook") as m:
        assert m.kernel_name(fixed=True) == "mfcc_fixed_kernel"
        got = m.process_fixed(torch.from_numpy(pcm).cuda()).cpu().numpy()
    ref = _batched_oracle(pcm, nfft, nmel, ncep, "notebook")
    for c in (0, 1, 7, nch - 1):                                       # the batched form is the oracle's own
        assert np.array_equal(ref[c], mx.mfcc_fixed_ref(pcm[c], nfft=nfft, nfilters=nmel, nceptrums=ncep,
                                                       pad_mode="notebook"))
    assert got.shape == ref.shape == (nch, frames, ncep) and nch * frames > 32_768
    bad = np.argwhere((got != ref).any(axis=2))
    assert len(bad) == 0, "%d frame(s) differ, first (channel, frame) %s" % (len(bad), tuple(bad[0]))


def test_one_channel_of_more_than_100k_frames(mfcc_amd, wav_pcm):
    import torch
    nfft, nmel, ncep = 64, 8, 8
    hop = nfft // 3
    n = hop * 100_500 + nfft + 9
    rng = np.random.default_rng(9)
    pcm = np.resize(wav_pcm, n).astype(np.int16)
    pcm[n // 3: n // 3 + 50_000] = rng.integers(-32768, 32768, 50_000)
    pcm[n // 2: n // 2 + 5_000] = 0
    with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=ncep, pad_mode="stream") as m:
        assert m.kernel_name(fixed=True) == "mfcc_fixed_kernel"
        got = m.process_fixed(torch.from_numpy(pcm).cuda()).cpu().numpy()
    ref = mx.mfcc_fixed_ref(pcm, nfft=nfft, nfilters=nmel, nceptrums=ncep, pad_mode="stream")
    assert got.shape == ref.shape and len(ref) > 100_000
    bad = np.argwhere((got != ref).any(axis=1))
    assert len(bad) == 0, "%d frame(s) differ, first %d" % (len(bad), bad[0][0])
