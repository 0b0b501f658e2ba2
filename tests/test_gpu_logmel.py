"""The log-mel output mode (``output="logmel"``) on the GPU: every float entry point returns rows of ``n_mel`` log2 mel
band energies, held element by element to the bound of tests/logmel_bound.py (the notebook's own log-mel stage and the
declared arithmetic of the kernel that ran), bit-identical across the one-shot, ragged and streaming entry points, and
refused by the fixed-point path and the ``.mfcc`` writers."""
import ctypes as C

import numpy as np
import pytest

import logmel_bound as lb
from oracle import error_bound as eb
from oracle import mfcc_float as mf

pytestmark = pytest.mark.gpu
W512, W1K, GEN = "mfcc_fused512_w12_kernel", "mfcc_fused1024_w12bf_kernel", "mfcc_float_generic_kernel"
KINDS = ["wav", "noise3000", "noise30", "uniform", "square", "sine", "dc_dither", "silences"]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def signal(kind, n, seed, wav_pcm):
    """The input kinds of tests/test_gpu_error_bound.py."""
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


def n_for(frames, nfft=512, hop=170):
    return nfft + hop * (frames - 1)


def check_channels(got, pcm, kernel, what, **kw):
    for c in range(len(pcm)):
        lb.check(got[c], pcm[c], kernel, "%s channel %d (%s)" % (what, c, KINDS[c % len(KINDS)]), **kw)


# ---------------------------------------------------------------------------------------------------- golden wav
@pytest.mark.parametrize("impl,kernel", [("auto", W512), ("generic", GEN)])
def test_logmel_golden_wav(mfcc_amd, wav_pcm, golden_dir, impl, kernel):
    import os
    gold = np.load(os.path.join(golden_dir, "f2bjrop_float64_logmel32.npy"))
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, impl=impl, output="logmel") as m:
        assert m.kernel_name() == kernel and m.num_features == 32
        got = m.process(wav_pcm)
    assert got.shape == (1046, 32) and got.dtype == np.float32
    assert np.abs(got - gold).max() / np.abs(gold).max() <= 1e-4
    lb.check(got, wav_pcm, kernel, "golden wav " + impl)


# ---------------------------------------------------------------------------------------------------- per element
@pytest.mark.parametrize("frames", [1, 15, 16, 17, 31, 33, 1500])
def test_logmel_bound_512_frame_counts(mfcc_amd, wav_pcm, frames):
    pcm = all_kinds(n_for(frames) + 37, 11 * frames, wav_pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, output="logmel") as m:
        assert m.kernel_name() == W512
        got = m.process(pcm)
    assert got.shape == (len(KINDS), frames, 32)
    check_channels(got, pcm, W512, "frames %d" % frames)


def test_logmel_bound_512_odd_stride_and_halo(mfcc_amd, wav_pcm):
    import torch
    nch, n, stride, off = 5, n_for(40) + 11, n_for(40) + 11 + 7, 3
    flat = np.concatenate([signal(KINDS[i % len(KINDS)], stride, 5 + i, wav_pcm) for i in range(nch)] +
                          [np.zeros(off, np.int16)])
    dev = torch.as_strided(torch.from_numpy(flat).cuda(), (nch, n), (stride, 1), storage_offset=off)
    pcm = np.stack([flat[off + c * stride: off + c * stride + n] for c in range(nch)])
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, output="logmel") as m:
        assert m.kernel_name() == W512
        got = m.process(dev)
        got_h = m.process(dev, halo=1)
        torch.cuda.synchronize()
    got, got_h = got.cpu().numpy(), got_h.cpu().numpy()
    assert got.shape == (nch, mf.num_frames_notebook(n), 32)
    for c in range(nch):
        lb.check(got[c], pcm[c], W512, "stride channel %d" % c)
        lb.check(got_h[c], pcm[c], W512, "halo channel %d" % c, halo=1)


def test_logmel_bound_512_stream_padding(mfcc_amd, wav_pcm):
    pcm = all_kinds(n_for(33) + 101, 3, wav_pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, pad_mode="stream", output="logmel") as m:
        assert m.kernel_name() == W512
        got = m.process(pcm)
    assert got.shape[1] == mf.num_frames_stream(pcm.shape[1])
    check_channels(got, pcm, W512, "stream padding", pad_mode="stream")


@pytest.mark.parametrize("rate", [16000, 44100, 48000])
@pytest.mark.parametrize("nmel", [16, 32])
def test_logmel_bound_512_nmel_and_rates(mfcc_amd, wav_pcm, nmel, rate):
    """n_mel 16 is a 16-wide row (the kernel must not store bands 16..31); 44.1 / 48 kHz take the exact-DC path."""
    import torch
    frames = 35
    pcm = all_kinds(n_for(frames), 17 + nmel, wav_pcm)
    nch = len(pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=nmel, nceptrums=13, samplerate=rate, output="logmel") as m:
        assert m.kernel_name() == W512 and m.num_features == nmel
        got = m.process(pcm)
        # device path into a buffer with a guard behind the last row: nothing may land past the output
        buf = torch.full((nch * frames * nmel + 256,), 12345.0, device="cuda")
        out = buf[:nch * frames * nmel].view(nch, frames, nmel)
        m.process(torch.from_numpy(pcm).cuda(), out=out)
        torch.cuda.synchronize()
    assert got.shape == (nch, frames, nmel)
    assert bool((buf[nch * frames * nmel:] == 12345.0).all())
    assert np.array_equal(out.cpu().numpy(), got)
    check_channels(got, pcm, W512, "n_mel %d at %d Hz" % (nmel, rate), n_mel=nmel, sample_rate=rate)


@pytest.mark.parametrize("rate", [16000, 48000])
def test_logmel_bound_1024(mfcc_amd, wav_pcm, rate):
    frames = 37
    pcm = all_kinds(n_for(frames, 1024, 341) + 5, 23, wav_pcm)
    with mfcc_amd.MFCC(nfft=1024, nfilters=40, nceptrums=13, samplerate=rate, output="logmel") as m:
        assert m.kernel_name() == W1K and m.num_features == 40
        got = m.process(pcm)
    assert got.shape == (len(KINDS), frames, 40)
    check_channels(got, pcm, W1K, "1024 at %d Hz" % rate, nfft=1024, hop=341, n_mel=40, sample_rate=rate)


@pytest.mark.parametrize("nfft", [256, 1024])
def test_logmel_bound_generic(mfcc_amd, wav_pcm, nfft):
    hop = nfft // 3
    frames = 21
    pcm = all_kinds(n_for(frames, nfft, hop), 29, wav_pcm)
    with mfcc_amd.MFCC(nfft=nfft, nfilters=64, nceptrums=13, output="logmel") as m:
        assert m.kernel_name() == GEN and m.num_features == 64
        got = m.process(pcm)
    assert got.shape == (len(KINDS), frames, 64)
    check_channels(got, pcm, GEN, "generic %d" % nfft, nfft=nfft, hop=hop, n_mel=64, power_scale=512.0)


# ---------------------------------------------------------------------------------------------------- consistency
@pytest.mark.parametrize("nfft,nmel,kernel", [(512, 32, W512), (1024, 40, W1K), (256, 24, GEN)])
def test_logmel_and_cepstra_agree(mfcc_amd, wav_pcm, nfft, nmel, kernel):
    """cepstra of a cepstra handle vs logmel @ dct[:n_cep].T of a log-mel handle, within B_cep + B_logmel @ |dct|.T"""
    hop, ncep = nfft // 3, 13
    pcm = signal("wav", n_for(50, nfft, hop), 3, wav_pcm)
    with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=ncep) as mc, \
            mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=ncep, output="logmel") as ml:
        assert ml.kernel_name() == kernel
        cep = mc.process(pcm).astype(np.float64)
        lm = ml.process(pcm).astype(np.float64)
        cep_model = eb.model_of(mc.kernel_name())
    D = mf.dct_basis(nmel, nmel)[:ncep]
    kw = dict(nfft=nfft, hop=hop, n_mel=nmel)
    _, b_cep = eb.reference_and_bound(pcm, cep_model, ncep, **kw)
    _, b_lm = lb.reference_and_bound(pcm, lb.MODEL[kernel], **kw)
    tol = b_cep + b_lm @ np.abs(D).T
    held = np.isfinite(tol)                                  # frames either bound leaves open are not compared
    assert held.mean() > 0.9
    d = np.abs(lm @ D.T - cep)
    assert (d[held] <= tol[held]).all(), float(np.max(d[held] / tol[held]))


# ---------------------------------------------------------------------------------------------------- ragged, streaming
LENS = [0, 5000, 511, 512, 12345, 170 * 40 + 512, 100, 3000, 70000, 513]


@pytest.mark.parametrize("nfft,nmel,impl", [(512, 32, "auto"), (512, 16, "auto"), (1024, 40, "auto"),
                                            (512, 32, "generic")])
def test_logmel_batch_is_bitwise_per_utterance(mfcc_amd, wav_pcm, nfft, nmel, impl):
    import torch
    utts = [signal(KINDS[i % len(KINDS)], n, 40 + i, wav_pcm) for i, n in enumerate(LENS)]
    with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=13, impl=impl, output="logmel") as m:
        one = [m.process(u) for u in utts]
        assert all(o.shape == (m.num_frames(len(u)), nmel) for o, u in zip(one, utts))
        host = m.process_batch(utts)
        dev = m.process_batch([torch.from_numpy(u).cuda() for u in utts])
        flat = torch.from_numpy(np.concatenate(utts)).cuda()
        offs = np.concatenate([[0], np.cumsum([len(u) for u in utts])])
        packed, fo = m.process_packed(flat, offs)
        # equal lengths: the multi-channel fast path
        eq = m.process_packed(torch.from_numpy(np.concatenate(utts[1:2] * 3)).cuda(), [0, 5000, 10000, 15000])[0]
        torch.cuda.synchronize()
    for i, o in enumerate(one):
        assert np.array_equal(host[i], o, equal_nan=True), i
        assert np.array_equal(dev[i].cpu().numpy(), o, equal_nan=True), i
        assert np.array_equal(packed[int(fo[i]):int(fo[i + 1])].cpu().numpy(), o, equal_nan=True), i
    assert np.array_equal(eq.cpu().numpy(), np.concatenate([one[1]] * 3), equal_nan=True)


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("nfft,nmel", [(512, 32), (1024, 40), (256, 64)])
def test_logmel_stream_is_bitwise_one_shot(mfcc_amd, wav_pcm, pad, nfft, nmel):
    n = n_for(30, nfft, nfft // 3) + 77
    pcm = signal("silences", n, 8, wav_pcm)
    with mfcc_amd.MFCC(nfft=nfft, nfilters=nmel, nceptrums=13, pad_mode=pad, output="logmel") as m:
        ref = m.process(pcm)
        rng = np.random.default_rng(1)
        for chunks in ("uneven", "ones"):
            with m.stream() as s:
                rows, i = [], 0
                while i < n:
                    k = 1 if chunks == "ones" and i < 1500 else int(rng.integers(1, 3 * nfft))
                    rows.append(s.push(pcm[i:i + k]))
                    i += k
                rows.append(s.flush())
            got = np.concatenate(rows)
            assert got.shape == ref.shape == (m.num_frames(n), nmel)
            assert np.array_equal(got, ref, equal_nan=True), chunks


def test_logmel_stream_capacity_is_in_rows_of_n_mel(mfcc_amd, wav_pcm):
    from mfcc_amd import _lib as L
    pcm = signal("wav", 512 + 170 * 9, 2, wav_pcm)            # 10 frames
    nf, ncep, nmel = 10, 13, 32
    with mfcc_amd.MFCC(nfft=512, nfilters=nmel, nceptrums=ncep, output="logmel") as m:
        s = m.stream()
        lib = m._lib
        out = np.full(nf * nmel, 7.0, np.float32)
        got = C.c_size_t(0)
        rc = lib.mfcc_hip_stream_push(s._s, pcm.ctypes.data, pcm.size, out.ctypes.data, nf * ncep, C.byref(got))
        assert rc == L.ERROR_BUFFER_SMALL and s.pending == 0 and (out == 7.0).all()
        rc = lib.mfcc_hip_stream_push(s._s, pcm.ctypes.data, pcm.size, out.ctypes.data, nf * nmel, C.byref(got))
        assert rc == L.SUCCESS and got.value == nf
        assert np.array_equal(out.reshape(nf, nmel), m.process(pcm))
        s.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_logmel_refuses_fixed_point_and_mfcc_files(mfcc_amd, wav_pcm, tmp_path):
    import torch
    from mfcc_amd import _lib as L
    from scipy.io import wavfile
    wav = str(tmp_path / "a.wav")
    wavfile.write(wav, 16000, wav_pcm[:5000])
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=32, pad_mode="stream", output="logmel") as m:
        calls = [lambda: m.process_fixed(wav_pcm[:5000]),
                 lambda: m.process_fixed(torch.from_numpy(wav_pcm[:5000]).cuda()),
                 lambda: m.process_batch([wav_pcm[:5000]], fixed=True),
                 lambda: m.stream(fixed=True),
                 lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=False),
                 lambda: m.convert(wav, str(tmp_path / "a.mfcc"), fixed=True),
                 lambda: m.convert_many([wav], [str(tmp_path / "a.mfcc")], fixed=False)]
        for i, call in enumerate(calls):
            with pytest.raises(mfcc_amd.MfccHipError) as e:
                call()
            assert e.value.code == L.ERROR_UNSUPPORTED, i
        assert not (tmp_path / "a.mfcc").exists()
        # the float path of the same handle still works
        assert m.process(wav_pcm[:5000]).shape == (mf.num_frames_stream(5000), 32)


def test_logmel_time_launches(mfcc_amd, wav_pcm):
    import torch
    pcm = torch.from_numpy(all_kinds(n_for(64), 1, wav_pcm)).cuda()
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, output="logmel") as m:
        out = torch.empty((pcm.shape[0], 64, 32), device="cuda")
        ms = m.time_launches(pcm, out, warmup=1, iters=3)
        ref = m.process(pcm.cpu().numpy())
    assert ms > 0 and np.array_equal(out.cpu().numpy(), ref, equal_nan=True)
