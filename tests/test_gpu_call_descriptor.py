"""Refused calls between good ones, on handles where every setting a call may have to ignore is set.

What a call computes travels through the host routes as a value (``Call`` and ``Samples`` in mfcc_hip.hip); no call writes a
setting of the handle.  So a call that is refused from INSIDE a route -- behind the decode and the resampling, in
``launch()`` or in the ragged scan -- must leave the handle exactly as it found it: the getters read as before and the next
good call of every kind returns the bits it returned first.  The handles carry a log-mel HTK bank, sliding mean / variance
normalization, PCEN, deltas, mu-law input at 8 kHz and a filterbank matrix; ``power_spectrum`` and ``filterbank`` ignore
the passes, ``process`` runs them all.  One handle runs the fused kernels (512 / 160 / 400), one the generic ones (256)."""
import ctypes as C
import wave

import numpy as np
import pytest

from kernel_families import same

pytestmark = pytest.mark.gpu

FRAMES = 17
OFFSETS = [0, 3000, 7000]
CFGS = {
    "fused512": (dict(nfft=512, hop=160, win_length=400), "mfcc_spectrum512_kernel", "mfcc_fbank512_kernel", False),
    "generic256": (dict(nfft=256, hop=80, win_length=200), "mfcc_spectrum_generic_kernel", "mfcc_fbank_generic_kernel", True),
}


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _open(mfcc_amd, cfg):
    geom, spec_kernel, fbank_kernel, generic = CFGS[cfg]
    m = mfcc_amd.MFCC(nfilters=16, nceptrums=13, samplerate=16000, output="logmel", mel="htk", normalize="meanvar",
                      normalize_window=9, deltas=2, pcen=True, sample_format="ulaw", input_rate=8000, **geom)
    try:
        m.set_filterbank(mfcc_amd.htk_filterbank(8, nfft=geom["nfft"], samplerate=16000), "log2")
        assert ("generic" in m.kernel_name()) == generic, m.kernel_name()
        assert m.spectrum_kernel_name() == spec_kernel and m.filterbank_kernel_name() == fbank_kernel
    except BaseException:
        m.close()
        raise
    return m


@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_refused_calls_leave_the_handle_as_it_was(mfcc_amd, cfg):
    import torch
    from mfcc_amd import _lib as L
    rng = np.random.default_rng(20)
    with _open(mfcc_amd, cfg) as m:
        lib, h = m._lib, m._h
        n = next(k for k in range(1, 4000) if m.num_frames(k) == FRAMES)
        x = torch.from_numpy(rng.integers(0, 256, (2, n), dtype=np.uint8)).cuda()
        flat = torch.from_numpy(rng.integers(0, 256, OFFSETS[-1], dtype=np.uint8)).cuda()

        def state():
            bands = C.c_size_t(0)
            assert lib.mfcc_hip_fbank_bands(h, C.byref(bands)) == L.SUCCESS
            return m.num_features, lib.mfcc_hip_sample_format(h), lib.mfcc_hip_input_rate(h), bands.value

        before = state()
        assert before == (16 * 3, L.SAMPLE_ULAW, 8000, 8)
        good = {
            "process": lambda: m.process(x),
            "spectrum": lambda: m.power_spectrum(x),
            "fbank": lambda: m.filterbank(x),
            "process_packed": lambda: m.process_packed(flat, OFFSETS)[0],
            "spectrum_packed": lambda: m.power_spectrum_packed(flat, OFFSETS)[0],
            "fbank_packed": lambda: m.filterbank_packed(flat, OFFSETS)[0],
        }
        want = {k: f().cpu() for k, f in good.items()}
        assert tuple(want["process"].shape) == (2, FRAMES, 48) and tuple(want["spectrum"].shape) == (2, FRAMES, m.num_bins)
        assert tuple(want["fbank"].shape) == (2, FRAMES, 8) and want["spectrum_packed"].shape[1] == m.num_bins
        assert want["process_packed"].shape[1] == 48 and want["fbank_packed"].shape[1] == 8
        assert not same(want["fbank"], want["process"][:, :, :8])                 # three outputs, not one

        got = C.c_size_t(0)
        out = torch.empty((2, FRAMES, m.num_bins), dtype=torch.float32, device="cuda")
        fo = np.zeros(3, np.uint64)
        down = np.array(OFFSETS[::-1], np.uint64)
        refused = [
            # a spectrum call with a misaligned `out`: refused by launch(), behind the decode and the resampling
            (lambda: lib.mfcc_hip_spectrum_i16_dev(h, L.ptr(x), n, n, 2, 0, out.data_ptr() + 2, C.byref(got)),
             L.ERROR_INVALID_PARAM),
            # a shard's edge on a handle with an input rate: refused by the dense route
            (lambda: lib.mfcc_hip_fbank_i16_dev(h, L.ptr(x), n - 1, n, 2, 1, L.ptr(out), C.byref(got)), L.ERROR_UNSUPPORTED),
            (lambda: lib.mfcc_hip_process_i16_dev(h, L.ptr(x), n - 1, n, 2, 1, L.ptr(out), C.byref(got)), L.ERROR_UNSUPPORTED),
            # decreasing offsets: refused by the ragged route
            (lambda: lib.mfcc_hip_spectrum_ragged_i16_dev(h, L.ptr(flat), L.ptr(down), 2, L.ptr(out), out.numel(), L.ptr(fo)),
             L.ERROR_INVALID_PARAM),
        ]
        # another order than the first pass, dense and packed forms in turn
        after = [("fbank_packed", "process", "spectrum_packed"), ("spectrum", "fbank", "process_packed"),
                 ("process", "fbank_packed", "spectrum"), ("spectrum_packed", "process_packed", "fbank")]
        for (call, code), kinds in zip(refused, after):
            assert call() == code
            m.synchronize()            # what the refused call had enqueued on the handle's own stream has left the scratch
            assert state() == before
            for k in kinds:
                assert same(good[k](), want[k]), "%s after a refused call" % k
        torch.cuda.synchronize()


def test_convert_wav_reads_pcm16_on_a_ulaw_handle(mfcc_amd, tmp_path, wav_pcm):
    """``convert`` hands the file's 16-bit PCM to the routes as int16, whatever the handle's sample format, and the handle
    keeps that format."""
    from mfcc_amd import _lib as L
    pcm = np.ascontiguousarray(wav_pcm[:4000], dtype="<i2")
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    ulaw = np.random.default_rng(21).integers(0, 256, 4000, dtype=np.uint8)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, samplerate=16000) as plain:
        rows = plain.process(pcm)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, samplerate=16000, sample_format="ulaw") as m:
        want = m.process(ulaw)
        nf = m.convert(str(path), str(tmp_path / "a.mfcc"), fixed=False)
        assert m._lib.mfcc_hip_sample_format(m._h) == L.SAMPLE_ULAW
        assert same(m.process(ulaw), want)
    # the file holds the int16 handle's rows of the PCM: NaN as 0, saturated, truncated
    assert nf == len(rows)
    as_i16 = np.clip(np.nan_to_num(rows, nan=0.0, posinf=32767.0, neginf=-32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(np.fromfile(tmp_path / "a.mfcc", dtype="<i2").reshape(nf, 13), as_i16)
