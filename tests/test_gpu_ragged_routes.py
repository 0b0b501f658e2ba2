"""One kernel family per route of a ragged call (mfcc_amd/csrc/batch_plan.hpp: mfcc_batch::Route), on the corpora that
tests/test_gpu_entry_points.py E6 does not contain: empty utterances at the front, at the end and in a row; no frame at
all; ``offsets[0]`` above 0; three equal lengths but for one sample, which only just miss the uniform route.  Every
corpus goes through the device entry and the host entry of the C ABI into a buffer with rows to spare, and is held bit for
bit against one call per utterance; the spare rows must come back untouched.  A handful of frames each."""
import ctypes as C

import numpy as np
import pytest

import kernel_families as kf
from kernel_families import as_np, open_handle, run, same

pytestmark = pytest.mark.gpu

# tile records, frame records, pack-and-gather (float and fixed), pack-and-gather on a fused kernel
ROUTES = ["f512", "x512", "g256", "x256_16", "f1024"]
FAMS = [f for f in kf.ALL if f.id in ROUTES]
SPARE, MARK = 3, 12345


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def corpus(fam, case):
    """(utterance lengths, offsets[0])"""
    hop, nfft = fam.hop, fam.nfft
    if case == "empties":
        return [0, 0, nfft + 2 * hop, 0, 0, 1, nfft, 17 * hop + nfft, 0], 0
    if case == "no_frames":
        return [0, 1, nfft - 1, 0], 0
    if case == "offset0":
        return [nfft + hop + 3, nfft - 1, 16 * hop + nfft], 5
    if case == "just_not_uniform":
        return [nfft + 3 * hop, nfft + 3 * hop + 1, nfft + 3 * hop], 0
    raise ValueError(case)


def ragged(m, fam, flat, offs, rows, host):
    """mfcc_hip_process_ragged_*[_dev] on ``flat`` into ``rows`` + SPARE rows of MARK: (code, rows, frame_offsets)"""
    import torch
    n = len(offs) - 1
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    fo = np.full(n + 1, 99, dtype=np.uint64)
    out = np.full((rows + SPARE, m._row(fam.fixed)), MARK, dtype=np.int16 if fam.fixed else np.float32)
    name = "mfcc_hip_process_ragged%s_i16%s" % ("_fixed" if fam.fixed else "", "" if host else "_dev")
    if host:
        flat = np.ascontiguousarray(flat)
        rc = getattr(m._lib, name)(m._h, flat.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), n,
                                   out.ctypes.data_as(C.c_void_p), out.size, fo.ctypes.data_as(C.c_void_p))
        return rc, out, fo
    d_flat, d_out = torch.from_numpy(np.ascontiguousarray(flat)).cuda(), torch.from_numpy(out).cuda()
    with m._on_torch_stream(d_flat.device):
        rc = getattr(m._lib, name)(m._h, C.c_void_p(d_flat.data_ptr()), offs.ctypes.data_as(C.c_void_p), n,
                                   C.c_void_p(d_out.data_ptr()), d_out.numel(), fo.ctypes.data_as(C.c_void_p))
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), fo


CASES = [(c, p) for c in ("empties", "offset0", "just_not_uniform") for p in ("notebook", "stream")] + [("no_frames", "notebook")]


@pytest.mark.parametrize("case,pad", CASES, ids=["%s-%s" % cp for cp in CASES])
@pytest.mark.parametrize("fam", FAMS, ids=[f.id for f in FAMS])
def test_ragged_route_equals_per_utterance_calls(mfcc_amd, wav_pcm, fam, case, pad):
    lens, off0 = corpus(fam, case)
    kinds = ["speech", "noise", "uniform", "square", "silences"]
    utts = [kf.signal(kinds[i % len(kinds)], v, 300 + i, wav_pcm) for i, v in enumerate(lens)]
    flat = np.concatenate([kf.signal("noise", off0, 299, wav_pcm)] + utts)
    offs = off0 + np.concatenate([[0], np.cumsum(lens)])
    with open_handle(mfcc_amd, fam, pad) as m:                  # asserts kernel_name() first
        one = [as_np(run(m, fam, u)) for u in utts]
        counts = [m.num_frames(v) for v in lens]
        assert [len(o) for o in one] == counts
        want_fo = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        total = int(want_fo[-1])
        assert (total == 0) == (case == "no_frames")
        for host in (False, True):
            rc, out, fo = ragged(m, fam, flat, offs, total, host)
            what = (fam.id, case, pad, "host" if host else "device")
            assert rc == 0 and np.array_equal(fo, want_fo), (what, rc, fo)
            for i, o in enumerate(one):
                assert same(out[int(fo[i]):int(fo[i + 1])], o), (what, i, lens[i])
            assert (out[total:] == MARK).all(), what             # nothing behind the last row (no frame: nothing at all)
