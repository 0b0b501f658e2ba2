"""What every entry point of ``mfcc_amd.api`` raises for an ``out`` tensor, an offsets array or a host sample array it
cannot take: the exception TYPE, pinned per entry point and kind of mistake (DESIGN.md has the table).  Every refusal
comes from Python or from the library's argument checks, in front of any launch, so after each one a valid ``process``
on the same handle still gives the bits it gave when the module started.  The forms of ``frame_offsets`` a segment pass
takes (a list, a NumPy array, a torch CPU tensor, one entry) are held to one result.

Shapes: a default 512 / 170 handle with 32 filters and 13 coefficients, ``pcm`` of 2 channels x 1022 samples (4 frames
each), rows tensors of ``(2, 8, 13)``."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH, NS, NF, W = 2, 1022, 4, 13            # channels, samples and frames of each, row width
ROWS, K = 8, 4                             # rows per segment of the rows tensors, rows of a gate window


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    rng = np.random.default_rng(11)
    e = types.SimpleNamespace(torch=torch, mfcc_amd=mfcc_amd)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        e.m = m
        e.pcm_np = rng.integers(-20000, 20000, (NCH, NS)).astype(np.int16)
        e.pcm = torch.from_numpy(e.pcm_np).cuda()
        e.flat = e.pcm.reshape(-1)
        assert m.num_frames(NS) == NF
        e.base = m.process(e.pcm).clone()
        e.rows_f = torch.from_numpy(rng.standard_normal((NCH, ROWS, W)).astype(np.float32)).cuda()
        e.rows_i = torch.from_numpy(rng.integers(-3000, 3000, (NCH, ROWS, W)).astype(np.int16)).cuda()
        e.voiced = torch.ones((NCH, ROWS), dtype=torch.uint8, device="cuda")
        e.mask = torch.ones(NCH * (ROWS - K + 1), dtype=torch.uint8, device="cuda")
        with m.stream() as e.stream, m.stream_bank(NCH) as e.bank, m.power_gate(NCH, n_frames=K) as e.gate:
            torch.cuda.synchronize()
            yield e


def still_right(e):
    """Nothing was enqueued, nothing was left switched: the handle computes what it computed before."""
    got = e.m.process(e.pcm)
    e.torch.cuda.synchronize()
    assert e.torch.equal(got, e.base)


def refused(e, exc, call):
    with pytest.raises(exc) as info:
        call()
    if exc is e.mfcc_amd.MfccHipError:
        assert info.value.code == e.mfcc_amd._lib.ERROR_INVALID_PARAM
    still_right(e)


# ---- out: (call taking the tensor, the shape it wants, its dtype, another dtype); every refusal is a ValueError
SAMPLE_OFFS = [0, NS, NCH * NS]
OUT_CALLS = {
    "process": (lambda e, o: e.m.process(e.pcm, out=o), (NCH, NF, W), "float32", "float16"),
    "process_fixed": (lambda e, o: e.m.process_fixed(e.pcm, out=o), (NCH, NF, W), "int16", "int32"),
    "process_packed": (lambda e, o: e.m.process_packed(e.flat, SAMPLE_OFFS, out=o), (NCH * NF, W), "float32", "float64"),
    "vad_rows": (lambda e, o: e.m.vad_rows(e.rows_f, out=o), (NCH, ROWS), "uint8", "int8"),
    "select_rows": (lambda e, o: e.m.select_rows(e.rows_f, e.voiced, out=o), (NCH * ROWS, W), "float32", "float16"),
    "deltas_rows": (lambda e, o: e.m.deltas_rows(e.rows_f, out=o), (NCH, ROWS, 3 * W), "float32", "float64"),
    "normalize_rows_sliding": (lambda e, o: e.m.normalize_rows(e.rows_f, window=4, min_window=1, out=o),
                               (NCH, ROWS, W), "float32", "float16"),
    "bank_push_packed": (lambda e, o: e.bank.push_packed(e.flat, SAMPLE_OFFS, out=o), (NCH * NF, W), "float32", "int16"),
    "gate_windows": (lambda e, o: e.m.gate_windows(e.rows_i, e.mask, n_frames=K, out=o), (NCH * (ROWS - K + 1), K, W),
                     "int16", "float32"),
}


def bad_out(torch, kind, shape, dtype, other):
    if kind == "dtype":
        return torch.empty(shape, dtype=getattr(torch, other), device="cuda")
    if kind == "shape":
        return torch.empty(shape[:-1] + (shape[-1] + 1,), dtype=getattr(torch, dtype), device="cuda")
    o = torch.empty(shape[:-1] + (2 * shape[-1],), dtype=getattr(torch, dtype), device="cuda")[..., ::2]
    assert tuple(o.shape) == shape and not o.is_contiguous()
    return o


@pytest.mark.parametrize("kind", ["dtype", "shape", "strided"])
@pytest.mark.parametrize("name", list(OUT_CALLS))
def test_out_refused(env, name, kind):
    call, shape, dtype, other = OUT_CALLS[name]
    o = bad_out(env.torch, kind, shape, dtype, other)
    refused(env, ValueError, lambda: call(env, o))


# ---- offsets: (call taking them, valid offsets, whether their count is fixed, whether an end is checked, what a
# decreasing list raises: "hip" is MfccHipError(INVALID_PARAM) from the library's own check)
ROW_OFFS = [0, ROWS, NCH * ROWS]
OFFSET_CALLS = {
    "process_packed": (lambda e, fo: e.m.process_packed(e.flat, fo), SAMPLE_OFFS, False, True, "value"),
    "vad_rows": (lambda e, fo: e.m.vad_rows(e.rows_f, fo), ROW_OFFS, False, True, "hip"),
    "select_rows": (lambda e, fo: e.m.select_rows(e.rows_f, e.voiced, fo), ROW_OFFS, False, True, "hip"),
    "deltas_rows": (lambda e, fo: e.m.deltas_rows(e.rows_f, fo), ROW_OFFS, False, True, "hip"),
    "normalize_rows": (lambda e, fo: e.m.normalize_rows(e.rows_f, fo), ROW_OFFS, False, True, "hip"),
    "normalize_rows_sliding": (lambda e, fo: e.m.normalize_rows(e.rows_f, fo, window=4, min_window=1), ROW_OFFS, False,
                               True, "hip"),
    "pcen_rows": (lambda e, fo: e.m.pcen_rows(e.rows_f, fo), ROW_OFFS, False, True, "hip"),
    "bank_push_packed": (lambda e, fo: e.bank.push_packed(e.flat, fo), SAMPLE_OFFS, True, True, "value"),
    "gate_rows": (lambda e, fo: e.m.gate_rows(e.rows_i, fo, n_frames=K), ROW_OFFS, False, True, "value"),
    "gate_windows": (lambda e, fo: e.m.gate_windows(e.rows_i, e.mask, fo, n_frames=K), ROW_OFFS, False, True, "value"),
    "gate_push": (lambda e, fo: e.gate.push(e.rows_i.reshape(-1, W), fo), ROW_OFFS, True, True, "value"),
    "gate_num_windows": (lambda e, fo: e.gate.num_windows(fo), ROW_OFFS, True, False, "value"),
}
OFFSET_CASES = [(name, kind) for name, c in OFFSET_CALLS.items() for kind in ["2d", "empty", "count", "past", "decreasing"]
                if (kind != "count" or c[2]) and (kind != "past" or c[3])]


@pytest.mark.parametrize("name,kind", OFFSET_CASES, ids=["%s-%s" % c for c in OFFSET_CASES])
def test_offsets_refused(env, name, kind):
    call, good, _, _, decreasing = OFFSET_CALLS[name]
    exc = ValueError
    if kind == "2d":
        fo = np.array(good, dtype=np.uint64)[:, None]
    elif kind == "empty":
        fo = np.zeros(0, dtype=np.uint64)
    elif kind == "count":
        fo = np.array(good[:-1], dtype=np.uint64)
    elif kind == "past":
        fo = np.array(good[:-1] + [good[-1] + 1], dtype=np.uint64)
    else:
        fo = np.array([good[0], good[2], good[1]], dtype=np.uint64)          # the last entry still lies inside
        exc = env.mfcc_amd.MfccHipError if decreasing == "hip" else ValueError
    refused(env, exc, lambda: call(env, fo))


def test_segment_offsets_accepted(env):
    """A segment pass takes its offsets as a list, a NumPy array of another integer type or a torch CPU tensor alike;
    one entry is no segment, wherever it points: nothing is read, nothing is written."""
    e, torch = env, env.torch
    want = e.m.deltas_rows(e.rows_f, np.array(ROW_OFFS, dtype=np.uint64))
    for fo in (ROW_OFFS, tuple(ROW_OFFS), np.array(ROW_OFFS, dtype=np.int32), torch.tensor(ROW_OFFS)):
        assert torch.equal(e.m.deltas_rows(e.rows_f, fo), want)
        assert torch.equal(e.m.vad_rows(e.rows_f, fo), e.m.vad_rows(e.rows_f))
    for fo in ([99], torch.tensor([99])):
        rows = e.rows_f.clone()
        assert e.m.normalize_rows(rows, fo) is rows and torch.equal(rows, e.rows_f)
        assert e.m.pcen_rows(rows, fo) is rows and torch.equal(rows, e.rows_f)
        got, oo = e.m.select_rows(e.rows_f, e.voiced, fo)
        assert tuple(got.shape) == (0, W) and np.array_equal(oo, [0])
    still_right(e)


# ---- host sample arrays: a float32 array on an int16 handle, and one dimension too many
def test_samples_refused(env):
    e = env
    refused(e, TypeError, lambda: e.m.process(e.pcm_np.astype(np.float32)))
    refused(e, ValueError, lambda: e.m.process(e.pcm_np[None]))                          # (1, channels, n)
    refused(e, TypeError, lambda: e.stream.push(e.pcm_np[0].astype(np.float32)))
    refused(e, TypeError, lambda: e.stream.push(e.pcm_np))
    chunks = [e.pcm_np[0], e.pcm_np[1]]
    refused(e, TypeError, lambda: e.bank.push([c.astype(np.float32) for c in chunks]))
    refused(e, TypeError, lambda: e.bank.push([chunks[0], e.pcm_np]))
    assert e.stream.pending == 0 and not e.bank.pending.any()                            # nothing was taken in


def test_handle_on_another_gpu(env):
    """A handle of GPU 1 while GPU 0 is current: what the gate copies in and what it allocates lives on GPU 1."""
    torch, mfcc_amd = env.torch, env.mfcc_amd
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    assert torch.cuda.current_device() == 0
    rows = env.rows_i.cpu().numpy()
    ref = env.m.gate_rows(rows, n_frames=K)
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13, device=1) as m1:
        got = m1.gate_rows(rows, n_frames=K)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
        with m1.power_gate(NCH, n_frames=K) as g:
            pushed = g.push(rows.reshape(-1, W), ROW_OFFS)
            for a, b in zip(pushed, ref):
                assert np.array_equal(a, b)
            last = g.last_windows(None)
            assert last.device == torch.device("cuda", 1)
            torch.cuda.synchronize(1)
            assert np.array_equal(last.cpu().numpy(), rows[:, ROWS - K:])
    assert torch.cuda.current_device() == 0
