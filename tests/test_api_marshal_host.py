"""The marshalling helpers of ``mfcc_amd/api.py`` and ``_lib.ptr``, on the host alone: no GPU, no handle, no library
call.  The GPU suite goes through them on every call; here every refusing condition and every accepted edge of each
helper stands on its own."""
import numpy as np
import pytest
import torch

from mfcc_amd import _lib, api


def u64(*v):
    return np.array(v, dtype=np.uint64)


# ---- api._offsets
@pytest.mark.parametrize("bad, kw", [
    (u64(0, 4, 8)[:, None], {}),                        # a wrong rank
    (u64(0, 4, 8)[None, :], {}),
    (u64(), {}),                                        # too few entries
    (u64(0, 8), dict(n=2)),                             # not n + 1 entries
    (u64(0, 4, 8, 8), dict(n=2)),
    (u64(), dict(n=0)),
    (u64(0, 8, 4), {}),                                 # decreasing
    (u64(8, 0), dict(n=1)),
    (u64(0, 4, 9), dict(limit=8)),                      # the last entry beyond the limit
    (u64(0, 4, 9), dict(limit=8 * 13, unit=13, ordered=False)),
    (u64(9), dict(limit=8)),
    (u64(0, 9), dict(limit=8, limit_from=2)),
])
def test_offsets_refuses(bad, kw):
    with pytest.raises(ValueError):
        api._offsets(bad, "offsets", "rows", **kw)


def test_offsets_accepts():
    for good, kw in [(u64(0), {}), (u64(5), dict(n=0, limit=5)), (u64(3, 3, 3), {}), (u64(3, 3, 3), dict(n=2, limit=3)),
                     (u64(0, 4, 8), dict(limit=8)), (u64(0, 4, 8), dict(limit=8 * 13, unit=13)), (u64(0, 4, 8), dict(n=2))]:
        got = api._offsets(good, "offsets", "rows", **kw)
        assert got.dtype == np.uint64 and got.ndim == 1 and got.flags.c_contiguous and np.array_equal(got, good)
    for conv in ([0, 4, 8], (0, 4, 8), np.array([0, 4, 8], dtype=np.int64), np.array([0, 9, 4, 9, 8], dtype=np.int32)[::2]):
        got = api._offsets(conv, "offsets", "rows", n=2, limit=8)
        assert got.dtype == np.uint64 and got.flags.c_contiguous and np.array_equal(got, u64(0, 4, 8))
    # the segment passes leave the order to the library (it answers INVALID_PARAM): the list comes back as it is
    assert np.array_equal(api._offsets([0, 8, 4], "offsets", "rows", limit=8, ordered=False), u64(0, 8, 4))


def test_offsets_of_the_segment_passes():
    """``MFCC._segments``' parameters: the limit holds from two entries on, and is decided on the converted array, so a
    list, a tuple, a NumPy array and a torch CPU tensor are all taken alike."""
    seg = dict(limit=16 * 13, unit=13, ordered=False, limit_from=2)
    for form in (list, tuple, np.array, torch.tensor, lambda v: torch.tensor(v, dtype=torch.int32)):
        got = api._offsets(form([0, 8, 16]), "frame_offsets", "rows", **seg)
        assert got.dtype == np.uint64 and got.flags.c_contiguous and np.array_equal(got, u64(0, 8, 16))
        assert np.array_equal(api._offsets(form([99]), "frame_offsets", "rows", **seg), u64(99))     # no segment
        assert np.array_equal(api._offsets(form([0, 16, 8]), "frame_offsets", "rows", **seg), u64(0, 16, 8))
        with pytest.raises(ValueError, match="run past the end of rows"):
            api._offsets(form([0, 8, 17]), "frame_offsets", "rows", **seg)
        with pytest.raises(ValueError, match="run past the end of rows"):
            api._offsets(form([99]), "frame_offsets", "rows", limit=16 * 13, unit=13)                # everyone else's rule


# ---- offsets from shapes and lengths, the index list
def test_shape_and_length_offsets():
    for got, want in [(api._shape_offsets((8, 13)), u64(0, 8)), (api._shape_offsets((2, 8, 13)), u64(0, 8, 16)),
                      (api._shape_offsets(torch.Size((3, 0, 5))), u64(0, 0, 0, 0)),
                      (api._length_offsets([3, 0, 5]), u64(0, 3, 3, 8)), (api._length_offsets([]), u64(0)),
                      (api._length_offsets(u64(7)), u64(0, 7))]:
        assert got.dtype == np.uint64 and got.flags.c_contiguous and np.array_equal(got, want)


def test_indices():
    assert api._indices(None, 5) == (None, 5)
    for idx, want in [([], u64()), ([2, 0], u64(2, 0)), (np.array([[1], [3]]), u64(1, 3))]:
        s, n = api._indices(idx, 5)
        assert s.dtype == np.uint64 and s.flags.c_contiguous and np.array_equal(s, want) and n == len(want)


# ---- the host sample array
@pytest.mark.parametrize("fmt", list(api._SAMPLE))
def test_host_samples(fmt):
    dtype = np.dtype(api._SAMPLE[fmt][1])
    x = np.arange(24).astype(dtype).reshape(2, 12)
    assert api._host_samples(x, fmt, "pcm") is x
    row = x[0]
    assert api._host_samples(row, fmt, "pcm", ndim=1) is row                 # nothing is copied that need not be
    strided = api._host_samples(x[:, ::2], fmt, "pcm", ndim=2)
    assert strided.flags.c_contiguous and np.array_equal(strided, x[:, ::2])
    wrong = np.float64 if dtype != np.float64 else np.int16
    for other in (wrong, np.int8, np.uint16):
        with pytest.raises(TypeError, match="pcm must be"):
            api._host_samples(x.astype(other), fmt, "pcm")
    with pytest.raises(TypeError, match="chunks must be 1-D %s " % dtype.name):
        api._host_samples(x, fmt, "chunks", ndim=1)
    with pytest.raises(TypeError, match="chunks must be 2-D %s " % dtype.name):
        api._host_samples(x[0], fmt, "chunks", ndim=2)


# ---- _lib.ptr
def test_ptr():
    a = np.arange(12, dtype=np.int16)
    assert _lib.ptr(a) == a.ctypes.data and _lib.ptr(a[3:]) == a.ctypes.data + 6
    t = torch.arange(12, dtype=torch.float32)
    assert _lib.ptr(t) == t.data_ptr() and _lib.ptr(t[3:]) == t.data_ptr() + 12
    assert _lib.ptr(None) is None
    assert isinstance(_lib.ptr(a), int) and isinstance(_lib.ptr(t), int)


# ---- api._out, on CPU tensors
def test_out():
    like = torch.zeros((2, 8, 13))
    f32 = torch.float32
    made = api._out(like, None, (2, 8, 39), f32, lambda: torch.empty((2, 8, 39)))
    assert tuple(made.shape) == (2, 8, 39)
    good = torch.empty((2, 8, 39))
    assert api._out(like, good, (2, 8, 39), f32, None) is good
    for cap in (0, 5, 16):                                                  # a capacity dimension takes any size
        o = torch.empty((cap, 13))
        assert api._out(like, o, (None, 13), f32, None) is o
    for bad, want in [(torch.empty((16, 39)), (2, 8, 39)),                  # a wrong rank
                      (torch.empty((2, 8, 39, 1)), (2, 8, 39)),
                      (torch.empty((16, 13, 1)), (None, 13)),
                      (torch.empty((2, 8, 38)), (2, 8, 39)),                # one wrong dimension
                      (torch.empty((2, 9, 39)), (2, 8, 39)),
                      (torch.empty((16, 12)), (None, 13)),
                      (torch.empty((2, 8, 39), dtype=torch.float64), (2, 8, 39)),         # a wrong dtype
                      (torch.empty((16, 13), dtype=torch.int16), (None, 13)),
                      (torch.empty((2, 8, 78))[..., ::2], (2, 8, 39)),      # not contiguous
                      (torch.empty((16, 26))[:, ::2], (None, 13)),
                      (torch.empty((2, 8, 39), device="meta"), (2, 8, 39))]:  # on another device than the input
        with pytest.raises(ValueError, match="out must be a contiguous float32 tensor of shape"):
            api._out(like, bad, want, f32, None)
    with pytest.raises(ValueError, match=r"shape \(capacity, 13\) on cpu"):
        api._out(like, torch.empty((16, 12)), (None, 13), f32, None)


def test_number_checks():
    assert api._is_int(3) and api._is_int(np.int64(3)) and not api._is_int(True) and not api._is_int(3.0)
    assert api._is_f32(1) and api._is_f32(2.5) and api._is_f32(np.float32(1)) and not api._is_f32(False)
    assert not api._is_f32(float("inf")) and not api._is_f32(1e39) and not api._is_f32("1") and not api._is_f32(None)
