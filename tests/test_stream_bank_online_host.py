"""Host side of the online stream bank (mfcc_hip_bank_create_online and its companions): the plan of a push with a lag
is lengths only and needs no GPU -- it is held against a model of N lagged sessions written here; argument checks of
the Python layer, NULL answers, the ctypes prototypes and the header."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import mfcc_amd
from mfcc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLINE = ["mfcc_hip_bank_create_online", "mfcc_hip_bank_row_width", "mfcc_hip_bank_lag", "mfcc_hip_bank_held",
          "mfcc_hip_bank_plan_online", "mfcc_hip_bank_flush_ragged"]


class LaggedSession:
    """One online session as the core's framer sees it (frame.py:65-153), behind which rows wait until ``lag`` more
    are known: a frame that leaves the framer joins the queue of finished rows, and whatever the queue holds beyond
    ``lag`` rows is returned."""

    def __init__(self, nfft, hop, lag):
        self.nfft, self.hop, self.lag, self.queued, self.held = nfft, hop, lag, 0, 0

    def push(self, n):
        returned = 0
        self.queued += n
        while self.queued >= self.nfft:
            self.queued -= self.hop
            self.held += 1
            if self.held > self.lag:
                self.held -= 1
                returned += 1
        return returned


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _plan(p, lag, pending, held, offsets, with_after=True):
    n = len(pending)
    fo = np.full(n + 1, 12345, dtype=np.uint64)
    pa = np.full(n, 12345, dtype=np.uint64)
    ha = np.full(n, 12345, dtype=np.uint64)
    rc = L.load().mfcc_hip_bank_plan_online(C.byref(p), lag, _ptr(pending), _ptr(held), _ptr(offsets), n, _ptr(fo),
                                            _ptr(pa) if with_after else None, _ptr(ha) if with_after else None)
    return rc, fo, pa, ha


def _rounds(rng, nfft, hop, n, rounds):
    sizes = [0, 1, 2, 7, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, 3 * nfft + 5]
    for rnd in range(rounds):
        lens = rng.choice(sizes, n)
        if rnd % 17 == 0:
            lens[rng.integers(n)] = int(rng.integers(0, 5 * nfft))
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[0] = int(rng.integers(0, 100))
        offsets[1:] = offsets[0] + np.cumsum(lens).astype(np.uint64)
        yield rnd, lens, offsets


@pytest.mark.parametrize("lag", [0, 1, 4, 16])
@pytest.mark.parametrize("nfft,hop", [(512, 170), (128, 1), (256, 256)])
def test_plan_online_equals_n_lagged_sessions(nfft, hop, lag):
    p = mfcc_amd.make_params(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    rng = np.random.default_rng(nfft * 1000 + hop + lag)
    n = 7
    sessions = [LaggedSession(nfft, hop, lag) for _ in range(n)]
    pending = np.zeros(n, dtype=np.uint64)
    held = np.zeros(n, dtype=np.uint64)
    for rnd, lens, offsets in _rounds(rng, nfft, hop, n, 120):
        rc, fo, pa, ha = _plan(p, lag, pending, held, offsets)
        assert rc == L.SUCCESS
        returned = [s.push(int(k)) for s, k in zip(sessions, lens)]
        assert fo[0] == 0 and np.array_equal(np.diff(fo.astype(np.int64)), returned), (rnd, lens)
        assert np.array_equal(pa, [s.queued for s in sessions]), (rnd, lens)
        assert np.array_equal(ha, [s.held for s in sessions]), (rnd, lens)
        assert int(ha.max()) <= lag and int(pa.max()) < nfft
        rc2, fo2, _, _ = _plan(p, lag, pending, held, offsets, with_after=False)      # the two may be NULL
        assert rc2 == L.SUCCESS and np.array_equal(fo2, fo)
        pending, held = pa, ha


@pytest.mark.parametrize("nfft,hop", [(512, 170), (128, 1), (256, 256)])
def test_plan_online_without_a_lag_is_the_plain_plan(nfft, hop):
    p = mfcc_amd.make_params(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    rng = np.random.default_rng(nfft + hop)
    n = 5
    pending = np.zeros(n, dtype=np.uint64)
    held = np.zeros(n, dtype=np.uint64)
    for rnd, lens, offsets in _rounds(rng, nfft, hop, n, 60):
        rc, fo, pa, ha = _plan(p, 0, pending, held, offsets)
        fo1 = np.zeros(n + 1, dtype=np.uint64)
        pa1 = np.zeros(n, dtype=np.uint64)
        rc1 = L.load().mfcc_hip_bank_plan(C.byref(p), _ptr(pending), _ptr(offsets), n, _ptr(fo1), _ptr(pa1))
        assert rc == rc1 == L.SUCCESS
        assert np.array_equal(fo, fo1) and np.array_equal(pa, pa1) and not ha.any(), rnd
        pending = pa


def test_plan_online_refusals():
    p = mfcc_amd.make_params()
    z = np.zeros(3, dtype=np.uint64)
    good = np.array([0, 600, 1200, 1800], dtype=np.uint64)
    inv = L.ERROR_INVALID_PARAM
    assert _plan(p, 4, z, z, good)[0] == L.SUCCESS
    assert _plan(p, -1, z, z, good)[0] == inv
    assert _plan(p, 4, z, np.array([0, 5, 0], dtype=np.uint64), good)[0] == inv        # held above the lag
    assert _plan(p, 4, z, z, np.array([0, 600, 500, 900], dtype=np.uint64))[0] == inv
    assert _plan(p, 4, np.array([0, 512, 0], dtype=np.uint64), z, good)[0] == inv
    assert _plan(mfcc_amd.make_params(nfft=500), 4, z, z, good)[0] == inv


def test_null_arguments_are_refused():
    lib = L.load()
    p = mfcc_amd.make_params()
    a = np.zeros(4, dtype=np.uint64)
    out = C.c_void_p()
    inv = L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_bank_create_online(None, 4, 1, 5, 0, 2, C.byref(out)) == inv and not out.value
    assert lib.mfcc_hip_bank_row_width(None) == 0
    assert lib.mfcc_hip_bank_lag(None) == 0
    assert lib.mfcc_hip_bank_held(None, _ptr(a)) == inv
    assert lib.mfcc_hip_bank_flush_ragged(None, None, 0, _ptr(a), 4, _ptr(a)) == inv
    args = [C.byref(p), 2, _ptr(a), _ptr(a), _ptr(a), 3, _ptr(a), None, None]
    assert lib.mfcc_hip_bank_plan_online(*args) == L.SUCCESS
    for k in (0, 2, 3, 4, 6):                                   # params, pending, held, offsets, frame_offsets
        bad = list(args)
        bad[k] = None
        assert lib.mfcc_hip_bank_plan_online(*bad) == inv, k


def test_python_layer_checks_its_arguments_before_the_library():
    stub = types.SimpleNamespace(_lib=L.load(), _h=None)          # never reached: every case fails in Python

    def bank(*a, **kw):
        return mfcc_amd.MfccStreamBank(stub, *a, **kw)

    with pytest.raises(ValueError, match="causal"):
        bank(2, normalize="meanvar")                              # no window: per-utterance statistics
    for kw in (dict(normalize="mean", normalize_window=5), dict(deltas=1), dict(deltas=2, delta_window=3),
               dict(normalize_window=5)):
        with pytest.raises(ValueError, match="fixed"):
            bank(2, True, **kw)
    for kw in (dict(normalize="median", normalize_window=5), dict(normalize="mean", normalize_window=0),
               dict(normalize="mean", normalize_window=L.MAX_NORMALIZE_WINDOW + 1),
               dict(normalize="mean", normalize_window=2.5), dict(deltas=3), dict(deltas=True),
               dict(deltas=1, delta_window=0), dict(deltas=1, delta_window=9)):
        with pytest.raises(ValueError):
            bank(2, **kw)
    with pytest.raises(ValueError):
        bank(0, deltas=1)
    with pytest.raises(TypeError):
        mfcc_amd.MFCC.stream_bank(stub, 2, False, "mean")          # the new settings are keyword only


def test_prototypes_and_header():
    for name in ONLINE:
        assert name in L.SYMBOLS, name
        assert hasattr(L.load(), name), name
    assert L.SYMBOLS["mfcc_hip_bank_row_width"][0] is C.c_size_t and L.SYMBOLS["mfcc_hip_bank_lag"][0] is C.c_int
    src = open(os.path.join(ROOT, "include", "mfcc_hip.h")).read()
    assert "#define MFCC_HIP_ABI_VERSION 2" in src
    assert C.sizeof(L.Params) == 64
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ONLINE:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for prop in ("num_features", "lag", "held"):
        assert isinstance(getattr(mfcc_amd.MfccStreamBank, prop), property), prop
