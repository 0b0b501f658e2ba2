"""Host side of the stream bank (mfcc_hip_bank_*): the plan of a push is lengths only and needs no GPU -- it is held
against a model of N independent sessions written here; argument checks, the ctypes prototypes and the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mfcc_amd
from mfcc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANK = ["mfcc_hip_bank_create", "mfcc_hip_bank_destroy", "mfcc_hip_bank_size", "mfcc_hip_bank_pending",
        "mfcc_hip_bank_plan", "mfcc_hip_bank_push", "mfcc_hip_bank_push_dev", "mfcc_hip_bank_flush",
        "mfcc_hip_bank_reset"]


class Session:
    """One online session as the core's framer sees it (frame.py:65-153): samples queue up; whenever nfft of them are
    there a frame leaves and the queue moves on by one hop."""

    def __init__(self, nfft, hop):
        self.nfft, self.hop, self.queued = nfft, hop, 0

    def push(self, n):
        frames = 0
        self.queued += n
        while self.queued >= self.nfft:
            frames += 1
            self.queued -= self.hop
        return frames


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _plan(p, pending, offsets, with_after=True):
    n = len(pending)
    fo = np.full(n + 1, 12345, dtype=np.uint64)
    after = np.full(n, 12345, dtype=np.uint64)
    rc = L.load().mfcc_hip_bank_plan(C.byref(p), _ptr(pending), _ptr(offsets), n, _ptr(fo),
                                     _ptr(after) if with_after else None)
    return rc, fo, after


@pytest.mark.parametrize("nfft,hop", [(512, 170), (1024, 341), (128, 1), (256, 256), (512, 257)])
def test_plan_equals_n_independent_sessions(nfft, hop):
    p = mfcc_amd.make_params(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    rng = np.random.default_rng(nfft * 1000 + hop)
    n = 7
    sessions = [Session(nfft, hop) for _ in range(n)]
    pending = np.zeros(n, dtype=np.uint64)
    sizes = [0, 1, 2, 7, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, 3 * nfft + 5]
    for rnd in range(200):
        lens = rng.choice(sizes, n)
        if rnd % 17 == 0:
            lens[rng.integers(n)] = int(rng.integers(0, 5 * nfft))
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[0] = int(rng.integers(0, 100))                 # the chunks need not start at sample 0 of the buffer
        offsets[1:] = offsets[0] + np.cumsum(lens).astype(np.uint64)
        rc, fo, after = _plan(p, pending, offsets)
        assert rc == L.SUCCESS
        frames = [s.push(int(k)) for s, k in zip(sessions, lens)]
        assert fo[0] == 0 and np.array_equal(np.diff(fo.astype(np.int64)), frames), (rnd, lens)
        assert np.array_equal(after, [s.queued for s in sessions]), (rnd, lens)
        assert int(after.max()) < nfft
        rc2, fo2, _ = _plan(p, pending, offsets, with_after=False)          # pending_after may be NULL
        assert rc2 == L.SUCCESS and np.array_equal(fo2, fo)
        pending = after


def test_plan_refuses_decreasing_offsets_and_bad_pending():
    p = mfcc_amd.make_params()
    pending = np.zeros(3, dtype=np.uint64)
    rc, fo, _ = _plan(p, pending, np.array([0, 600, 500, 900], dtype=np.uint64))
    assert rc == L.ERROR_INVALID_PARAM
    assert fo[0] == 0 and fo[1] == 1                    # filled up to the offending stream
    rc, _, _ = _plan(p, np.array([0, 512, 0], dtype=np.uint64), np.array([0, 1, 2, 3], dtype=np.uint64))
    assert rc == L.ERROR_INVALID_PARAM                  # a session never holds a whole frame back
    bad = mfcc_amd.make_params(nfft=500)
    rc, _, _ = _plan(bad, pending, np.array([0, 1, 2, 3], dtype=np.uint64))
    assert rc == L.ERROR_INVALID_PARAM


def test_null_arguments_are_refused():
    lib = L.load()
    p = mfcc_amd.make_params()
    a = np.zeros(4, dtype=np.uint64)
    out = C.c_void_p()
    nf = C.c_size_t(0)
    inv = L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_bank_create(None, 0, 4, C.byref(out)) == inv and not out.value
    lib.mfcc_hip_bank_destroy(None)
    assert lib.mfcc_hip_bank_size(None) == 0
    assert lib.mfcc_hip_bank_pending(None, _ptr(a)) == inv
    assert lib.mfcc_hip_bank_plan(None, _ptr(a), _ptr(a), 3, _ptr(a), None) == inv
    assert lib.mfcc_hip_bank_plan(C.byref(p), None, _ptr(a), 3, _ptr(a), None) == inv
    assert lib.mfcc_hip_bank_plan(C.byref(p), _ptr(a), None, 3, _ptr(a), None) == inv
    assert lib.mfcc_hip_bank_plan(C.byref(p), _ptr(a), _ptr(a), 3, None, None) == inv
    assert lib.mfcc_hip_bank_push(None, _ptr(a), _ptr(a), _ptr(a), 4, _ptr(a)) == inv
    assert lib.mfcc_hip_bank_push_dev(None, _ptr(a), _ptr(a), _ptr(a), 4, _ptr(a)) == inv
    assert lib.mfcc_hip_bank_flush(None, None, 0, _ptr(a), 4, C.byref(nf)) == inv
    assert lib.mfcc_hip_bank_reset(None, None, 0) == inv


def test_prototypes_and_header():
    for name in BANK:
        assert name in L.SYMBOLS, name
        assert hasattr(L.load(), name), name
    assert L.SYMBOLS["mfcc_hip_bank_size"][0] is C.c_size_t and L.SYMBOLS["mfcc_hip_bank_destroy"][0] is None
    src = open(os.path.join(ROOT, "include", "mfcc_hip.h")).read()
    assert "#define MFCC_HIP_ABI_VERSION 2" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in BANK:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "typedef struct mfcc_hip_bank mfcc_hip_bank;" in code
    assert hasattr(mfcc_amd, "MfccStreamBank") and hasattr(mfcc_amd.MFCC, "stream_bank")
