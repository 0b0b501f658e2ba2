"""CPU-side checks of the power gate: the reference model against answers worked by hand and against the receiver's
literal loop, the host-only entry points (mfcc_hip_eval_power32, mfcc_hip_gate_count, mfcc_hip_gate_plan) against the
model, the argument checks that need no GPU and the Python validators."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mfcc_amd
from mfcc_amd import _lib as L
from mfcc_amd import wire

import gate_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfcc_hip_eval_power32", "mfcc_hip_gate_count", "mfcc_hip_gate_dev", "mfcc_hip_gate_windows_dev",
       "mfcc_hip_gate_create", "mfcc_hip_gate_destroy", "mfcc_hip_gate_seen", "mfcc_hip_gate_plan",
       "mfcc_hip_gate_push_dev", "mfcc_hip_gate_reset", "mfcc_hip_gate_window_dev"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_every_new_declaration_is_declared_exported_and_typed():
    src = open(os.path.join(ROOT, "include", "mfcc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mfcc_hip_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS, name
    assert re.search(r"#define\s+MFCC_HIP_MAX_GATE_WINDOW\s+4096\b", src)
    assert re.search(r"#define\s+MFCC_HIP_POWER_THRESHOLD\s+100000000", src)
    assert L.MAX_GATE_WINDOW == 4096 and L.POWER_THRESHOLD == wire.POWER_THRESHOLD == gr.POWER_THRESHOLD == 10 ** 8
    assert L.load().mfcc_hip_abi_version() == 2            # unchanged


def test_hand_worked_geometry():
    # 5 cep x 4 frames: size 20, first 6, last 13 -> elements 6 and 11: column 1 of frames 1 and 2
    assert gr.loop_elements(5, 4) == [6, 11]
    assert gr.geometry(5, 4) == (2, 1, 1)
    rows = np.arange(20, dtype=np.int16).reshape(4, 5) * 100
    p, g, r, wo = gr.gate(rows, [0, 4], 4, 1)
    assert list(wo) == [0, 1] and p[0] == 600 ** 2 + 1100 ** 2 and g[0] == 0 and r[0] == 0
    # 1 x 1: first = last = 0: nothing is summed; the gate opens only at threshold 0
    assert gr.loop_elements(1, 1) == [] and gr.geometry(1, 1) == (0, 0, 0)
    one = np.full((3, 1), -32768, np.int16)
    p, g, r, wo = gr.gate(one, [0, 3], 1, 1)
    assert list(wo) == [0, 3] and not p.any() and not g.any() and not r.any()
    p, g, r, _ = gr.gate(one, [0, 3], 1, 1, threshold=0)
    assert g.all() and r.all()
    # the reference's 16 x 93: column 0 of frames 31 .. 61
    assert gr.geometry(16, 93) == (31, 31, 0)
    assert gr.loop_elements(16, 93) == [16 * f for f in range(31, 62)]


def test_geometry_is_the_literal_loop():
    """(K, f0, c0) against the receiver's loop for every n_cep 1..64 x n_frames 1..200; c0 is not 0 in general."""
    off_column = 0
    for n_cep in range(1, 65):
        for n_frames in range(1, 201):
            el = gr.loop_elements(n_cep, n_frames)
            K, f0, c0 = gr.geometry(n_cep, n_frames)
            assert el == [(f0 + k) * n_cep + c0 for k in range(K)], (n_cep, n_frames)
            assert K == 0 or f0 + K <= n_frames, (n_cep, n_frames)
            off_column += c0 != 0
    assert off_column > 64 * 200 // 3
    K, f0, c0 = gr.geometry(3, 4096)
    assert K == 1366                                        # the most any shape sums


def _circular(rows, head_frames):
    """rows (frames, n_cep) stored as the receiver's circular buffer with its oldest frame at frame head_frames."""
    return np.roll(rows, head_frames, axis=0), head_frames * rows.shape[1]


def test_eval_power32_is_the_32_bit_accumulator():
    lib = L.load()
    rng = np.random.default_rng(11)
    for n_cep, n_frames in [(16, 93), (5, 4), (13, 93), (1, 1), (2, 7), (64, 3)]:
        for trial in range(6):
            rows = rng.integers(-32768, 32768, (n_frames, n_cep)).astype(np.int16)
            if trial & 1:
                rows[rng.integers(0, n_frames, max(1, n_frames // 2))] = -32768
            ref, _, _, _ = gr.gate(rows, [0, n_frames], n_frames, 1)
            want = int(gr.wrap32(ref)[0])
            for hf in (0, 1 % n_frames, n_frames // 2, n_frames - 1):
                buf, head = _circular(rows, hf)
                assert wire.cepstrum_eval_power(buf, head) == (int(ref[0]), int(ref[0]) >= 10 ** 8)
                assert wire.cepstrum_eval_power32(buf, head) == (want, want >= 10 ** 8), (n_cep, n_frames, hf)
    # 3 cep x 6 frames: size 18, elements 6, 9 -> column 0 of frames 2 and 3; 3 x 12: frames 4 .. 7; 3 x 15: frames 5 .. 9
    def window(n_frames, values):
        K, f0, c0 = gr.geometry(3, n_frames)
        assert c0 == 0 and K == len(values)
        w = np.zeros((n_frames, 3), np.int16)
        w[f0:f0 + K, 0] = values
        return _circular(w, n_frames - 1)                   # head != 0
    buf, head = window(6, [-32768, -32768])                 # 2^31: passes in 64 bits, -2^31 in 32
    assert wire.cepstrum_eval_power(buf, head) == (2 ** 31, True)
    assert wire.cepstrum_eval_power32(buf, head) == (-2 ** 31, False)
    buf, head = window(12, [-32768] * 4)                    # 2^32: 0 in 32 bits
    assert wire.cepstrum_eval_power(buf, head) == (2 ** 32, True)
    assert wire.cepstrum_eval_power32(buf, head) == (0, False)
    buf, head = window(15, [-32768] * 4 + [10000])          # 2^32 + 1e8: exactly the threshold in 32 bits
    assert wire.cepstrum_eval_power(buf, head) == (2 ** 32 + 10 ** 8, True)
    assert wire.cepstrum_eval_power32(buf, head) == (10 ** 8, True)
    # bad arguments
    p = C.c_int32(0)
    w = np.zeros(4, np.int16)
    assert lib.mfcc_hip_eval_power32(None, 2, 2, 0, C.byref(p)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_eval_power32(_p(w), 0, 2, 0, C.byref(p)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_eval_power32(_p(w), 2, 0, 0, C.byref(p)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_eval_power32(_p(w), 2, 2, 4, C.byref(p)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_eval_power32(_p(w), 2, 2, 3, None) == 0


SHAPES = [(93, 1), (93, 31), (4, 1), (1, 1), (3, 2), (1500, 7), (4096, 4096), (9, 1), (7, 10), (2, 4096)]


def _lengths(rng, n_frames, stride, extra=8):
    base = [0, n_frames - 1, n_frames, n_frames + 1, n_frames + stride]
    return np.array(base + [int(v) for v in rng.integers(0, 3 * n_frames + 4 * stride, extra)], dtype=np.uint64)


def test_gate_count_is_the_model():
    lib = L.load()
    rng = np.random.default_rng(5)
    for n_frames, stride in SHAPES:
        lens = _lengths(rng, n_frames, stride)
        rng.shuffle(lens)
        off = np.concatenate([[7], 7 + np.cumsum(lens)]).astype(np.uint64)      # rows before off[0] do not count
        wo = np.zeros(len(off), np.uint64)
        assert lib.mfcc_hip_gate_count(n_frames, stride, _p(off), len(lens), _p(wo)) == 0
        assert np.array_equal(wo.astype(np.int64), gr.win_offsets(off, n_frames, stride)), (n_frames, stride)
        assert np.array_equal(wire.gate_count(lens, n_frames, stride), wo)
        assert np.array_equal(wire.gate_count(off, n_frames, stride, offsets=True), wo)
        for T, want in ((n_frames - 1, 0), (n_frames, 1), (n_frames + stride - 1, 1), (n_frames + stride, 2)):
            assert int(wire.gate_count([T], n_frames, stride)[-1]) == want == gr.windows_of(T, n_frames, stride)
    one = np.zeros(1, np.uint64)
    assert lib.mfcc_hip_gate_count(93, 1, None, 0, _p(one)) == 0 and one[0] == 0
    off = np.array([0, 5, 3], np.uint64)
    wo = np.zeros(3, np.uint64)
    assert lib.mfcc_hip_gate_count(2, 1, _p(off), 2, _p(wo)) == L.ERROR_INVALID_PARAM        # decreasing
    for nf, st in ((0, 1), (4097, 1), (1, 0), (1, 4097), (-1, 1)):
        assert lib.mfcc_hip_gate_count(nf, st, _p(off), 1, _p(wo)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_count(2, 1, None, 1, _p(wo)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_count(2, 1, _p(off), 1, None) == L.ERROR_INVALID_PARAM


def test_gate_plan_is_the_model():
    lib = L.load()
    rng = np.random.default_rng(6)
    for n_frames, stride in SHAPES:
        n = 13
        model = gr.Tracker(n, 1, n_frames, stride)
        for step in range(5):
            lens = _lengths(rng, n_frames, stride)
            rng.shuffle(lens)
            lens = lens[:n]
            if step == 1:
                lens[:] = 1                                 # one row per push
            seen = model.seen.astype(np.uint64)
            fo = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.uint64)
            wo, after = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64)
            assert lib.mfcc_hip_gate_plan(n_frames, stride, _p(seen), _p(fo), n, _p(wo), _p(after)) == 0
            assert np.array_equal(wo.astype(np.int64), model.plan(lens)), (n_frames, stride, step)
            assert np.array_equal(after, seen + lens)
            wo2 = np.zeros(n + 1, np.uint64)
            assert lib.mfcc_hip_gate_plan(n_frames, stride, _p(seen), _p(fo), n, _p(wo2), None) == 0
            assert np.array_equal(wo, wo2)
            model.push([np.zeros((int(v), 1), np.int16) for v in lens])
        # all pushes together complete the windows of the whole sequence
        total = model.seen
        assert all(gr.windows_of(int(t), n_frames, stride) >= 0 for t in total)
    seen, fo, wo = np.zeros(2, np.uint64), np.array([0, 4, 2], np.uint64), np.zeros(3, np.uint64)
    assert lib.mfcc_hip_gate_plan(2, 1, _p(seen), _p(fo), 2, _p(wo), None) == L.ERROR_INVALID_PARAM       # decreasing
    for nf, st in ((0, 1), (4097, 1), (1, 0), (1, 4097)):
        assert lib.mfcc_hip_gate_plan(nf, st, _p(seen), _p(fo), 1, _p(wo), None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_plan(2, 1, None, _p(fo), 1, _p(wo), None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_plan(2, 1, _p(seen), None, 1, _p(wo), None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_plan(2, 1, _p(seen), _p(fo), 1, None, None) == L.ERROR_INVALID_PARAM


def test_plan_chunking_sums_to_the_one_shot_count():
    rng = np.random.default_rng(8)
    for n_frames, stride in SHAPES[:9]:
        T = int(rng.integers(n_frames, 3 * n_frames + 5 * stride))
        model = gr.Tracker(1, 1, n_frames, stride)
        done, left = 0, T
        while left:
            c = int(min(left, rng.integers(0, n_frames + stride + 2)))
            done += int(model.plan([c])[-1])
            model.push([np.zeros((c, 1), np.int16)])
            left -= c
        assert done == gr.windows_of(T, n_frames, stride)


def test_entry_points_refuse_without_a_handle():
    lib = L.load()
    off = np.array([0, 100], np.uint64)
    buf = np.zeros(64, np.uint64)
    assert lib.mfcc_hip_gate_dev(None, _p(buf), 16, _p(off), 1, 93, 1, 10 ** 8, _p(buf), None, None) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_windows_dev(None, _p(buf), 16, _p(off), 1, 93, 1, _p(buf), _p(buf), None, 1, _p(buf)) == \
        L.ERROR_INVALID_PARAM
    g = C.c_void_p()
    assert lib.mfcc_hip_gate_create(None, 4, 16, 93, 1, 10 ** 8, C.byref(g)) == L.ERROR_INVALID_PARAM and not g.value
    assert lib.mfcc_hip_gate_seen(None, _p(buf)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_push_dev(None, _p(buf), _p(off), _p(buf), None, None, 8, _p(buf)) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_reset(None, None, 0) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_gate_window_dev(None, _p(off), 1, _p(buf)) == L.ERROR_INVALID_PARAM
    lib.mfcc_hip_gate_destroy(None)                         # a no-op


def test_python_validators():
    assert wire.gate_args() == (93, 1, 10 ** 8)
    assert wire.gate_args(4096, 4096, 0, n_cep=64) == (4096, 4096, 0)
    for kw in (dict(n_frames=0), dict(n_frames=4097), dict(n_frames=93.0), dict(n_frames=True), dict(stride=0),
               dict(stride=4097), dict(stride=None), dict(threshold=-1), dict(threshold=2 ** 63), dict(threshold=1e8),
               dict(n_cep=0), dict(n_cep=65), dict(n_cep=1.5)):
        with pytest.raises(ValueError):
            wire.gate_args(**kw)
    with pytest.raises(ValueError):
        wire.gate_count([[1, 2]], 93, 1)
    with pytest.raises(ValueError):
        wire.gate_count([1.5], 93, 1)
    with pytest.raises(ValueError):
        wire.gate_count([-1], 93, 1)
    with pytest.raises(ValueError):
        wire.gate_count([], 93, 1, offsets=True)
    with pytest.raises(mfcc_amd.MfccHipError):
        wire.gate_count([5, 3], 2, 1, offsets=True)         # decreasing offsets: the library's refusal
    assert list(wire.gate_count([], 93, 1)) == [0]
    with pytest.raises(ValueError):
        wire.cepstrum_eval_power32(np.zeros(4, np.int16))
    assert hasattr(mfcc_amd, "MfccPowerGate") and hasattr(mfcc_amd.MFCC, "gate_rows") and \
        hasattr(mfcc_amd.MFCC, "gate_windows") and hasattr(mfcc_amd.MFCC, "power_gate")
