"""Serial wire format of the FPGA's coefficient stream and the receiver's power gate -- the data
formats on the far side of the hot path.  Thin wrappers over the host-only
C-ABI functions of libmfcc_hip.so (include/mfcc_hip.h); names follow the reference:

  mfcc/misc/magic.py:9-41        MagicInserter: 0xa55a in front of every frame's coefficients
  software/serial.c:89-122       expect_magic: byte-wise resynchronisation, big endian
  software/cepstrum.c:15-71      cepstrum_get_column: magic, then n_cep big-endian int16
  software/cepstrum.c:161-183    cepstrum_eval_power: sum of c0^2 over the middle third >= 1e8
                                 (cepstrum_eval_power32: with the reference's own 32-bit accumulator)
"""
import ctypes as C

import numpy as np

from . import _lib

MAGIC = 0xA55A                 # magic.py:10, serial.c:13-14
POWER_THRESHOLD = 100000000    # cepstrum.c:13


def pack_columns(cep) -> bytes:
    """int16 ``(frames, n_cep)`` (what ``MFCC.process_fixed`` returns) -> the UART byte stream."""
    cep = np.ascontiguousarray(cep, dtype=np.int16)
    if cep.ndim != 2:
        raise ValueError("cep must be (frames, n_cep)")
    lib = _lib.load()
    nf, nc = cep.shape
    out = np.empty(lib.mfcc_hip_serial_packed_size(nf, nc), dtype=np.uint8)
    _lib.check(lib.mfcc_hip_serial_pack(cep.ctypes.data_as(C.c_void_p), nf, nc,
                                        out.ctypes.data_as(C.c_void_p), out.size), "serial_pack")
    return out.tobytes()


def unpack_columns(data, n_cep, max_frames=None):
    """Byte stream -> (int16 ``(frames, n_cep)``, bytes consumed); resynchronises on the magic exactly
    like ``expect_magic`` + ``cepstrum_get_column``.  Bytes after the last whole column are left for
    the next call (``data[consumed:]``)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    lib = _lib.load()
    cap = buf.size // (2 * (n_cep + 1)) + 1 if max_frames is None else int(max_frames)
    cep = np.empty((cap, n_cep), dtype=np.int16)
    nf, used = C.c_size_t(0), C.c_size_t(0)
    _lib.check(lib.mfcc_hip_serial_unpack(buf.ctypes.data_as(C.c_void_p), buf.size, int(n_cep),
                                          cep.ctypes.data_as(C.c_void_p), cap, C.byref(nf), C.byref(used)),
               "serial_unpack")
    return cep[:nf.value].copy(), int(used.value)


def cepstrum_eval_power(window, head=0):
    """``cepstrum_eval_power`` on an int16 window ``(frames, n_cep)`` stored as the reference's circular
    buffer with its oldest element at flat index ``head``.  Returns ``(power, power >= 1e8)``."""
    window = np.ascontiguousarray(window, dtype=np.int16)
    if window.ndim != 2:
        raise ValueError("window must be (frames, n_cep)")
    lib = _lib.load()
    p = C.c_longlong(0)
    rc = lib.mfcc_hip_eval_power(window.ctypes.data_as(C.c_void_p), window.shape[1], window.shape[0],
                                 int(head), C.byref(p))
    if rc < 0:
        _lib.check(rc, "eval_power")
    return int(p.value), bool(rc)


def cepstrum_eval_power32(window, head=0):
    """:func:`cepstrum_eval_power` with the reference's own accumulator, a 32-bit ``int`` that wraps (what gcc on x86-64
    makes of the loop): returns ``(power32, power32 >= 1e8)`` -- the decision a receiver built from the reference takes.
    Two coefficients of -32768 give ``(-2**31, False)`` where the 64-bit sum passes."""
    window = np.ascontiguousarray(window, dtype=np.int16)
    if window.ndim != 2:
        raise ValueError("window must be (frames, n_cep)")
    lib = _lib.load()
    p = C.c_int32(0)
    rc = lib.mfcc_hip_eval_power32(window.ctypes.data_as(C.c_void_p), window.shape[1], window.shape[0],
                                   int(head), C.byref(p))
    if rc < 0:
        _lib.check(rc, "eval_power32")
    return int(p.value), bool(rc)


def gate_args(n_frames=93, stride=1, threshold=POWER_THRESHOLD, n_cep=None):
    """``(n_frames, stride, threshold)`` as ints for the gate entry points, or ValueError: ``n_frames`` and ``stride``
    1..4096 (MFCC_HIP_MAX_GATE_WINDOW), ``threshold`` an int in 0..2**63 - 1, ``n_cep`` (when given) 1..64."""
    def is_int(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not is_int(n_frames) or not 1 <= int(n_frames) <= _lib.MAX_GATE_WINDOW:
        raise ValueError("n_frames must be 1..%d, not %r" % (_lib.MAX_GATE_WINDOW, n_frames))
    if not is_int(stride) or not 1 <= int(stride) <= _lib.MAX_GATE_WINDOW:
        raise ValueError("stride must be 1..%d, not %r" % (_lib.MAX_GATE_WINDOW, stride))
    if not is_int(threshold) or not 0 <= int(threshold) < 2 ** 63:
        raise ValueError("threshold must be an int in 0..2**63 - 1, not %r" % (threshold,))
    if n_cep is not None and (not is_int(n_cep) or not 1 <= int(n_cep) <= 64):
        raise ValueError("n_cep must be 1..64, not %r" % (n_cep,))
    return int(n_frames), int(stride), int(threshold)


def gate_count(lengths_or_offsets, n_frames=93, stride=1, offsets=False):
    """Window offsets of segments (host only, ``mfcc_hip_gate_count``): a segment of ``T`` rows has
    ``(T - n_frames) // stride + 1`` windows (0 when ``T < n_frames``).  ``lengths_or_offsets``: the row count of every
    segment, or with ``offsets=True`` the ``n_segments + 1`` row offsets (what ``process_packed`` returns).  Returns the
    running sum, uint64 ``(n_segments + 1,)``: the global window index the gate's outputs are indexed by."""
    n_frames, stride, _ = gate_args(n_frames, stride)
    a = np.asarray(lengths_or_offsets)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu") or (a.size and int(a.min()) < 0):
        raise ValueError("lengths / offsets must be a 1-D array of non-negative ints")
    if offsets:
        if a.size < 1:
            raise ValueError("offsets need n_segments + 1 entries")
        off = np.ascontiguousarray(a, dtype=np.uint64)
    else:
        off = np.zeros(a.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum(a, dtype=np.uint64)
    wo = np.zeros(len(off), dtype=np.uint64)
    _lib.check(_lib.load().mfcc_hip_gate_count(n_frames, stride, off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                               wo.ctypes.data_as(C.c_void_p)), "gate_count")
    return wo
