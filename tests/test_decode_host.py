"""CPU-side checks of the sample formats (``enum mfcc_hip_sample_format``, ``mfcc_hip_decode_host``,
``MFCC(sample_format=...)``): every rule of include/mfcc_hip.h, bit for bit, against tests/decode_ref.py, whose G.711 tables
are pinned to the standard by literal anchors.  No GPU needed; tests/test_gpu_decode.py holds the kernel to
``mfcc_hip_decode_host``."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import decode_ref as dr
import mfcc_amd
from mfcc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(x, fmt):
    """mfcc_hip_decode_host through the package, and the raw call's return code checked."""
    return mfcc_amd.decode(np.asarray(x, dtype=dr.DTYPES[fmt]), fmt)


def test_enum_values_match_the_binding():
    assert [getattr(L, "SAMPLE_" + f.upper()) for f in dr.FORMATS] == list(range(7))
    src = open(os.path.join(ROOT, "include", "mfcc_hip.h")).read()
    for f in dr.FORMATS:
        assert re.search(r"MFCC_HIP_SAMPLE_%s\s*=\s*%d\b" % (f.upper(), dr.CODES[f]), src), f
    assert "enum mfcc_hip_sample_format" in src
    assert "#define MFCC_HIP_ABI_VERSION 2" in src
    assert "i2s_mic.py:62" in src                       # the I2S rule cites the reference's line


@pytest.mark.parametrize("fmt", ["ulaw", "alaw", "u8"])
def test_all_256_codes(fmt):
    codes = np.arange(256, dtype=np.uint8)
    got = host(codes, fmt)
    assert got.dtype == np.int16 and np.array_equal(got, dr.decode(codes, fmt))


def test_g711_anchors():
    """Literal values of ITU-T G.711: they pin decode_ref to the standard, not to the library."""
    u = dr.decode(np.arange(256, dtype=np.uint8), "ulaw")
    assert (u[0x00], u[0x80], u[0x7f], u[0xff]) == (-32124, 32124, 0, 0)
    a = dr.decode(np.arange(256, dtype=np.uint8), "alaw")
    assert (a[0x55], a[0xd5], a[0x2a], a[0xaa]) == (-8, 8, -32256, 32256)
    # ... and the library agrees with the literals directly
    assert host([0x00, 0x80, 0x7f, 0xff], "ulaw").tolist() == [-32124, 32124, 0, 0]
    assert host([0x55, 0xd5, 0x2a, 0xaa], "alaw").tolist() == [-8, 8, -32256, 32256]


@pytest.mark.parametrize("fmt", ["ulaw", "alaw"])
def test_g711_tables_are_odd_symmetric_and_monotone(fmt):
    b = np.arange(256)
    t = host(b, fmt).astype(np.int64)
    assert np.array_equal(t[b ^ 0x80], -t)
    # per sign, ordered by the magnitude code (mu-law sends the complement, A-law toggles the even bits)
    for sign in (0, 0x80):
        if fmt == "ulaw":
            codes = [(~(sign | m)) & 0xff for m in range(128)]
        else:
            codes = [(sign | m) ^ 0x55 for m in range(128)]
        mag = np.abs(t[codes])
        assert np.all(np.diff(mag) > 0), (fmt, sign)
        assert len(set(np.sign(t[codes][1:]))) == 1         # mu-law's smallest magnitude is 0 for both signs


WORDS = [0, 1 << 10, (1 << 10) - 1, 0x7fffffff, 0x80000000, 0xffffffff, 1 << 25, 1 << 26]


@pytest.mark.parametrize("fmt", ["i2s32", "s32"])
def test_word_formats(fmt):
    w = np.array(WORDS, dtype=np.uint32).view(np.int32)
    got = host(w, fmt)
    assert np.array_equal(got, dr.decode(w, fmt))
    if fmt == "i2s32":
        # bits 25..10: 1 << 10 is the LSB, 1 << 25 the sign bit, 1 << 26 lies above the cut
        assert got.tolist() == [0, 1, 0, -1, 0, -1, -32768, 0]
    else:
        assert got.tolist() == [0, 0, 0, 32767, -32768, -1, 512, 1024]
    rng = np.random.default_rng(1)
    r = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.int32)
    assert np.array_equal(host(r, fmt), dr.decode(r, fmt))


def test_f32():
    e = np.float32(32767.5) / np.float32(32768.0)
    x = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, e, -e], dtype=np.float32)
    got = host(x, "f32")
    assert np.array_equal(got, dr.decode(x, "f32"))
    assert got.tolist() == [0, 0, 32767, -32768, 32767, -32768, 32767, -32768]
    ties = np.array([(k + 0.5) / 32768.0 for k in range(-3, 4)], dtype=np.float32)      # exact in fp32
    assert np.array_equal(ties * np.float32(32768.0), np.arange(-3, 4) + 0.5)
    got = host(ties, "f32")
    assert got.tolist() == [-2, -2, 0, 0, 2, 2, 4]                                        # to even
    assert np.array_equal(got, dr.decode(ties, "f32"))
    odd = np.array([0.99999, -1.00001, np.inf, -np.inf, np.nan, np.float32(1e-45)], dtype=np.float32)
    got = host(odd, "f32")
    assert np.array_equal(got, dr.decode(odd, "f32"))
    assert got.tolist() == [32767, -32768, 32767, -32768, 0, 0]
    r = np.random.default_rng(2).uniform(-1.2, 1.2, size=4096).astype(np.float32)
    assert np.array_equal(host(r, "f32"), dr.decode(r, "f32"))


def test_s16_is_the_identity():
    x = np.random.default_rng(3).integers(-32768, 32768, size=1000).astype(np.int16)
    assert np.array_equal(host(x, "s16"), x)


def test_sample_size():
    lib = L.load()
    assert [lib.mfcc_hip_sample_size(dr.CODES[f]) for f in dr.FORMATS] == [2, 1, 1, 1, 4, 4, 4]
    assert [dr.SIZES[f] for f in dr.FORMATS] == [2, 1, 1, 1, 4, 4, 4]
    for bad in (-1, 7, 100):
        assert lib.mfcc_hip_sample_size(bad) == 0


def test_decode_host_refusals():
    lib = L.load()
    x = np.zeros(8, dtype=np.uint8)
    out = np.full(8, 77, dtype=np.int16)
    for bad in (-1, 7):
        assert lib.mfcc_hip_decode_host(bad, x.ctypes.data, 8, out.ctypes.data) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_decode_host(L.SAMPLE_ULAW, None, 8, out.ctypes.data) == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_decode_host(L.SAMPLE_ULAW, x.ctypes.data, 8, None) == L.ERROR_INVALID_PARAM
    assert np.all(out == 77)
    assert lib.mfcc_hip_decode_host(L.SAMPLE_ULAW, None, 0, None) == L.SUCCESS
    # an unaligned word pointer is fine on the host
    raw = np.zeros(4 * 5 + 1, dtype=np.uint8)
    words = np.array([1 << 26, -1, 5 << 16, 1 << 25, 0], dtype=np.int32)
    raw[1:] = words.view(np.uint8)
    out = np.zeros(5, dtype=np.int16)
    assert lib.mfcc_hip_decode_host(L.SAMPLE_S32, raw.ctypes.data + 1, 5, out.ctypes.data) == L.SUCCESS
    assert np.array_equal(out, dr.decode(words, "s32"))
    with pytest.raises(TypeError):
        mfcc_amd.decode(np.zeros(4, np.int16), "ulaw")
    with pytest.raises(ValueError):
        mfcc_amd.decode(np.zeros(4, np.uint8), "mp3")


def test_unknown_format_and_wrong_dtype_raise_in_python():
    with pytest.raises(ValueError):
        mfcc_amd.MFCC(nfilters=32, nceptrums=13, sample_format="mp3")
    import torch
    if torch.cuda.is_available():
        m = mfcc_amd.MFCC(nfilters=32, nceptrums=13, sample_format="ulaw")
    else:
        # no handle can be made here: what the constructor sets before it asks for the device
        m = mfcc_amd.MFCC.__new__(mfcc_amd.MFCC)
        m.sample_format = "ulaw"
    # the dtype is checked before the library is asked for anything
    with pytest.raises(TypeError):
        m.process(np.zeros(600, np.int16))
    with pytest.raises(TypeError):
        m.process_fixed(np.zeros(600, np.float32))
    with pytest.raises(TypeError):
        m.process_batch([np.zeros(600, np.int16)])
    m.close()
    assert mfcc_amd.MFCC.sample_format == "s16"


def test_decode_grid_rule():
    """mfcc_fc::decode_grid (launch_geom.hpp has no HIP in it): at most 8 workgroups per CU over both axes, never more
    than the groups need, never none -- tests/test_gpu_decode.py picks its two-trip length from these numbers."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "g.cpp")
        open(src, "w").write(
            '#include <cstdio>\n#include <cstdlib>\n#include "launch_geom.hpp"\n'
            "int main(int c, char **v) { unsigned x, y; mfcc_fc::decode_grid(atoll(v[1]), atoll(v[2]), atoi(v[3]), x, y);\n"
            ' printf("%u %u %d %d %d\\n", x, y, mfcc_fc::kDecodeThreads, mfcc_fc::kDecodeGroup, mfcc_fc::kDecodeBlocksPerCu); }\n')
        exe = os.path.join(d, "g")
        subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "mfcc_amd", "csrc"), src, "-o", exe])

        def grid(groups, rows, n_cu):
            return tuple(int(t) for t in subprocess.check_output([exe, str(groups), str(rows), str(n_cu)]).split())
        assert grid(0, 1, 256) == (1, 1, 256, 8, 8)
        assert grid(1, 1, 256)[:2] == (1, 1)
        assert grid(257, 1, 256)[:2] == (2, 1)
        assert grid(1 << 25, 1, 256)[:2] == (2048, 1)
        assert grid(1 << 25, 2, 256)[:2] == (1024, 2)
        assert grid(1 << 25, 100000, 256)[:2] == (1, 65535)
        assert grid(1 << 25, 3, 1)[:2] == (2, 3)
