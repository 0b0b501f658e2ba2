"""NumPy restatement of the sample-format rules of include/mfcc_hip.h (``enum mfcc_hip_sample_format``): the reference of
tests/test_decode_host.py and tests/test_gpu_decode.py.  Integer arithmetic in int64 (nothing here comes near its range),
the one fp32 multiply of F32 in float32."""
import numpy as np

FORMATS = ("s16", "ulaw", "alaw", "u8", "i2s32", "s32", "f32")
CODES = {name: i for i, name in enumerate(FORMATS)}
DTYPES = {"s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8, "u8": np.uint8, "i2s32": np.int32, "s32": np.int32,
          "f32": np.float32}
SIZES = {"s16": 2, "ulaw": 1, "alaw": 1, "u8": 1, "i2s32": 4, "s32": 4, "f32": 4}


def ulaw(b):
    u = ~np.asarray(b, dtype=np.int64) & 0xff
    t = (((u & 0x0f) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def alaw(b):
    a = np.asarray(b, dtype=np.int64) ^ 0x55
    seg = (a & 0x70) >> 4
    t = (a & 0x0f) << 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t)


def u8(b):
    return (np.asarray(b, dtype=np.int64) - 128) << 8


def i2s32(w):
    bits = (np.asarray(w).astype(np.int64) & 0xffffffff) >> 10          # the word as uint32, shifted
    return (bits & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)


def s32(w):
    return np.asarray(w).astype(np.int64) >> 16                         # arithmetic


def f32(x):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, dtype=np.float32) * np.float32(32768.0)       # one fp32 multiply
        r = np.rint(v)                                                   # ties to even
        s = np.where(r < -32768, -32768.0, np.where(r > 32767, 32767.0, r))
        s = np.where(np.isnan(r), 0.0, s)
    return s.astype(np.int64)


RULES = {"s16": lambda x: np.asarray(x).astype(np.int64), "ulaw": ulaw, "alaw": alaw, "u8": u8, "i2s32": i2s32, "s32": s32,
         "f32": f32}


def decode(x, fmt):
    """int16 array of the shape of ``x`` (dtype ``DTYPES[fmt]``)."""
    x = np.asarray(x)
    assert x.dtype == DTYPES[fmt], (x.dtype, fmt)
    out = RULES[fmt](x)
    assert out.min(initial=0) >= -32768 and out.max(initial=0) <= 32767
    return out.astype(np.int16)


def encode_like(pcm, fmt, rng):
    """Samples of format ``fmt`` for an end-to-end test from int16 ``pcm``: random bytes for the G.711 formats (every
    code, both signs), the exact pre-image for the others."""
    pcm = np.asarray(pcm, dtype=np.int16)
    if fmt == "s16":
        return pcm.copy()
    if fmt in ("ulaw", "alaw"):
        return rng.integers(0, 256, size=pcm.shape, dtype=np.uint8)
    if fmt == "u8":
        return ((pcm.astype(np.int32) >> 8) + 128).astype(np.uint8)
    if fmt == "i2s32":
        # bits 25..10 carry the sample; random bits above and below, which the rule drops
        w = (pcm.astype(np.int64) & 0xffff) << 10
        w |= rng.integers(0, 1 << 10, size=pcm.shape, dtype=np.int64)
        w |= rng.integers(0, 1 << 6, size=pcm.shape, dtype=np.int64) << 26
        return (w & 0xffffffff).astype(np.uint32).view(np.int32)
    if fmt == "s32":
        w = (pcm.astype(np.int64) << 16) | rng.integers(0, 1 << 16, size=pcm.shape, dtype=np.int64)
        return (w & 0xffffffff).astype(np.uint32).view(np.int32)
    return (pcm.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
