// Sample formats (include/mfcc_hip.h: enum mfcc_hip_sample_format): the rules that turn a G.711
// byte, an 8-bit sample, an I2S word, an int32 or a float into the int16 the MFCC kernels read, and the streaming kernel
// that applies them.  The rules are plain integer arithmetic (one named fp32 multiply and one rintf for F32), written
// once for the host (mfcc_hip_decode_host) and the device.
//
// decode_samples_kernel<FMT>: grid-stride over groups of 8 samples per lane.  A group is one 8-byte load (1-byte
// formats) or two 16-byte loads (4-byte formats) and one 16-byte store of eight int16.  The OUTPUT decides the alignment:
// `head` samples go one by one up to the first 16-byte-aligned output element, the samples behind the last whole group go
// one by one too, both by the first workgroup of the same launch.  Where the input of the aligned groups is not aligned
// for the wide load the host picks narrower loads for the whole launch (load_bytes, wave-uniform).  Nothing outside
// [in, in + n * size) of a row is read, nothing outside [out, out + n) written.  No LDS, no atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mfcc_hip.h"
#include "launch_geom.hpp"

namespace mfcc_decode {

using mfcc_fc::kDecodeGroup;
using mfcc_fc::kDecodeThreads;

#define MFCC_DEC_HD __host__ __device__ __forceinline__

// ---- the rules (include/mfcc_hip.h states them; all integers 32-bit two's complement)
MFCC_DEC_HD int rule_ulaw(unsigned b) {
    const unsigned u = ~b & 0xffu;
    const int t = int((((u & 0x0fu) << 3) + 0x84u) << ((u & 0x70u) >> 4));
    return (u & 0x80u) ? 0x84 - t : t - 0x84;
}

MFCC_DEC_HD int rule_alaw(unsigned b) {
    const unsigned a = (b ^ 0x55u) & 0xffu, seg = (a & 0x70u) >> 4, t0 = (a & 0x0fu) << 4;
    // seg 0: t0 + 8; seg 1: t0 + 0x108; else (t0 + 0x108) << (seg - 1) -- one shift and one select, no branch
    const unsigned big = (t0 + 0x108u) << (seg ? seg - 1u : 0u);
    const int t = int(seg ? big : t0 + 8u);
    return (a & 0x80u) ? t : -t;
}

MFCC_DEC_HD int rule_u8(unsigned b) { return (int(b & 0xffu) - 128) * 256; }

// bits 25..10 of the word: da_shreg[-22:-6] of the reference's receiver (mfcc/io/i2s_mic.py:62)
MFCC_DEC_HD int rule_i2s32(unsigned w) { return int(int16_t(uint16_t(w >> 10))); }

MFCC_DEC_HD int rule_s32(unsigned w) { return int(w) >> 16; }

MFCC_DEC_HD int rule_f32(float x) {
    const float r = rintf(x * 32768.0f);               // one fp32 multiply, then ties to even
    if (!(r == r)) return 0;                            // NaN
    return r < -32768.0f ? -32768 : r > 32767.0f ? 32767 : int(r);
}

constexpr bool known(int fmt) { return fmt >= MFCC_HIP_SAMPLE_S16 && fmt <= MFCC_HIP_SAMPLE_F32; }

constexpr size_t sample_size(int fmt) {
    return fmt == MFCC_HIP_SAMPLE_S16 ? 2 : fmt >= MFCC_HIP_SAMPLE_ULAW && fmt <= MFCC_HIP_SAMPLE_U8 ? 1 : known(fmt) ? 4 : 0;
}

// bytes of the widest load of a group: the whole group of a 1-byte format, half the group of a 4-byte one
constexpr size_t wide_load(int fmt) { return sample_size(fmt) == 1 ? 8 : 16; }

// the int16 of one raw unit (a byte in the low bits of `raw`, or a 4-byte word)
template <int FMT>
MFCC_DEC_HD int rule(unsigned raw) {
    if (FMT == MFCC_HIP_SAMPLE_ULAW) return rule_ulaw(raw);
    if (FMT == MFCC_HIP_SAMPLE_ALAW) return rule_alaw(raw);
    if (FMT == MFCC_HIP_SAMPLE_U8) return rule_u8(raw);
    if (FMT == MFCC_HIP_SAMPLE_I2S32) return rule_i2s32(raw);
    if (FMT == MFCC_HIP_SAMPLE_S32) return rule_s32(raw);
#ifdef __HIP_DEVICE_COMPILE__
    return rule_f32(__uint_as_float(raw));
#else
    float x;
    __builtin_memcpy(&x, &raw, sizeof x);
    return rule_f32(x);
#endif
}

// the host form of every rule (S16 included): n samples at `in`, unaligned
inline void decode_host(int fmt, const void *in, size_t n, int16_t *out) {
    const unsigned char *p = static_cast<const unsigned char *>(in);
    auto word = [&](size_t i) {
        uint32_t w;
        __builtin_memcpy(&w, p + 4 * i, 4);
        return w;
    };
    switch (fmt) {
    case MFCC_HIP_SAMPLE_S16: __builtin_memcpy(out, in, n * sizeof(int16_t)); break;
    case MFCC_HIP_SAMPLE_ULAW: for (size_t i = 0; i < n; ++i) out[i] = int16_t(rule_ulaw(p[i])); break;
    case MFCC_HIP_SAMPLE_ALAW: for (size_t i = 0; i < n; ++i) out[i] = int16_t(rule_alaw(p[i])); break;
    case MFCC_HIP_SAMPLE_U8: for (size_t i = 0; i < n; ++i) out[i] = int16_t(rule_u8(p[i])); break;
    case MFCC_HIP_SAMPLE_I2S32: for (size_t i = 0; i < n; ++i) out[i] = int16_t(rule_i2s32(word(i))); break;
    case MFCC_HIP_SAMPLE_S32: for (size_t i = 0; i < n; ++i) out[i] = int16_t(rule_s32(word(i))); break;
    case MFCC_HIP_SAMPLE_F32: for (size_t i = 0; i < n; ++i) out[i] = int16_t(rule<MFCC_HIP_SAMPLE_F32>(word(i))); break;
    default: break;
    }
}

// The launch.  n > 0, rows > 0, in aligned to the sample size, out to 2 bytes, out_stride a multiple of 8 where rows > 1
// (checked by the callers).  Returns false for a format that has no kernel (S16, unknown).
// The kernels and this function are compiled in a translation unit of their own (decode.hip defines
// MFCC_DECODE_DEFINE_KERNELS): they form a code object of their own, and the code object of the MFCC kernels is, byte
// for byte, what it is without them.
bool launch(int fmt, const void *in, int16_t *out, size_t n, size_t rows, size_t in_stride_samples, size_t out_stride,
            int n_cu, hipStream_t stream);

#ifdef MFCC_DECODE_DEFINE_KERNELS

// ---- the kernel
typedef unsigned int dec_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int dec_u32x2 __attribute__((ext_vector_type(2)));

// the WORDS dwords of a group at p, read with loads of LW bytes each (p is aligned to LW)
template <int WORDS, int LW>
__device__ __forceinline__ void load_group(const unsigned char *p, unsigned (&w)[WORDS]) {
    if constexpr (LW == 16) {
#pragma unroll
        for (int k = 0; k < WORDS / 4; ++k) {
            const dec_u32x4 v = reinterpret_cast<const dec_u32x4 *>(p)[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    } else if constexpr (LW == 8) {
#pragma unroll
        for (int k = 0; k < WORDS / 2; ++k) {
            const dec_u32x2 v = reinterpret_cast<const dec_u32x2 *>(p)[k];
            w[2 * k] = v.x; w[2 * k + 1] = v.y;
        }
    } else if constexpr (LW == 4) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) w[k] = reinterpret_cast<const unsigned *>(p)[k];
    } else if constexpr (LW == 2) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) {
            const unsigned short *q = reinterpret_cast<const unsigned short *>(p) + 2 * k;
            w[k] = unsigned(q[0]) | unsigned(q[1]) << 16;
        }
    } else {
#pragma unroll
        for (int k = 0; k < WORDS; ++k)
            w[k] = unsigned(p[4 * k]) | unsigned(p[4 * k + 1]) << 8 | unsigned(p[4 * k + 2]) << 16 | unsigned(p[4 * k + 3]) << 24;
    }
}

// the whole groups of a row: src and dst point behind its head, dst is 16-byte aligned
template <int FMT, int LW>
__device__ __forceinline__ void decode_groups(const unsigned char *src, int16_t *dst, long long groups) {
    constexpr int kSize = int(sample_size(FMT)), kWords = kDecodeGroup * kSize / 4;
    const long long step = (long long)gridDim.x * kDecodeThreads;
    for (long long g = (long long)blockIdx.x * kDecodeThreads + threadIdx.x; g < groups; g += step) {
        unsigned w[kWords];
        load_group<kWords, LW>(src + g * (kDecodeGroup * kSize), w);
        int s[kDecodeGroup];
#pragma unroll
        for (int k = 0; k < kDecodeGroup; ++k)
            s[k] = kSize == 1 ? rule<FMT>((w[k >> 2] >> (8 * (k & 3))) & 0xffu) : rule<FMT>(w[k * kSize / 4]);
        dec_u32x4 v;
        v.x = (unsigned(s[0]) & 0xffffu) | unsigned(s[1]) << 16;
        v.y = (unsigned(s[2]) & 0xffffu) | unsigned(s[3]) << 16;
        v.z = (unsigned(s[4]) & 0xffffu) | unsigned(s[5]) << 16;
        v.w = (unsigned(s[6]) & 0xffffu) | unsigned(s[7]) << 16;
        reinterpret_cast<dec_u32x4 *>(dst)[g] = v;
    }
}

template <int FMT>
__device__ __forceinline__ int decode_one(const unsigned char *src, long long i) {
    if constexpr (sample_size(FMT) == 1) return rule<FMT>(src[i]);
    else return rule<FMT>(reinterpret_cast<const unsigned *>(src)[i]);
}

// rows of n samples: row r reads in + r * in_stride (bytes) and writes out + r * out_stride (samples).  head < 8 is the
// same for every row (the host sees to it: out_stride is a multiple of 8 where there is more than one row), and so is
// load_bytes, the widest load every row's groups are aligned for.  grid: x strides over the groups, y over the rows
template <int FMT>
__global__ __launch_bounds__(kDecodeThreads) void decode_samples_kernel(const unsigned char *__restrict__ in,
                                                                         int16_t *__restrict__ out, long long n, long long rows,
                                                                         long long in_stride, long long out_stride, int head,
                                                                         int load_bytes) {
    constexpr int kSize = int(sample_size(FMT)), kWide = int(wide_load(FMT));
    const long long groups = (n - head) >> 3, tail0 = head + 8 * groups;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const unsigned char *src = in + r * in_stride;
        int16_t *dst = out + r * out_stride;
        if (blockIdx.x == 0) {
            const int t = threadIdx.x;
            if (t < head) dst[t] = int16_t(decode_one<FMT>(src, t));
            if (t >= 64 && tail0 + (t - 64) < n) dst[tail0 + (t - 64)] = int16_t(decode_one<FMT>(src, tail0 + (t - 64)));
        }
        src += (long long)head * kSize;
        dst += head;
        if (load_bytes == kWide) decode_groups<FMT, kWide>(src, dst, groups);
        else if (load_bytes == kWide / 2) decode_groups<FMT, kWide / 2>(src, dst, groups);
        else if (load_bytes == kWide / 4) decode_groups<FMT, kWide / 4>(src, dst, groups);
        else decode_groups<FMT, kSize>(src, dst, groups);
    }
}

bool launch(int fmt, const void *in, int16_t *out, size_t n, size_t rows, size_t in_stride_samples, size_t out_stride,
            int n_cu, hipStream_t stream) {
    const size_t size = sample_size(fmt);
    if (size == 0 || fmt == MFCC_HIP_SAMPLE_S16) return false;
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) >> 1;
    if (head > n) head = n;
    const uintptr_t first = reinterpret_cast<uintptr_t>(in) + head * size;
    const size_t in_stride = in_stride_samples * size;
    // the widest load the groups of every row are aligned for: 8, 4, 2, 1 bytes (1-byte formats) or 16, 8, 4 (4-byte ones)
    size_t lw = wide_load(fmt);
    while (lw > size && ((first & (lw - 1)) || (rows > 1 && (in_stride & (lw - 1))))) lw >>= 1;
    unsigned gx, gy;
    mfcc_fc::decode_grid((long long)((n - head) >> 3), (long long)rows, n_cu, gx, gy);
    const dim3 grid(gx, gy), block(kDecodeThreads);
    const unsigned char *src = static_cast<const unsigned char *>(in);
#define MFCC_DEC_CASE(F)                                                                                                      \
    case F:                                                                                                                   \
        hipLaunchKernelGGL(decode_samples_kernel<F>, grid, block, 0, stream, src, out, (long long)n, (long long)rows,         \
                           (long long)in_stride, (long long)out_stride, int(head), int(lw));                                  \
        break;
    switch (fmt) {
        MFCC_DEC_CASE(MFCC_HIP_SAMPLE_ULAW)
        MFCC_DEC_CASE(MFCC_HIP_SAMPLE_ALAW)
        MFCC_DEC_CASE(MFCC_HIP_SAMPLE_U8)
        MFCC_DEC_CASE(MFCC_HIP_SAMPLE_I2S32)
        MFCC_DEC_CASE(MFCC_HIP_SAMPLE_S32)
        MFCC_DEC_CASE(MFCC_HIP_SAMPLE_F32)
    default: return false;
    }
#undef MFCC_DEC_CASE
    return true;
}

#endif  // MFCC_DECODE_DEFINE_KERNELS

}  // namespace mfcc_decode
