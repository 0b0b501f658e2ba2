// Centred framing on the device (center_plan.hpp states the rule): the streaming kernel that writes
// the padded signal p of a row x, decoding x by mfcc_decode::rule<FMT> while it pads (S16: as it is).
//
// center_samples_kernel<FMT> (rows at a stride) and center_utterances_kernel<FMT> (a record per utterance) share one row
// body in the shape of decode_samples_kernel: groups of 8 output samples per lane, one 16-byte store each.  The OUTPUT
// decides the alignment: `head` samples go one by one up to the first 16-byte-aligned output element, the samples behind
// the last whole group too.  An interior group -- its eight sources all lie in [0, n) -- reads them with the widest load
// their address is aligned for (the source is displaced by PL against the output: S16 takes the unaligned 16-byte form
// of pack_utterances_kernel, the other formats aligned loads of 16 / 8 / 4 / 2 / 1 bytes, chosen per row, wave-uniform).
// A group that touches an edge fetches its eight samples one by one through the index rule.  All index arithmetic in 64
// bits.  Nothing outside [in, in + n * size) of a row is read, nothing outside [out, out + N') written.  No LDS, no atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "center_plan.hpp"
#include "kernel_decode.hpp"

namespace mfcc_center {

// The launches.  Dense: `rows` rows of n samples in format fmt (row r at sample r * in_stride of `in`) -> rows of np =
// padded(g, n) int16 at out + r * out_stride; np > 0, out_stride a multiple of 8 where rows > 1.  Ragged: the n_utt
// records of d_recs (center_plan.hpp: fill_table; source offsets in samples from `in`, destination offsets from `out`),
// max_padded the longest N' among them.  Both return false for an unknown format.  The kernels and these functions are
// compiled in a translation unit of their own (center.hip defines MFCC_CENTER_DEFINE_KERNELS): a code object of their own.
bool launch_dense(int fmt, const void *in, int16_t *out, size_t n, size_t np, size_t rows, size_t in_stride, size_t out_stride,
                  const Geom &g, int n_cu, hipStream_t stream);
bool launch_ragged(int fmt, const void *in, int16_t *out, const long long *d_recs, size_t n_utt, size_t max_padded,
                   const Geom &g, int n_cu, hipStream_t stream);

#ifdef MFCC_CENTER_DEFINE_KERNELS

using mfcc_decode::sample_size;
using mfcc_fc::kDecodeGroup;
using mfcc_fc::kDecodeThreads;

typedef unsigned int ctr_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int ctr_u32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(2))) CtrUnaligned16 {
    ctr_u32x4 v;
};

// bytes of the widest load of an interior group (S16: the one unaligned form)
constexpr int wide_load(int fmt) { return sample_size(fmt) == 1 ? 8 : 16; }

// sample j of the row, 0 <= j < n
template <int FMT>
__device__ __forceinline__ int sample_at(const unsigned char *src, long long j) {
    if constexpr (FMT == MFCC_HIP_SAMPLE_S16) return reinterpret_cast<const int16_t *>(src)[j];
    else if constexpr (sample_size(FMT) == 1) return mfcc_decode::rule<FMT>(src[j]);
    else return mfcc_decode::rule<FMT>(reinterpret_cast<const unsigned *>(src)[j]);
}

// p[i] by the index rule (center_plan.hpp: source)
template <int FMT>
__device__ __forceinline__ int padded_at(const unsigned char *src, long long n, long long i, long long left, int zeros) {
    long long j = i - left;
    if (j < 0 || j >= n) {
        if (zeros) return 0;
        j = j < 0 ? -j : 2 * (n - 1) - j;
        if (j < 0 || j >= n) return 0;
    }
    return sample_at<FMT>(src, j);
}

__device__ __forceinline__ ctr_u32x4 pack8(const int (&s)[kDecodeGroup]) {
    ctr_u32x4 v;
    v.x = (unsigned(s[0]) & 0xffffu) | unsigned(s[1]) << 16;
    v.y = (unsigned(s[2]) & 0xffffu) | unsigned(s[3]) << 16;
    v.z = (unsigned(s[4]) & 0xffffu) | unsigned(s[5]) << 16;
    v.w = (unsigned(s[6]) & 0xffffu) | unsigned(s[7]) << 16;
    return v;
}

// the eight int16 of an interior group whose sources start at p, read with loads of LW bytes (p is aligned to LW)
template <int FMT, int LW>
__device__ __forceinline__ ctr_u32x4 interior_group(const unsigned char *p) {
    if constexpr (FMT == MFCC_HIP_SAMPLE_S16) {
        return reinterpret_cast<const CtrUnaligned16 *>(p)->v;
    } else {
        constexpr int kSize = int(sample_size(FMT)), kWords = kDecodeGroup * kSize / 4;
        unsigned w[kWords];
        if constexpr (LW == 16) {
#pragma unroll
            for (int k = 0; k < kWords / 4; ++k) {
                const ctr_u32x4 v = reinterpret_cast<const ctr_u32x4 *>(p)[k];
                w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
            }
        } else if constexpr (LW == 8) {
#pragma unroll
            for (int k = 0; k < kWords / 2; ++k) {
                const ctr_u32x2 v = reinterpret_cast<const ctr_u32x2 *>(p)[k];
                w[2 * k] = v.x; w[2 * k + 1] = v.y;
            }
        } else if constexpr (LW == 4) {
#pragma unroll
            for (int k = 0; k < kWords; ++k) w[k] = reinterpret_cast<const unsigned *>(p)[k];
        } else if constexpr (LW == 2) {
#pragma unroll
            for (int k = 0; k < kWords; ++k) {
                const unsigned short *q = reinterpret_cast<const unsigned short *>(p) + 2 * k;
                w[k] = unsigned(q[0]) | unsigned(q[1]) << 16;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kWords; ++k)
                w[k] = unsigned(p[4 * k]) | unsigned(p[4 * k + 1]) << 8 | unsigned(p[4 * k + 2]) << 16 | unsigned(p[4 * k + 3]) << 24;
        }
        int s[kDecodeGroup];
#pragma unroll
        for (int k = 0; k < kDecodeGroup; ++k)
            s[k] = kSize == 1 ? mfcc_decode::rule<FMT>((w[k >> 2] >> (8 * (k & 3))) & 0xffu) : mfcc_decode::rule<FMT>(w[k * kSize / 4]);
        return pack8(s);
    }
}

// the whole groups g0, g0 + gstep, .. of a row: dst points behind its head (16-byte aligned), i0 = head
template <int FMT, int LW>
__device__ __forceinline__ void center_groups(const unsigned char *src, long long n, int16_t *dst, long long groups, long long head,
                                              long long left, int zeros, long long g0, long long gstep) {
    constexpr int kSize = int(sample_size(FMT));
    for (long long g = g0; g < groups; g += gstep) {
        const long long i0 = head + g * kDecodeGroup, j0 = i0 - left;
        ctr_u32x4 v;
        if (j0 >= 0 && j0 + kDecodeGroup <= n) {
            v = interior_group<FMT, LW>(src + j0 * kSize);
        } else {
            int s[kDecodeGroup];
#pragma unroll
            for (int k = 0; k < kDecodeGroup; ++k) s[k] = padded_at<FMT>(src, n, i0 + k, left, zeros);
            v = pack8(s);
        }
        reinterpret_cast<ctr_u32x4 *>(dst)[g] = v;
    }
}

// One row: src holds n samples, dst takes np.  The lanes that call it share the groups g0, g0 + gstep, ..; those with
// `ends` set also write the head and the tail, lane `lane` of `lanes`
template <int FMT>
__device__ __forceinline__ void center_row(const unsigned char *src, long long n, int16_t *dst, long long np, long long left,
                                           int zeros, long long g0, long long gstep, bool ends, int lane, int lanes) {
    constexpr int kSize = int(sample_size(FMT)), kWide = wide_load(FMT);
    long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 1);
    if (head > np) head = np;
    const long long groups = (np - head) >> 3, tail0 = head + 8 * groups;
    if (ends) {
        for (long long i = lane; i < head; i += lanes) dst[i] = int16_t(padded_at<FMT>(src, n, i, left, zeros));
        for (long long i = tail0 + lane; i < np; i += lanes) dst[i] = int16_t(padded_at<FMT>(src, n, i, left, zeros));
    }
    if constexpr (FMT == MFCC_HIP_SAMPLE_S16) {
        center_groups<FMT, kWide>(src, n, dst + head, groups, head, left, zeros, g0, gstep);
    } else {
        // the sources of group g start at src + (head + 8 g - left) * size: every group of the row has the alignment of
        // the first (only the low bits matter, so an address below src is as good as any)
        const uintptr_t a = reinterpret_cast<uintptr_t>(src) + uintptr_t((head - left) * kSize);
        int lw = kWide;
        while (lw > kSize && (a & uintptr_t(lw - 1))) lw >>= 1;
        if (lw == kWide) center_groups<FMT, kWide>(src, n, dst + head, groups, head, left, zeros, g0, gstep);
        else if (lw == kWide / 2) center_groups<FMT, kWide / 2>(src, n, dst + head, groups, head, left, zeros, g0, gstep);
        else if (lw == kWide / 4) center_groups<FMT, kWide / 4>(src, n, dst + head, groups, head, left, zeros, g0, gstep);
        else center_groups<FMT, kSize>(src, n, dst + head, groups, head, left, zeros, g0, gstep);
    }
}

// rows of n samples: row r reads in + r * in_stride (bytes) and writes np samples at out + r * out_stride (samples).
// grid: x strides over the groups, y over the rows
template <int FMT>
__global__ __launch_bounds__(kDecodeThreads) void center_samples_kernel(const unsigned char *__restrict__ in,
                                                                         int16_t *__restrict__ out, long long n, long long np,
                                                                         long long rows, long long in_stride, long long out_stride,
                                                                         long long left, int zeros) {
    for (long long r = blockIdx.y; r < rows; r += gridDim.y)
        center_row<FMT>(in + r * in_stride, n, out + r * out_stride, np, left, zeros,
                        (long long)blockIdx.x * kDecodeThreads + threadIdx.x, (long long)gridDim.x * kDecodeThreads, blockIdx.x == 0,
                        int(threadIdx.x), kDecodeThreads);
}

// a record per utterance (center_plan.hpp: kRecLL): x strides over the utterances, y over the groups of each
template <int FMT>
__global__ __launch_bounds__(kDecodeThreads) void center_utterances_kernel(const unsigned char *__restrict__ in,
                                                                            int16_t *__restrict__ out,
                                                                            const long long *__restrict__ recs, long long n_utt,
                                                                            long long left, int zeros) {
    constexpr long long kSize = (long long)sample_size(FMT);
    for (long long u = blockIdx.x; u < n_utt; u += gridDim.x) {
        const long long s0 = recs[kRecLL * u], n = recs[kRecLL * u + 1], d0 = recs[kRecLL * u + 2], np = recs[kRecLL * u + 3];
        if (np <= 0) continue;
        center_row<FMT>(in + s0 * kSize, n, out + d0, np, left, zeros, (long long)blockIdx.y * kDecodeThreads + threadIdx.x,
                        (long long)gridDim.y * kDecodeThreads, blockIdx.y == 0, int(threadIdx.x), kDecodeThreads);
    }
}

#define MFCC_CTR_FORMATS(X)                                                                                                   \
    X(MFCC_HIP_SAMPLE_S16) X(MFCC_HIP_SAMPLE_ULAW) X(MFCC_HIP_SAMPLE_ALAW) X(MFCC_HIP_SAMPLE_U8) X(MFCC_HIP_SAMPLE_I2S32)     \
    X(MFCC_HIP_SAMPLE_S32) X(MFCC_HIP_SAMPLE_F32)

bool launch_dense(int fmt, const void *in, int16_t *out, size_t n, size_t np, size_t rows, size_t in_stride, size_t out_stride,
                  const Geom &g, int n_cu, hipStream_t stream) {
    const size_t size = sample_size(fmt);
    if (size == 0) return false;
    unsigned gx, gy;
    mfcc_fc::decode_grid((long long)(np >> 3), (long long)rows, n_cu, gx, gy);
    const dim3 grid(gx, gy), block(kDecodeThreads);
    const unsigned char *src = static_cast<const unsigned char *>(in);
#define MFCC_CTR_CASE(F)                                                                                                      \
    case F:                                                                                                                   \
        hipLaunchKernelGGL(center_samples_kernel<F>, grid, block, 0, stream, src, out, (long long)n, (long long)np,           \
                           (long long)rows, (long long)(in_stride * size), (long long)out_stride, g.left,                     \
                           int(g.edge == kZeros));                                                                            \
        break;
    switch (fmt) {
        MFCC_CTR_FORMATS(MFCC_CTR_CASE)
    default: return false;
    }
#undef MFCC_CTR_CASE
    return true;
}

bool launch_ragged(int fmt, const void *in, int16_t *out, const long long *d_recs, size_t n_utt, size_t max_padded,
                   const Geom &g, int n_cu, hipStream_t stream) {
    if (sample_size(fmt) == 0) return false;
    // the grid of the dense form with the utterances as rows (on x here: there is no limit of 65535 on x)
    long long cap = (long long)n_cu * mfcc_fc::kDecodeBlocksPerCu;
    long long x = (long long)n_utt < cap ? (long long)n_utt : cap;
    if (x < 1) x = 1;
    long long y = ((long long)(max_padded >> 3) + kDecodeThreads - 1) / kDecodeThreads;
    if (y > cap / x) y = cap / x;
    if (y < 1) y = 1;
    const dim3 grid((unsigned)x, (unsigned)y), block(kDecodeThreads);
    const unsigned char *src = static_cast<const unsigned char *>(in);
#define MFCC_CTR_CASE(F)                                                                                                      \
    case F:                                                                                                                   \
        hipLaunchKernelGGL(center_utterances_kernel<F>, grid, block, 0, stream, src, out, d_recs, (long long)n_utt, g.left,   \
                           int(g.edge == kZeros));                                                                            \
        break;
    switch (fmt) {
        MFCC_CTR_FORMATS(MFCC_CTR_CASE)
    default: return false;
    }
#undef MFCC_CTR_CASE
    return true;
}

#undef MFCC_CTR_FORMATS

#endif  // MFCC_CENTER_DEFINE_KERNELS

}  // namespace mfcc_center
