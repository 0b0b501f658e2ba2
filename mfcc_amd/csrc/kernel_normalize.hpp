// Per-segment mean / variance normalization of float rows already in HBM (include/mfcc_hip.h:
// mfcc_hip_normalize_dev).  A pass after the MFCC kernels, not a change to them.
//
// rows: float32 [R][W], W = 1..64; a segment is a range of whole rows (one channel of a dense call, one utterance of
// a ragged one).  Three launches:
//   stats     one read of the rows: every workgroup takes a tile of kTileFloats / W rows of ONE segment (tiles
//             counted from the segment's own first row), stages it in LDS and writes the tile's per-column
//             (n, mean, M2) of the finite values in float64 (two passes over the LDS copy: sum, then squares of the
//             deviations from the tile mean)
//   finalize  one workgroup per segment combines its tiles' partials with Chan's formula in a fixed order and
//             stores (mu, 1/sigma') per column, each rounded once to fp32
//   apply     one read and one write: y = (x - mu) * r for finite x, x unchanged otherwise
// Every order of summation is a function of W and of the segment's rows alone (the 16-byte-aligned float4 body of
// a tile only decides how the bytes reach LDS or registers): a segment gives the same bits wherever it lies, in
// whatever call.  No atomics.
//
// These lines are compiled twice.  In the MFCC kernels' unit, mfcc_hip.hip, they are namespace
// mfcc_norm with width-sized LDS arrays of 64 columns, as they always were.  In post_wide.hip (MFCC_POST_WIDE_UNIT) they
// are namespace mfcc_norm_wide with arrays of 128 columns and kernels named *_wide_kernel: the filterbank post-passes'
// rows of 65 .. 128 floats.  Nothing else differs: the tile is kTileFloats in both, G = 256 / W is 3 for 65 .. 85 and 2
// for 86 .. 128, and a thread with g >= G reads mean_s[c] with c = t % W < W like any other.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seg_plan.hpp"      // Segs, BlockRec, tile_of: shared with the host planner

#ifdef MFCC_POST_WIDE_UNIT
#define MFCC_NORM_NS mfcc_norm_wide
#define MFCC_NORM_MAX_WIDTH 128
#define MFCC_NORM_STATS_KERNEL normalize_stats_wide_kernel
#define MFCC_NORM_FINALIZE_KERNEL normalize_finalize_wide_kernel
#define MFCC_NORM_APPLY_KERNEL normalize_apply_wide_kernel
#else
#define MFCC_NORM_NS mfcc_norm
#define MFCC_NORM_MAX_WIDTH 64
#define MFCC_NORM_STATS_KERNEL normalize_stats_kernel
#define MFCC_NORM_FINALIZE_KERNEL normalize_finalize_kernel
#define MFCC_NORM_APPLY_KERNEL normalize_apply_kernel
#endif

namespace MFCC_NORM_NS {

#ifdef MFCC_POST_WIDE_UNIT
using mfcc_norm::Segs;
using mfcc_norm::BlockRec;
using mfcc_norm::tile_of;
#endif

constexpr int kThreads = 256;
constexpr int kTileFloats = 8192;      // 32 KB of LDS per stats workgroup
constexpr int kMaxWidth = MFCC_NORM_MAX_WIDTH;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// rows per tile: a function of the row width only
__host__ __device__ inline int tile_rows(int width) { return kTileFloats / width; }

// per-column partial of one tile: count, mean and sum of squared deviations of the finite values
struct Part {
    double n, mean, m2;
};

__device__ __forceinline__ bool finite(float v) { return __builtin_isfinite(v); }

// Elements [e0, e0 + n) of x: the first one at which x + e is 16-byte aligned (x itself is 4-byte aligned; mis =
// its offset from 16 bytes in floats), clamped to n.  Everything before is the scalar head, then float4s, then the
// scalar tail; nothing outside [e0, e0 + n) is read.
__device__ __forceinline__ int head_of(long long e0, int n, unsigned mis) {
    const int head = int((4u - unsigned((e0 + mis) & 3)) & 3u);
    return head < n ? head : n;
}

__global__ __launch_bounds__(kThreads) void MFCC_NORM_STATS_KERNEL(const float *__restrict__ x, Segs s,
                                                                   Part *__restrict__ part) {
    __shared__ float tile[kTileFloats];
    __shared__ double red[kThreads];
    __shared__ double cnt[kThreads];
    __shared__ double mean_s[kMaxWidth];
    const int W = s.width, G = kThreads / W, t = threadIdx.x, c = t % W, g = t / W;
    const unsigned mis = unsigned(reinterpret_cast<uintptr_t>(x) >> 2) & 3u;
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg;
        int rows;
        tile_of(s, b, row0, rows, seg);
        const long long e0 = row0 * W;
        const int n = rows * W, head = head_of(e0, n, mis), nv = (n - head) >> 2;
        const f32x4 *xv = reinterpret_cast<const f32x4 *>(x + e0 + head);
        for (int i = t; i < nv; i += kThreads) {
            const f32x4 v = xv[i];
            float *d = tile + head + 4 * i;
            d[0] = v.x;
            d[1] = v.y;
            d[2] = v.z;
            d[3] = v.w;
        }
        if (t < head) tile[t] = x[e0 + t];
        for (int i = head + 4 * nv + t; i < n; i += kThreads) tile[i] = x[e0 + i];
        __syncthreads();
        // pass 1: thread (c, g) takes rows g, g + G, ... of column c; the G stripes are then added in order
        double sum = 0.0, k = 0.0;
        if (g < G)
            for (int r = g; r < rows; r += G) {
                const float v = tile[r * W + c];
                if (finite(v)) {
                    sum += double(v);
                    k += 1.0;
                }
            }
        red[t] = sum;
        cnt[t] = k;
        __syncthreads();
        if (t < W) {
            double S = 0.0, K = 0.0;
            for (int j = 0; j < G; ++j) {
                S += red[j * W + t];
                K += cnt[j * W + t];
            }
            mean_s[t] = K > 0.0 ? S / K : 0.0;
        }
        __syncthreads();
        // pass 2: squared deviations from the tile's mean
        const double m = mean_s[c];
        double q = 0.0;
        if (g < G)
            for (int r = g; r < rows; r += G) {
                const float v = tile[r * W + c];
                if (finite(v)) {
                    const double d = double(v) - m;
                    q += d * d;
                }
            }
        red[t] = q;
        __syncthreads();
        if (t < W) {
            double Q = 0.0, K = 0.0;
            for (int j = 0; j < G; ++j) {
                Q += red[j * W + t];
                K += cnt[j * W + t];
            }
            part[b * W + t] = Part{K, mean_s[t], Q};
        }
        __syncthreads();           // the next tile overwrites tile, red and cnt
    }
}

// Chan et al.: (n, m, q) <- (n, m, q) combined with (nb, mb, qb)
__device__ __forceinline__ void chan(double &n, double &m, double &q, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    if (n == 0.0) {
        n = nb;
        m = mb;
        q = qb;
        return;
    }
    const double N = n + nb, d = mb - m;
    m += d * (nb / N);
    q += qb + d * d * (n * nb / N);
    n = N;
}

// mode: 1 = mean only (r = 1), 2 = mean and variance.  coef[seg][col] = (mu, r), fp32
__global__ __launch_bounds__(kThreads) void MFCC_NORM_FINALIZE_KERNEL(Segs s, const Part *__restrict__ part,
                                                                      float2 *__restrict__ coef, int mode) {
    __shared__ double sn[kThreads], sm[kThreads], sq[kThreads];
    const int W = s.width, G = kThreads / W, t = threadIdx.x, c = t % W, g = t / W;
    for (long long seg = blockIdx.x; seg < s.n_segs; seg += gridDim.x) {
        long long b0, b1;
        if (!s.blk) {
            b0 = seg * s.blocks_per_seg;
            b1 = b0 + s.blocks_per_seg;
        } else {
            b0 = s.seg_blk0[seg];
            b1 = s.seg_blk0[seg + 1];
        }
        // stripe g combines tiles b0 + g, b0 + g + G, ... in order; then the stripes are combined in order
        double n = 0.0, m = 0.0, q = 0.0;
        if (g < G)
            for (long long b = b0 + g; b < b1; b += G) {
                const Part p = part[b * W + c];
                chan(n, m, q, p.n, p.mean, p.m2);
            }
        sn[t] = n;
        sm[t] = m;
        sq[t] = q;
        __syncthreads();
        if (t < W) {
            n = m = q = 0.0;
            for (int j = 0; j < G; ++j) chan(n, m, q, sn[j * W + t], sm[j * W + t], sq[j * W + t]);
            float mu = 0.0f, r = 1.0f;          // no finite value: y = (x - 0) * 1 = x
            if (n > 0.0) {
                mu = float(m);
                if (mode == 2) {
                    double sd = sqrt(q / n);
                    if (sd < 10.0 * 2.220446049250313e-16) sd = 1.0;      // sklearn's _handle_zeros_in_scale
                    r = float(1.0 / sd);
                }
            }
            coef[seg * W + t] = make_float2(mu, r);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float apply1(float v, float2 cf) { return finite(v) ? (v - cf.x) * cf.y : v; }

__global__ __launch_bounds__(kThreads) void MFCC_NORM_APPLY_KERNEL(float *__restrict__ x, Segs s,
                                                                   const float2 *__restrict__ coef) {
    __shared__ float2 cf[kMaxWidth];
    const int W = s.width, t = threadIdx.x;
    const int step = (4 * kThreads) % W;          // column advance of a lane per float4 stride
    const unsigned mis = unsigned(reinterpret_cast<uintptr_t>(x) >> 2) & 3u;
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg;
        int rows;
        tile_of(s, b, row0, rows, seg);
        if (t < W) cf[t] = coef[seg * W + t];
        __syncthreads();
        // a tile starts on a row: the column of element e0 + i is i % W
        const long long e0 = row0 * W;
        const int n = rows * W, head = head_of(e0, n, mis), nv = (n - head) >> 2;
        f32x4 *xv = reinterpret_cast<f32x4 *>(x + e0 + head);
        int col = (head + 4 * t) % W;
        for (int i = t; i < nv; i += kThreads) {
            f32x4 v = xv[i];
            int k = col;
            v.x = apply1(v.x, cf[k]);
            if (++k == W) k = 0;
            v.y = apply1(v.y, cf[k]);
            if (++k == W) k = 0;
            v.z = apply1(v.z, cf[k]);
            if (++k == W) k = 0;
            v.w = apply1(v.w, cf[k]);
            xv[i] = v;
            col += step;
            if (col >= W) col -= W;
        }
        if (t < head) x[e0 + t] = apply1(x[e0 + t], cf[t % W]);
        for (int i = head + 4 * nv + t; i < n; i += kThreads) x[e0 + i] = apply1(x[e0 + i], cf[i % W]);
        __syncthreads();           // the next tile overwrites cf
    }
}

}  // namespace mfcc_norm / mfcc_norm_wide

#ifdef MFCC_POST_WIDE_UNIT
// what kernel_deltas.hpp takes from mfcc_norm by name: in this unit, the wide unit's
namespace mfcc_norm {
using mfcc_norm_wide::f32x4;
using mfcc_norm_wide::head_of;
using mfcc_norm_wide::kMaxWidth;
}  // namespace mfcc_norm
#endif
