// Delta and delta-delta coefficients of float rows already in HBM (include/mfcc_hip.h: mfcc_hip_deltas_dev,
// DESIGN.md section 4.7).  A pass after the MFCC kernels and after normalization, not a change to either.
//
// in: float32 static rows [R][W], W = 1..64; out: rows [R][W * (1 + K)] at the same row indices, each
// [ s_t | D_t | DD_t (K = 2) ].  A segment is a range of whole rows (one channel of a dense call, one utterance of a
// ragged one); its tiles are those of kernel_normalize.hpp (Segs / tile_of / BlockRec), only the tile size differs.
//   D_t  = r * sum_{n=1..N} n (s_{t+n} - s_{t-n}),  r = 1 / (2 sum n^2),  indices clamped to the segment
//   DD_t = the same formula on the D rows, clamped the same way
// Every element is this fixed fp32 sequence (acc = fma(n, a_n - b_n, acc) for n ascending, then acc * r32, nothing
// else contracted): the tile size, the alignment of the rows and the entry point cannot change a bit.
//
// One workgroup per tile of T rows of one segment.  The static rows [t0 - KN, t0 + T + KN) go to LDS: the part inside
// the segment with float4 loads (scalar head and tail, as in normalization; nothing outside the segment is read), the
// part outside it as copies of the segment's first / last row -- the clamped indices, made once per tile.  Then one
// thread per (row, column) element, with no index arithmetic in the taps: with K = 2 the D rows [t0 - N, t0 + T + N)
// (a row outside the segment gets the D of the segment's edge row, which is what clamping D's index means), then s, D
// and DD of every tile row into an LDS copy of the tile's output, in the output's own layout.  Last, the tile's
// T * W * (1 + K) contiguous output floats leave with float4 stores (the copy is placed so that its 16-byte boundaries
// are those of the output).  K and N are template parameters: the taps unroll.  No atomics.
//
// These lines are compiled twice, as kernel_normalize.hpp's are: as mfcc_delta::deltas_kernel over
// 16 KB of LDS in mfcc_hip.hip, and as mfcc_delta_wide::deltas_wide_kernel over post_plan.hpp's kDeltaWideLdsFloats in
// post_wide.hip (MFCC_POST_WIDE_UNIT), for rows of 65 .. 128 floats.  delta_at is the same lines in both: a column gets the
// same bits from either.  At 128 x (1 + 2) the int products stay small: a tile's output is at most kLdsFloats floats.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_normalize.hpp"
#include "post_plan.hpp"

#ifdef MFCC_POST_WIDE_UNIT
#define MFCC_DELTA_NS mfcc_delta_wide
#define MFCC_DELTA_LDS_FLOATS mfcc_post::kDeltaWideLdsFloats
#define MFCC_DELTAS_KERNEL deltas_wide_kernel
#else
#define MFCC_DELTA_NS mfcc_delta
#define MFCC_DELTA_LDS_FLOATS 4096
#define MFCC_DELTAS_KERNEL deltas_kernel
#endif

namespace MFCC_DELTA_NS {

constexpr int kThreads = 256;
constexpr int kLdsFloats = MFCC_DELTA_LDS_FLOATS;      // 16 KB of LDS per workgroup (eight per CU): static rows, (K = 2) D rows, output tile
constexpr int kMaxWidth = mfcc_norm::kMaxWidth;
constexpr int kMaxWindow = 8;

using mfcc_norm::f32x4;

// rows per tile: what fits in LDS with the halos.  K = 1: (T + 2N) W static + T 2W output floats; K = 2:
// (T + 4N) W static + (T + 2N) W delta + T 3W output floats; 8 floats of slack for the alignment of the output copy.
// At least 3 rows for every W <= 64, N <= 8 (60 at W = 13, K = N = 2)
__host__ __device__ inline int tile_rows(int width, int order, int window) {
    return mfcc_post::delta_tile_rows_of(kLdsFloats, width, order, window);
}

// r32 = (float)(1 / (2 sum_{n=1..N} n^2))
__host__ __device__ inline float delta_scale(int window) {
    const int s = window * (window + 1) * (2 * window + 1) / 6;
    return float(1.0 / (2.0 * double(s)));
}

// the delta of column c of the row at src (rows W floats apart; the rows N above and below are there, already clamped)
template <int N>
__device__ __forceinline__ float delta_at(const float *src, int W, float r32) {
#pragma clang fp contract(off)
    float acc = 0.0f;
#pragma unroll
    for (int k = 1; k <= N; ++k) acc = __builtin_fmaf(float(k), src[k * W] - src[-k * W], acc);
    return acc * r32;
}

template <int K, int N>
__global__ __launch_bounds__(kThreads) void MFCC_DELTAS_KERNEL(const float *__restrict__ x, float *__restrict__ y,
                                                               mfcc_norm::Segs s, float r32) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    constexpr int H = K * N;                                      // static rows staged on each side of the tile
    const int W = s.width, WO = W * (1 + K), t = threadIdx.x, T = s.tile_rows;
    float *sx = lds;                                              // static rows row0 - H .. row0 + T + H
    float *sd = lds + (T + 2 * H) * W;                            // D rows row0 - N .. row0 + T + N (K = 2)
    float *so = lds + (((T + 2 * H) * W + (K == 2 ? (T + 2 * N) * W : 0) + 3) & ~3);   // the output tile
    const unsigned mis_x = unsigned(reinterpret_cast<uintptr_t>(x) >> 2) & 3u;
    const unsigned mis_y = unsigned(reinterpret_cast<uintptr_t>(y) >> 2) & 3u;
    const int r_t = t / W, c_t = t - r_t * W, dr = kThreads / W, dc = kThreads % W;   // (row, col) of element t, step
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg, lo, hi;
        int rows;
        mfcc_norm::tile_of(s, b, row0, rows, seg);
        if (!s.blk) {
            lo = s.base_row + seg * s.seg_rows;
            hi = lo + s.seg_rows;
        } else {
            const mfcc_norm::BlockRec f = s.blk[s.seg_blk0[seg]], l = s.blk[s.seg_blk0[seg + 1] - 1];
            lo = f.row0;
            hi = l.row0 + l.rows;
        }
        const long long a = row0 - H > lo ? row0 - H : lo;
        const long long e = row0 + rows + H < hi ? row0 + rows + H : hi;
        const int va = int(a - (row0 - H)), ve = int(e - (row0 - H)), nv_rows = rows + 2 * H;   // [va, ve): loaded
        {
            const long long e0 = a * W;
            const int n = (ve - va) * W, head = mfcc_norm::head_of(e0, n, mis_x), nv = (n - head) >> 2;
            const f32x4 *xv = reinterpret_cast<const f32x4 *>(x + e0 + head);
            float *dst = sx + va * W;
            for (int i = t; i < nv; i += kThreads) {
                const f32x4 v = xv[i];
                float *d = dst + head + 4 * i;
                d[0] = v.x;
                d[1] = v.y;
                d[2] = v.z;
                d[3] = v.w;
            }
            if (t < head) dst[t] = x[e0 + t];
            for (int i = head + 4 * nv + t; i < n; i += kThreads) dst[i] = x[e0 + i];
        }
        __syncthreads();
        if (va > 0 || ve < nv_rows) {                             // a segment edge: its row stands in for the rows beyond
            for (int i = t; i < va * W; i += kThreads) sx[i] = sx[va * W + i % W];
            for (int i = ve * W + t; i < nv_rows * W; i += kThreads) sx[i] = sx[(ve - 1) * W + i % W];
            __syncthreads();
        }
        // the output copy: element q of the tile's output at so[pad + q], pad such that so + pad + head is 16-aligned
        const long long o0 = row0 * WO;
        const int pad = int((o0 + mis_y) & 3);
        float *sq = so + pad;
        if (K == 2) {
            // D row u is row row0 - N + u, computed at that row clamped to the segment: local static row v
            const int ulo = int(lo - (row0 - N) > 0 ? lo - (row0 - N) : 0);
            const int uhi = int(hi - (row0 - N) < rows + 2 * N ? hi - (row0 - N) : rows + 2 * N) - 1;
            int r = r_t, c = c_t;
            for (int i = t; i < (rows + 2 * N) * W; i += kThreads) {
                const int u = r < ulo ? ulo : (r > uhi ? uhi : r);
                const float d = delta_at<N>(sx + (u + N) * W + c, W, r32);
                sd[i] = d;
                const int rt = r - N;                               // row of the tile, if it is one
                if (rt >= 0 && rt < rows) {
                    sq[rt * WO + c] = sx[(rt + H) * W + c];
                    sq[rt * WO + W + c] = d;
                }
                r += dr;
                c += dc;
                if (c >= W) c -= W, ++r;
            }
            __syncthreads();
            r = r_t;
            c = c_t;
            for (int i = t; i < rows * W; i += kThreads) {
                sq[r * WO + 2 * W + c] = delta_at<N>(sd + (r + N) * W + c, W, r32);
                r += dr;
                c += dc;
                if (c >= W) c -= W, ++r;
            }
        } else {
            int r = r_t, c = c_t;
            for (int i = t; i < rows * W; i += kThreads) {
                sq[r * WO + c] = sx[(r + H) * W + c];
                sq[r * WO + W + c] = delta_at<N>(sx + (r + H) * W + c, W, r32);
                r += dr;
                c += dc;
                if (c >= W) c -= W, ++r;
            }
        }
        __syncthreads();
        const int n = rows * WO, head = mfcc_norm::head_of(o0, n, mis_y), nv = (n - head) >> 2;
        f32x4 *yv = reinterpret_cast<f32x4 *>(y + o0 + head);
        const f32x4 *qv = reinterpret_cast<const f32x4 *>(sq + head);
        for (int i = t; i < nv; i += kThreads) __builtin_nontemporal_store(qv[i], yv + i);
        if (t < head) y[o0 + t] = sq[t];
        for (int i = head + 4 * nv + t; i < n; i += kThreads) y[o0 + i] = sq[i];
        __syncthreads();           // the next tile overwrites the LDS
    }
}

// the instantiation for (order, window); nullptr outside 1..2 x 1..kMaxWindow
typedef void (*DeltasKernel)(const float *__restrict__, float *__restrict__, mfcc_norm::Segs, float);
inline DeltasKernel deltas_kernel_of(int order, int window) {
    static const DeltasKernel k[2][kMaxWindow] = {
#define MFCC_DK MFCC_DELTAS_KERNEL
        {MFCC_DK<1, 1>, MFCC_DK<1, 2>, MFCC_DK<1, 3>, MFCC_DK<1, 4>, MFCC_DK<1, 5>, MFCC_DK<1, 6>, MFCC_DK<1, 7>, MFCC_DK<1, 8>},
        {MFCC_DK<2, 1>, MFCC_DK<2, 2>, MFCC_DK<2, 3>, MFCC_DK<2, 4>, MFCC_DK<2, 5>, MFCC_DK<2, 6>, MFCC_DK<2, 7>, MFCC_DK<2, 8>}};
#undef MFCC_DK
    if (order < 1 || order > 2 || window < 1 || window > kMaxWindow) return nullptr;
    return k[order - 1][window - 1];
}

}  // namespace mfcc_delta / mfcc_delta_wide
