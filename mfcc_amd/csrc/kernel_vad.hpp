// Energy voice-activity decision and voiced-row selection of float rows already in HBM (include/mfcc_hip.h:
// mfcc_hip_vad_dev / mfcc_hip_select_dev).  Passes after the MFCC kernels, not a change to them.
//
// A segment is a range of whole rows (one channel, one utterance); its tiles are those of kernel_normalize.hpp
// (Segs / tile_of / BlockRec), only the tile sizes differ.  The decision (Kaldi's ComputeVadEnergy) on column c of rows
// [R][W], W = 1..64:
//   mean     per tile of kMeanTileRows rows: float64 (n, sum) of the finite values of the column -- every thread adds
//            its rows in ascending order, then a halving tree over the 256 partial sums
//   theta    one workgroup per segment adds the tiles' partials (stripes of 256, then the same tree) and stores
//            theta = thr + scale * (sum / n) as a double, +inf when no value is finite (nothing is above it)
//   decide   per tile of rows plus a ctx-row halo of the column (nothing outside the segment is read): the `above`
//            flags as 64-bit ballots in LDS, then per row the popcount of its window [t - ctx, t + ctx] clipped to the
//            segment; voiced = (float)num >= (float)den * p.  Writes one byte per row and the tile's voiced count
// The orders of summation are functions of the segment's rows alone: the same bits wherever the segment lies.
// The selection of rows [R][W'], W' = 1..192, by a byte mask:
//   count    per tile, the number of non-zero mask bytes (not needed when `decide` ran on the same tiles)
//   scan     one workgroup of 1024: exclusive prefix of the tile counts -- tiles are in segment order, so the prefix at the
//            first tile of every segment is the segment's first row in the packed result
//   gather   per tile: the rank of every voiced row from ballots and a cross-wave prefix in LDS, the voiced rows staged
//            in LDS in the output's layout (placed so that its 16-byte boundaries are the output's) and written with
//            float4 nontemporal stores, scalar head and tail
// No atomics anywhere: the packed rows keep their order and every run gives the same bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_normalize.hpp"

namespace mfcc_vad {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;   // __ballot is 64 lanes wide on gfx950
constexpr int kMaxWidth = mfcc_norm::kMaxWidth;     // rows the decision reads
constexpr int kMaxSelectWidth = 3 * kMaxWidth;      // rows the selection moves: statics with D and DD
constexpr int kMaxContext = 64;
constexpr int kMeanTileRows = 4096;
constexpr int kMaxTileRows = 1024;      // decide / gather
constexpr int kLdsFloats = 4096;        // 16 KB: the gather's output tile (eight workgroups per CU)
constexpr int kScanThreads = 1024;

using mfcc_norm::f32x4;
using mfcc_norm::Segs;

// rows per tile of the selection (and of a decision whose counts feed it): what the output tile holds
__host__ __device__ inline int select_tile_rows(int width) {
    const int r = (kLdsFloats - 8) / width;
    return r < kMaxTileRows ? r : kMaxTileRows;
}

struct MeanPart {
    double n, sum;
};

// rows [lo, hi) of segment seg
__device__ __forceinline__ void seg_bounds(const Segs &s, long long seg, long long &lo, long long &hi) {
    if (!s.blk) {
        lo = s.base_row + seg * s.seg_rows;
        hi = lo + s.seg_rows;
    } else {
        const mfcc_norm::BlockRec f = s.blk[s.seg_blk0[seg]], l = s.blk[s.seg_blk0[seg + 1] - 1];
        lo = f.row0;
        hi = l.row0 + l.rows;
    }
}

// red[0] <- red[0] + ... + red[kThreads - 1], as a halving tree (a fixed order)
__device__ __forceinline__ void tree_sum(double *a, double *b, int t) {
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (t < st) {
            a[t] += a[t + st];
            b[t] += b[t + st];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void vad_mean_kernel(const float *__restrict__ x, Segs s, int column,
                                                            MeanPart *__restrict__ part) {
    __shared__ double rs[kThreads], rn[kThreads];
    const int W = s.width, t = threadIdx.x;
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg;
        int rows;
        mfcc_norm::tile_of(s, b, row0, rows, seg);
        const float *col = x + row0 * W + column;
        double sum = 0.0, k = 0.0;
        for (int r = t; r < rows; r += kThreads) {
            const float v = col[(long long)r * W];
            if (mfcc_norm::finite(v)) {
                sum += double(v);
                k += 1.0;
            }
        }
        rs[t] = sum;
        rn[t] = k;
        tree_sum(rs, rn, t);
        if (t == 0) part[b] = MeanPart{rn[0], rs[0]};
        __syncthreads();           // the next tile overwrites rs and rn
    }
}

__global__ __launch_bounds__(kThreads) void vad_theta_kernel(Segs s, const MeanPart *__restrict__ part, double thr,
                                                             double scale, double *__restrict__ theta) {
#pragma clang fp contract(off)
    __shared__ double rs[kThreads], rn[kThreads];
    const int t = threadIdx.x;
    for (long long seg = blockIdx.x; seg < s.n_segs; seg += gridDim.x) {
        long long b0, b1;
        if (!s.blk) {
            b0 = seg * s.blocks_per_seg;
            b1 = b0 + s.blocks_per_seg;
        } else {
            b0 = s.seg_blk0[seg];
            b1 = s.seg_blk0[seg + 1];
        }
        double sum = 0.0, k = 0.0;
        for (long long b = b0 + t; b < b1; b += kThreads) {
            const MeanPart p = part[b];
            sum += p.sum;
            k += p.n;
        }
        rs[t] = sum;
        rn[t] = k;
        tree_sum(rs, rn, t);
        if (t == 0) {
            const double mean = rs[0] / rn[0];
            theta[seg] = rn[0] > 0.0 ? thr + scale * mean : __builtin_inf();      // no finite value: nothing is above
        }
        __syncthreads();
    }
}

// set bits of entries [i0, i1] (inclusive) of the ballot words
__device__ __forceinline__ int count_range(const unsigned long long *masks, int i0, int i1) {
    const int w0 = i0 >> 6, w1 = i1 >> 6;
    int n = 0;
    for (int w = w0; w <= w1; ++w) {
        unsigned long long m = masks[w];
        if (w == w0) m &= ~0ull << (i0 & 63);
        if (w == w1) m &= ~0ull >> (63 - (i1 & 63));
        n += __popcll(m);
    }
    return n;
}

// theta_seg: one double per segment, or nullptr: theta_const for all (scale 0: no mean is taken)
__global__ __launch_bounds__(kThreads) void vad_decide_kernel(const float *__restrict__ x, Segs s, int column,
                                                              const double *__restrict__ theta_seg, double theta_const,
                                                              int ctx, float p, unsigned char *__restrict__ voiced,
                                                              unsigned *__restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ unsigned long long masks[(kMaxTileRows + 2 * kMaxContext + kThreads) / 64 + 1];
    __shared__ unsigned wsum[kWaves];
    const int W = s.width, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg, lo, hi;
        int rows;
        mfcc_norm::tile_of(s, b, row0, rows, seg);
        seg_bounds(s, seg, lo, hi);
        const double theta = theta_seg ? theta_seg[seg] : theta_const;
        // entry i is row row0 - ctx + i; a row outside the segment is not read and not above
        const long long first = row0 - ctx;
        const int nent = rows + 2 * ctx;
        for (int base = 0; base < nent; base += kThreads) {
            const int i = base + t;
            const long long row = first + i;
            bool f = false;
            if (i < nent && row >= lo && row < hi) {
                const float e = x[row * W + column];
                f = mfcc_norm::finite(e) && double(e) > theta;
            }
            const unsigned long long m = __ballot(f);
            if (lane == 0) masks[i >> 6] = m;
        }
        __syncthreads();
        unsigned cnt = 0;
        for (int base = 0; base < rows; base += kThreads) {
            const int r = base + t;
            bool v = false;
            if (r < rows) {
                const long long row = row0 + r;
                const int cl = int(row - lo < ctx ? row - lo : ctx), cr = int(hi - 1 - row < ctx ? hi - 1 - row : ctx);
                const int num = count_range(masks, r + ctx - cl, r + ctx + cr), den = cl + cr + 1;
                v = float(num) >= float(den) * p;
                voiced[row] = v ? 1 : 0;
            }
            cnt += unsigned(__popcll(__ballot(v)));
        }
        if (lane == 0) wsum[wave] = cnt;
        __syncthreads();
        if (t == 0) {
            unsigned n = 0;
            for (int w = 0; w < kWaves; ++w) n += wsum[w];
            counts[b] = n;
        }
        __syncthreads();           // the next tile overwrites masks and wsum
    }
}

__global__ __launch_bounds__(kThreads) void vad_count_kernel(const unsigned char *__restrict__ voiced, Segs s,
                                                             unsigned *__restrict__ counts) {
    __shared__ unsigned wsum[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg;
        int rows;
        mfcc_norm::tile_of(s, b, row0, rows, seg);
        unsigned cnt = 0;
        for (int base = 0; base < rows; base += kThreads) {
            const int r = base + t;
            cnt += unsigned(__popcll(__ballot(r < rows && voiced[row0 + r] != 0)));
        }
        if (lane == 0) wsum[wave] = cnt;
        __syncthreads();
        if (t == 0) {
            unsigned n = 0;
            for (int w = 0; w < kWaves; ++w) n += wsum[w];
            counts[b] = n;
        }
        __syncthreads();
    }
}

// tile_off[b] = counts[0] + ... + counts[b - 1] for b = 0 .. n_blocks, seg_off[k] = tile_off[first tile of segment k]
// for k = 0 .. n_segs (the first tile of "segment n_segs" is n_blocks).  One workgroup of kScanThreads: every thread
// sums a contiguous run of counts, the run sums are prefixed inside each wave with shuffles and across the sixteen
// waves through LDS, then every thread writes the prefixes of its run.
__global__ __launch_bounds__(kScanThreads) void vad_scan_kernel(Segs s, const unsigned *counts, long long *tile_off,
                                                                long long *seg_off) {
    __shared__ long long wtot[kScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long n = s.n_blocks, per = (n + kScanThreads - 1) / kScanThreads;
    const long long b0 = t * per < n ? t * per : n, b1 = b0 + per < n ? b0 + per : n;
    long long sum = 0;
#pragma unroll 4
    for (long long b = b0; b < b1; ++b) sum += counts[b];
    long long inc = sum;                                          // inclusive prefix of the run sums within the wave
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    long long acc = inc - sum;
    for (int w = 0; w < wave; ++w) acc += wtot[w];
    if (t == kScanThreads - 1) tile_off[n] = acc + sum;
    for (long long b = b0; b < b1; ++b) {
        tile_off[b] = acc;
        acc += counts[b];
    }
    __syncthreads();               // tile_off is read below by other threads of this workgroup
    for (long long k = t; k <= s.n_segs; k += kScanThreads)
        seg_off[k] = tile_off[s.blk ? s.seg_blk0[k] : k * s.blocks_per_seg];
}

__global__ __launch_bounds__(kThreads) void vad_gather_kernel(const float *__restrict__ x,
                                                              const unsigned char *__restrict__ voiced, Segs s,
                                                              const long long *__restrict__ tile_off,
                                                              float *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    __shared__ unsigned short src[kMaxTileRows];                  // src[j]: the tile row of the tile's j-th voiced row
    __shared__ unsigned wtot[kWaves];
    const int W = s.width, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned mis_y = unsigned(reinterpret_cast<uintptr_t>(y) >> 2) & 3u;
    const int j_t = t / W, c_t = t - j_t * W, dj = kThreads / W, dc = kThreads % W;   // (row, col) of element t, step
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg;
        int rows;
        mfcc_norm::tile_of(s, b, row0, rows, seg);
        const long long out_row = tile_off[b];
        const int cnt = int(tile_off[b + 1] - out_row);
        if (cnt == 0) continue;                                   // the whole workgroup: nothing of this tile is kept
        int run = 0;
        for (int base = 0; base < rows; base += kThreads) {
            const int r = base + t;
            const bool v = r < rows && voiced[row0 + r] != 0;
            const unsigned long long m = __ballot(v);
            if (lane == 0) wtot[wave] = unsigned(__popcll(m));
            __syncthreads();
            int pre = run, tot = 0;
            for (int w = 0; w < kWaves; ++w) {
                if (w < wave) pre += int(wtot[w]);
                tot += int(wtot[w]);
            }
            if (v) src[pre + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)r;
            run += tot;
            __syncthreads();       // wtot is rewritten; src is complete after the last round
        }
        // the output copy: element q of the tile's output at sq[q], sq + head 16-byte aligned like y + o0 + head
        const long long o0 = out_row * W;
        float *sq = lds + int((o0 + mis_y) & 3);
        const int n = (run < cnt ? run : cnt) * W;                // run == cnt: the counts are those of this mask
        // four elements per thread and round, so that four loads are in flight before the first is stored
        int j = j_t, c = c_t;
        int i = t;
        for (; i + 3 * kThreads < n; i += 4 * kThreads) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = x[(row0 + src[j]) * W + c];
                j += dj;
                c += dc;
                if (c >= W) c -= W, ++j;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) sq[i + u * kThreads] = v[u];
        }
        for (; i < n; i += kThreads) {
            sq[i] = x[(row0 + src[j]) * W + c];
            j += dj;
            c += dc;
            if (c >= W) c -= W, ++j;
        }
        __syncthreads();
        const int head = mfcc_norm::head_of(o0, n, mis_y), nv = (n - head) >> 2;
        f32x4 *yv = reinterpret_cast<f32x4 *>(y + o0 + head);
        const f32x4 *qv = reinterpret_cast<const f32x4 *>(sq + head);
        for (int i = t; i < nv; i += kThreads) __builtin_nontemporal_store(qv[i], yv + i);
        if (t < head) y[o0 + t] = sq[t];
        for (int i = head + 4 * nv + t; i < n; i += kThreads) y[o0 + i] = sq[i];
        __syncthreads();           // the next tile overwrites the LDS
    }
}

}  // namespace mfcc_vad
