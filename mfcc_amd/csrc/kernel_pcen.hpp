// Per-channel energy normalization (PCEN) of log-mel rows already in HBM (include/mfcc_hip.h: mfcc_hip_set_pcen /
// mfcc_hip_pcen_dev).  A pass after the MFCC kernels, in place, in front of the normalization.
//
// rows: float32 [R][W], W = 1..64, log2 energies (non-finite: E = 0); a segment is a range of whole rows.  The smoother
// M_t = (1 - s) M_{t-1} + s E_t is the one recursive stage of the front end.  Its order of operations is fixed by tiles
// of kTile rows counted from the segment's own first row (frame t = slot k of tile i):
//     L_{i,-1} = 0,  L_{i,k} = fmaf(a, L_{i,k-1}, s * E_t)            the tile's own smoother, every term >= 0
//     C_0 = E_0,     C_{i+1} = fmaf(A_{T-1}, C_i, L_{i,T-1})          the carry into the next tile
//     M_t = fmaf(A_k, C_i, L_{i,k})                                   A_k = (float)((1 - s)^(k + 1)), from the host
// Three launches:
//   tile end  one thread per (full tile, column) runs the L recurrence over the tile and writes L_{i,T-1}
//   carry     one thread per (segment, column) walks the segment's tiles in order and writes C_i per tile
//   apply     one thread per (tile, column) runs the L recurrence again and writes y over x
// A lane is a column and a workgroup takes kThreads / W tiles, so every time step of a tile reads W contiguous floats.
// The only dependent chain is one fmaf per step: the loads of kAhead steps are issued before the first of them is used
// and exp2 / log2 hang off the chain.  The bits of a segment depend on its rows, W and the parameters alone.  No atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bank_plan.hpp"
#include "kernel_normalize.hpp"

namespace mfcc_pcen {

constexpr int kThreads = 256;
constexpr int kTile = 128;             // MFCC_HIP_PCEN_TILE
constexpr int kMaxWidth = mfcc_norm::kMaxWidth;
constexpr int kAhead = 8;              // time steps whose loads are in flight together

using mfcc_norm::Segs;
using mfcc_norm::tile_of;

// the parameters as the kernels use them (mfcc_hip_pcen_constants): passed by value, read with scalar loads
struct Prm {
    float s, a, alpha, r, eps, delta, delta_r;
    float decay[kTile];                // A_k
};

// E of one log2 energy: a silent band (-inf) and every other non-finite value count as 0
__device__ __forceinline__ float energy(float x) { return __builtin_isfinite(x) ? __builtin_amdgcn_exp2f(x) : 0.0f; }

// THE per-element arithmetic, x_t to y_t, of every PCEN kernel (the online bank's included): advances the tile's local
// smoother L by frame x and, with kOut, returns y for the carry C and the decay A_k of the frame's slot; M is the
// smoother's value (the next carry when the slot is the tile's last).  Without kOut only L is advanced.
template <bool kOut>
__device__ __forceinline__ float element(const Prm &p, float x, float A_k, float C, float &L, float &M) {
#pragma clang fp contract(off)
    const float E = energy(x);
    const float sE = p.s * E;
    L = __builtin_fmaf(p.a, L, sE);
    if (!kOut) return 0.0f;
    M = __builtin_fmaf(A_k, C, L);
    const float g = __builtin_amdgcn_logf(p.eps + M);
    const float q = __builtin_amdgcn_exp2f(-p.alpha * g);
    const float u = __builtin_fmaf(E, q, p.delta);
    const float w = p.r * __builtin_amdgcn_logf(u);
    return __builtin_amdgcn_exp2f(w) - p.delta_r;
}

// tiles per workgroup: a function of the row width only
__host__ __device__ inline int tiles_per_group(int width) { return kThreads / width; }

// lend[b][c] = L_{i,T-1} of every FULL tile b (a segment's last, partial tile has no successor to carry into)
__global__ __launch_bounds__(kThreads) void pcen_tile_end_kernel(const float *__restrict__ x, Segs s, Prm p,
                                                                 float *__restrict__ lend) {
    const int W = s.width, G = tiles_per_group(W), g = threadIdx.x / W, c = threadIdx.x - g * W;
    const long long n_groups = (s.n_blocks + G - 1) / G;
    for (long long j = blockIdx.x; j < n_groups; j += gridDim.x) {
        const long long b = j * G + g;
        if (g >= G || b >= s.n_blocks) continue;
        long long row0, seg;
        int rows;
        tile_of(s, b, row0, rows, seg);
        if (rows < kTile) continue;
        const float *px = x + row0 * W + c;
        float L = 0.0f, M;
        for (int k0 = 0; k0 < kTile; k0 += kAhead) {
            float v[kAhead];
#pragma unroll
            for (int i = 0; i < kAhead; ++i) v[i] = px[(k0 + i) * W];
#pragma unroll
            for (int i = 0; i < kAhead; ++i) element<false>(p, v[i], 0.0f, 0.0f, L, M);
        }
        lend[b * W + c] = L;
    }
}

// carry[b][c] = C_i of every tile b of every segment, from the segment's first frame and the tile ends in order
__global__ __launch_bounds__(kThreads) void pcen_carry_kernel(const float *__restrict__ x, Segs s, Prm p,
                                                              const float *__restrict__ lend, float *__restrict__ carry) {
    const int W = s.width;
    const long long n = s.n_segs * W;
    const float A = p.decay[kTile - 1];
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const long long seg = i / W;
        const int c = int(i - seg * W);
        long long b0, b1, row0;
        if (!s.blk) {
            b0 = seg * s.blocks_per_seg;
            b1 = b0 + s.blocks_per_seg;
            row0 = s.base_row + seg * s.seg_rows;
        } else {
            b0 = s.seg_blk0[seg];
            b1 = s.seg_blk0[seg + 1];
            row0 = b0 < b1 ? s.blk[b0].row0 : 0;
        }
        if (b0 >= b1) continue;                           // a segment without rows
        float C = energy(x[row0 * W + c]);
        const float *pl = lend + b0 * W + c;
        float *pc = carry + b0 * W + c;
        const long long nt = b1 - b0;                      // tiles 0 .. nt - 2 are full
        long long k = 0;
        for (; k + kAhead < nt; k += kAhead) {
            float le[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) le[j] = pl[(k + j) * W];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                pc[(k + j) * W] = C;
                C = __builtin_fmaf(A, C, le[j]);
            }
        }
        for (; k < nt; ++k) {
            pc[k * W] = C;
            if (k + 1 < nt) C = __builtin_fmaf(A, C, pl[k * W]);
        }
    }
}

// y over x, tile by tile; rows outside the segments are not touched
__global__ __launch_bounds__(kThreads) void pcen_apply_kernel(float *__restrict__ x, Segs s, Prm p,
                                                              const float *__restrict__ carry) {
    const int W = s.width, G = tiles_per_group(W), g = threadIdx.x / W, c = threadIdx.x - g * W;
    const long long n_groups = (s.n_blocks + G - 1) / G;
    for (long long j = blockIdx.x; j < n_groups; j += gridDim.x) {
        const long long b = j * G + g;
        if (g >= G || b >= s.n_blocks) continue;
        long long row0, seg;
        int rows;
        tile_of(s, b, row0, rows, seg);
        float *px = x + row0 * W + c;
        const float C = carry[b * W + c];
        float L = 0.0f, M;
        int k0 = 0;
        for (; k0 + kAhead <= rows; k0 += kAhead) {
            float v[kAhead];
#pragma unroll
            for (int i = 0; i < kAhead; ++i) v[i] = px[(k0 + i) * W];
#pragma unroll
            for (int i = 0; i < kAhead; ++i) px[(k0 + i) * W] = element<true>(p, v[i], p.decay[k0 + i], C, L, M);
        }
        for (; k0 < rows; ++k0) px[k0 * W] = element<true>(p, px[k0 * W], p.decay[k0], C, L, M);
    }
}

// ---- the online bank's form (mfcc_hip_bank_create_online_pcen).  State per (stream,
// column): the carry C of the tile in progress and its local smoother L, state[stream][2][W].  The stream's frame
// count `seen` (mirrored on the host) gives the slot of its first fresh row; with seen = 0 nothing of the state is read.
// One OnlineRec (bank_plan.hpp) per stream with fresh rows.
// one thread per (record, column): the fresh rows in order, through element() with the slot's A_k (decay: A_k in HBM,
// the slot differs from lane to lane); L starts from 0 at slot 0, C is latched from M at slot kTile - 1 -- the values
// pcen_carry_kernel and pcen_apply_kernel give the same frames of a one-shot segment
__global__ __launch_bounds__(kThreads) void online_pcen_kernel(const float *raw, float *dst, const OnlineRec *__restrict__ rec,
                                                               long long n_rec, int W, Prm p, const float *__restrict__ decay,
                                                               float *__restrict__ state) {
    const long long n = n_rec * W;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const long long ri = i / W;
        const int c = int(i - ri * W);
        const OnlineRec q = rec[ri];
        const float *px = raw + q.row0 * W + c;
        float *py = dst + q.out_row * W + c;
        float *st = state + q.stream * 2 * W + c;
        float C, L, M;
        if (q.seen == 0) {
            C = energy(px[0]);
            L = 0.0f;
        } else {
            C = st[0];
            L = st[W];
        }
        int k = int(q.seen % kTile);
        for (long long f = 0; f < q.nf; ++f) {
            if (k == 0) L = 0.0f;
            py[f * W] = element<true>(p, px[f * W], decay[k], C, L, M);
            if (++k == kTile) {
                C = M;
                k = 0;
            }
        }
        st[0] = C;
        st[W] = L;
    }
}

}  // namespace mfcc_pcen
