// Online stream bank: causal sliding-window CMVN and lagged delta coefficients as device state of a bank
// (include/mfcc_hip.h: mfcc_hip_bank_create_online).  These kernels run after the bank's
// frame launch (kernel_stream_bank.hpp), on the raw rows [active][nfmax][W] it left in the handle's scratch; the MFCC
// kernels and bank_advance_kernel are unchanged.
//
// Frames of a stream are numbered from 0 at create / reset.  Before a push stream u has `seen` rows, the push adds nf
// (rows seen .. seen + nf, the FRESH rows; row0 is the index of the first of them in the launch's buffers).
//
// State per stream:
//   ring  [D][W] raw rows, D = N + S (N the window, S = mfcc_slide::run_rows(N)); row t lives in slot t mod D.  Only
//         with normalization.  Valid for rows [seen - D, seen).
//   tail  [2L][W] static rows (normalized, or raw without normalization), L = K Nd the lag; row t lives in slot
//         t mod 2L.  Only with deltas.  Valid for rows [seen - 2L, seen).
//   Both are rings indexed by the absolute frame number, so nothing is ever moved inside them: the carry writes the
//   fresh rows into slots no other row of the same push maps to (at most D, resp. 2L, of them are written).
//
// online_cmvn_kernel: one thread per (run, column), G = 256 / W runs per workgroup, one record per run.  A run is the
//   rows [t0, t1) of one stream, t0 a multiple of S in ABSOLUTE frame numbers -- the partition the one-shot kernel
//   (kernel_normalize_sliding.hpp) makes of a segment, which starts its float64 sums afresh at every run.  t0 may lie
//   before `seen`: the rows [t0, seen) are recomputed from the ring and not written, so that the sums of the first
//   fresh row have been through exactly the adds and drops they go through in the one-shot call.  The sequence per
//   row is that kernel's: adds in row order, then drops, then the same expressions (standardize below).  Row i is
//   read from the ring if i < seen, else from the fresh rows; the ring is only READ here.
//   The earliest row read is max(0, t0 - N) > seen - S - N = seen - D: inside the ring.
// online_deltas_kernel: one workgroup per (stream, tile of emitted rows [e, e + g)).  Static rows [e - L, e + g + L),
//   clamped to [0, last] (last = the stream's final row during a flush, no edge otherwise: e + g + L <= seen + nf
//   then), go to LDS from tail and fresh rows; with K = 2 the delta rows [e - Nd, e + g + Nd), each computed at its
//   clamped index, too; [s | D | DD] leaves for out_row + (row - e).  The fp32 sequence of an element is that of
//   kernel_deltas.hpp (acc = fma(n, a_n - b_n, acc), n ascending, then acc * r32, nothing contracted).
// online_carry_kernel: one workgroup per stream that got fresh rows, behind the two above in stream order: the last
//   min(nf, D) fresh raw rows into the ring, the last min(nf, 2L) fresh statics into the tail.
// online_deltas_wide_kernel: the same lines over kWideLdsFloats of LDS, for the rows of 65 .. 128 floats of a filterbank
//   bank (mfcc_hip_bank_create_filterbank).  It is the kernel of bank_wide.hip, a code object
//   of its own (MFCC_ONLINE_WIDE_UNIT: this header then gives that kernel and its launcher only); everywhere else the
//   header declares the launcher, launch_deltas_wide.
// Wave64, 256 threads; no atomics; every store is a plain vector store.
//
// What each unit sees of this header:
//   mfcc_hip.hip (MFCC_ONLINE_WIDE_UNIT not defined): Rows .. online_cmvn_kernel, delta_at, the delta kernel's lines as
//     online_deltas_kernel, online_carry_kernel, and the DECLARATION of launch_deltas_wide;
//   bank_wide.hip (MFCC_ONLINE_WIDE_UNIT defined): delta_at, the delta kernel's lines as online_deltas_wide_kernel, and
//     the declaration AND definition of launch_deltas_wide -- nothing of the CMVN or carry kernels, whose host stubs
//     would otherwise be defined twice in the library.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bank_plan.hpp"                                   // Rec (one struct for the three passes), kNoEdge, the tile sizes
#ifndef MFCC_ONLINE_WIDE_UNIT
#include "kernel_normalize_sliding.hpp"
#endif

namespace mfcc_online {

constexpr int kThreads = 256;

#ifndef MFCC_ONLINE_WIDE_UNIT

// column c of a stream's raw rows: the ring below `seen`, the fresh rows from there on
struct Rows {
    const float *ring, *fresh;
    long long seen;
    int D, W;
};
struct Cur {
    long long i;                                           // absolute row
    int slot;                                              // i mod D
};
__device__ __forceinline__ Cur cur_at(const Rows &r, long long i) { return Cur{i, int(i % r.D)}; }
__device__ __forceinline__ float load(const Rows &r, const Cur &c) {
    return c.i < r.seen ? r.ring[(long long)c.slot * r.W] : r.fresh[(c.i - r.seen) * r.W];
}
__device__ __forceinline__ void next(const Rows &r, Cur &c) {
    ++c.i;
    if (++c.slot == r.D) c.slot = 0;
}

// Row value v standardized with the sums u of its window (the adds and drops of the row are done): the expressions of
// normalize_sliding_kernel's row loop from its `finite(v) && u.n > 0` test to `out`, written out again.  (Moving them
// into a function shared with that kernel changed its gfx950 code -- block layout and register numbers -- so it was
// left as it is; tests/test_gpu_stream_bank_online.py holds the two to the same bits.)  n_inv / inv cache 1 / n;
// restart(w) adds the rows of the current window to the fresh sums w, in row order
template <class Restart>
__device__ __forceinline__ float standardize(mfcc_slide::Sums &u, float v, int &n_inv, double &inv, int mode,
                                             Restart restart) {
    using mfcc_slide::kStale;
    using mfcc_slide::Sums;
    float out = v;
    if (mfcc_norm::finite(v) && u.n > 0) {
        if (u.n != n_inv) {                                             // n rarely changes from row to row
            n_inv = u.n;
            inv = 1.0 / double(u.n);
        }
        double m = u.s * inv, var = u.q * inv - m * m;
        if (var < kStale * u.d2max * inv) {                             // stale sums (see kStale): start over
            u = Sums{0.0, 0.0, 0.0, 0.0, 0, false};
            restart(u);
            m = u.s * inv;                                              // n is what it was
            var = u.q * inv - m * m;
        }
        float r32 = 1.0f;
        if (mode == 2) {
            double sd = var > 0.0 ? sqrt(var) : 0.0;
            if (sd < 10.0 * 2.220446049250313e-16) sd = 1.0;
            r32 = float(1.0 / sd);
        }
        out = (v - float(u.p + m)) * r32;
    }
    return out;
}

// mode: 1 = mean only, 2 = mean and variance
__global__ __launch_bounds__(kThreads) void online_cmvn_kernel(const float *__restrict__ ring,
                                                                const float *__restrict__ fresh, float *__restrict__ y,
                                                                const Rec *__restrict__ rec, long long n_rec, int W, int N,
                                                                int D, int mode) {
    using namespace mfcc_slide;
    const int G = kThreads / W, t = threadIdx.x, g = t / W, c = t - g * W;
    if (g >= G) return;
    const long long n_blk = (n_rec + G - 1) / G;
    for (long long b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const long long ri = b * G + g;
        if (ri >= n_rec) continue;
        const Rec q = rec[ri];
        const Rows rows{ring + q.stream * D * W + c, fresh + q.row0 * W + c, q.seen, D, W};
        float *py = y + q.out_row * W + c;
        Sums u{0.0, 0.0, 0.0, 0.0, 0, false};
        long long wa, wb;
        window_of(q.t0, kNoEdge, N, 1, 0, wa, wb);
        Cur ca = cur_at(rows, wa), cb = ca, cx = cur_at(rows, q.t0);    // next row to drop, to add, to normalize
        // the first window, four loads in flight; the order of the additions is the rows'
        while (cb.i + 4 <= wb) {
            const float v0 = load(rows, cb);
            next(rows, cb);
            const float v1 = load(rows, cb);
            next(rows, cb);
            const float v2 = load(rows, cb);
            next(rows, cb);
            const float v3 = load(rows, cb);
            next(rows, cb);
            add(u, v0);
            add(u, v1);
            add(u, v2);
            add(u, v3);
        }
        int n_inv = 0;
        double inv = 0.0;
        for (long long r = q.t0; r < q.cnt; ++r) {
            window_of(r, kNoEdge, N, 1, 0, wa, wb);
            const float v = load(rows, cx);
            next(rows, cx);
            for (; cb.i < wb; next(rows, cb)) add(u, load(rows, cb));
            for (; ca.i < wa; next(rows, ca)) drop(u, load(rows, ca));
            const float out = standardize(u, v, n_inv, inv, mode, [&](Sums &w) {
                for (Cur cr = ca; cr.i < cb.i; next(rows, cr)) add(w, load(rows, cr));
            });
            if (r >= q.seen) py[(r - q.seen) * W] = out;
        }
    }
}

#endif  // MFCC_ONLINE_WIDE_UNIT

// the delta of column c of the row at src (rows W floats apart; the rows N above and below are there, already clamped)
__device__ __forceinline__ float delta_at(const float *src, int W, int N, float r32) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    for (int k = 1; k <= N; ++k) acc = __builtin_fmaf(float(k), src[k * W] - src[-k * W], acc);
    return acc * r32;
}

// The delta kernel: these lines are compiled once per unit -- as online_deltas_kernel over kLdsFloats in the MFCC
// kernels' unit, as online_deltas_wide_kernel over kWideLdsFloats in bank_wide.hip.  (As a function that two kernels
// inline -- the tile its own as a template on the size, or handed to it -- the same lines gave the narrow kernel other
// gfx950 code: instruction order and register numbers.  This way its code is what it was.)  Every record fits its
// kernel's LDS: bank_plan.hpp, tile_rows / wide_tile_rows
#ifdef MFCC_ONLINE_WIDE_UNIT
#define MFCC_ONLINE_DELTAS_KERNEL online_deltas_wide_kernel
#define MFCC_ONLINE_DELTAS_LDS kWideLdsFloats
#else
#define MFCC_ONLINE_DELTAS_KERNEL online_deltas_kernel
#define MFCC_ONLINE_DELTAS_LDS kLdsFloats
#endif
__global__ __launch_bounds__(kThreads) void MFCC_ONLINE_DELTAS_KERNEL(const float *__restrict__ tail,
                                                                       const float *__restrict__ fresh, float *__restrict__ y,
                                                                       const Rec *__restrict__ rec, long long n_rec, int W,
                                                                       int K, int N, float r32) {
    __shared__ float lds[MFCC_ONLINE_DELTAS_LDS];
    const int L = K * N, L2 = 2 * L, WO = W * (1 + K), t = threadIdx.x;
    for (long long b = blockIdx.x; b < n_rec; b += gridDim.x) {
        const Rec q = rec[b];
        const long long e = q.t0;
        const int g = int(q.cnt), ns = g + L2;
        const float *tl = tail + q.stream * L2 * W, *fr = fresh + q.row0 * W;
        float *sx = lds;                                               // static rows e - L .. e + g + L
        float *sd = lds + ns * W;                                      // D rows e - N .. e + g + N (K = 2)
        for (int i = t; i < ns * W; i += kThreads) {
            const int v = i / W, c = i - v * W;
            long long row = e - L + v;
            row = row < 0 ? 0 : (row > q.last ? q.last : row);
            sx[i] = row < q.seen ? tl[(row % L2) * W + c] : fr[(row - q.seen) * W + c];
        }
        __syncthreads();
        float *o = y + q.out_row * WO;
        if (K == 2) {
            for (int i = t; i < (g + 2 * N) * W; i += kThreads) {
                const int v = i / W, c = i - v * W;
                long long row = e - N + v;                             // D row v, computed at its clamped index
                row = row < 0 ? 0 : (row > q.last ? q.last : row);
                const float d = delta_at(sx + int(row - (e - L)) * W + c, W, N, r32);
                sd[i] = d;
                const int rt = v - N;                                  // row of the tile, if it is one
                if (rt >= 0 && rt < g) {
                    o[(long long)rt * WO + c] = sx[(rt + L) * W + c];
                    o[(long long)rt * WO + W + c] = d;
                }
            }
            __syncthreads();
            for (int i = t; i < g * W; i += kThreads) {
                const int v = i / W, c = i - v * W;
                o[(long long)v * WO + 2 * W + c] = delta_at(sd + (v + N) * W + c, W, N, r32);
            }
        } else {
            for (int i = t; i < g * W; i += kThreads) {
                const int v = i / W, c = i - v * W;
                o[(long long)v * WO + c] = sx[(v + L) * W + c];
                o[(long long)v * WO + W + c] = delta_at(sx + (v + L) * W + c, W, N, r32);
            }
        }
        __syncthreads();                                               // the next tile overwrites the LDS
    }
}

#undef MFCC_ONLINE_DELTAS_KERNEL
#undef MFCC_ONLINE_DELTAS_LDS

#ifndef MFCC_ONLINE_WIDE_UNIT

// ring / tail may be null (no normalization / no deltas); stat = the fresh static rows (raw without normalization)
__global__ __launch_bounds__(kThreads) void online_carry_kernel(float *ring, float *tail, const float *__restrict__ raw,
                                                                 const float *__restrict__ stat, const Rec *__restrict__ rec,
                                                                 long long n_rec, int W, int D, int L2) {
    for (long long b = blockIdx.x; b < n_rec; b += gridDim.x) {
        const Rec q = rec[b];
        if (ring) {
            const long long k = q.nf < D ? q.nf : D, f0 = q.nf - k;    // the last k fresh rows: distinct slots
            float *dst = ring + q.stream * D * W;
            const float *src = raw + (q.row0 + f0) * W;
            for (long long i = threadIdx.x; i < k * W; i += kThreads) {
                const long long v = i / W, c = i - v * W;
                dst[((q.seen + f0 + v) % D) * W + c] = src[i];
            }
        }
        if (tail) {
            const long long k = q.nf < L2 ? q.nf : L2, f0 = q.nf - k;
            float *dst = tail + q.stream * L2 * W;
            const float *src = stat + (q.row0 + f0) * W;
            for (long long i = threadIdx.x; i < k * W; i += kThreads) {
                const long long v = i / W, c = i - v * W;
                dst[((q.seen + f0 + v) % L2) * W + c] = src[i];
            }
        }
    }
}

#endif  // MFCC_ONLINE_WIDE_UNIT

// online_deltas_wide_kernel over `blocks` workgroups on `stream`; the arguments are online_deltas_kernel's
void launch_deltas_wide(const float *tail, const float *fresh, float *y, const Rec *rec, long long n_rec, int W, int K, int N,
                        float r32, unsigned blocks, hipStream_t stream);

#ifdef MFCC_ONLINE_WIDE_UNIT

void launch_deltas_wide(const float *tail, const float *fresh, float *y, const Rec *rec, long long n_rec, int W, int K, int N,
                        float r32, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(online_deltas_wide_kernel, dim3(blocks), dim3(kThreads), 0, stream, tail, fresh, y, rec, n_rec, W, K, N,
                       r32);
}

#endif  // MFCC_ONLINE_WIDE_UNIT

}  // namespace mfcc_online
