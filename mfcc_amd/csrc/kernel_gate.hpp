// The receiver's power gate and window extraction on int16 rows already in HBM (include/mfcc_hip.h: mfcc_hip_gate_dev /
// mfcc_hip_gate_windows_dev / mfcc_hip_gate_*, DESIGN.md sections 4.10 and 6c-quater).  Passes after the fixed-point
// frame kernels, not a change to them.
//
// rows: int16 [R][n_cep], n_cep = 1..64.  Window j of a segment of T rows is rows [j stride, j stride + n_frames) of it;
// its power is the sum of the squares of column c0 of its frames f0 .. f0 + K - 1 (Geo: the closed form of the
// reference's loop `for (i = size / 3; i < 2 * size / 3; i += n_cep)` on a linear window).  Everything is integer
// arithmetic: a square is at most 2^30, a sum at most 1366 * 2^30 < 2^41, so int64 sums are exact in any order.
//
// The tiles are those of kernel_normalize.hpp (Segs / tile_of / BlockRec) laid over the WINDOW index space: a "row" of
// Segs is a window, a tile a run of consecutive windows of one segment.  Wins adds what maps a window to its first row:
// delta[seg] = (first row of the segment) - (first window of the segment) * stride, so that global window w starts at
// row delta[seg] + w * stride.
//   gate_power_kernel   per tile of nw windows: the squares of column c0 of the (nw - 1) stride + K frames the tile's
//                       sums cover go to LDS as int64 (each value is read from HBM once per tile, nothing outside the
//                       segment is read), an exclusive prefix sum is formed in place (every thread scans a contiguous
//                       run, the run sums are prefixed with wave shuffles and across the four waves through LDS), and
//                       window j's power is pre[j stride + K] - pre[j stride]: two LDS reads per window whatever K is.
//   gate_gather_kernel  the selection's third pass (counts and prefix are mfcc_vad::vad_count_kernel / vad_scan_kernel
//                       on the mask, unchanged): per tile the rank of every kept window from ballots, then one wave per
//                       kept window copies its n_frames * n_cep int16 -- ONE contiguous run in the source and in the
//                       destination -- in the widest unit (16, 8, 4 or 2 bytes) the two addresses share, 2-byte head
//                       and tail, and writes the window's first row to `starts`.
// The tracker (N live lines, state on the device: a ring [D][n_cep] per line, D = n_frames + stride - 1, row t in slot
// t mod D, indexed by the absolute frame number like the rings of kernel_stream_bank_online.hpp):
//   gate_live_kernel    one thread per completed window: its K squares in int64; frame i comes from the ring if
//                       i < seen, else from the fresh rows (the access rule of online_cmvn_kernel).  The ring is only read.
//   gate_carry_kernel   behind it on the same stream: the last min(nf, D) fresh rows into their slots (one row per slot)
//   gate_window_kernel  ring -> [n][n_frames][n_cep]
// Wave64, 256 threads; no atomics; every store is a plain vector store.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_normalize.hpp"

namespace mfcc_gate {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWidth = 64;
constexpr int kMaxWindow = 4096;        // n_frames and stride
constexpr int kSpan = 4096;             // squares a power tile stages: 32 KB of LDS as int64 (four workgroups per CU)
constexpr int kMaxTileWins = 1024;      // windows per power tile at most
constexpr int kSelTileWins = 1024;      // windows per tile of the selection (the mask bytes a count / gather tile reads)

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

using mfcc_norm::Segs;

// the elements the reference's loop visits: column c0 of frames f0 .. f0 + K - 1 of a linear window
struct Geo {
    int n_cep, n_frames, stride, K, f0, c0;
};

__host__ __device__ inline Geo geometry(int n_cep, int n_frames, int stride) {
    const int size = n_frames * n_cep, first = size / 3, last = 2 * size / 3;     // at most 4096 * 64
    return Geo{n_cep, n_frames, stride, (last - first + n_cep - 1) / n_cep, first / n_cep, first % n_cep};
}

// windows per power tile: the most whose span (tile - 1) stride + K fits kSpan, 1024 at most.  K <= 1366 < kSpan: at
// least one.  A function of K and stride alone
__host__ __device__ inline int power_tile_wins(int K, int stride) {
    const int t = (kSpan - K) / stride + 1;
    return t < kMaxTileWins ? t : kMaxTileWins;
}

// Segs over the window index space plus the first row of every segment's windows.  Uniform form (delta == nullptr):
// segment k is rows [base_row + k seg_rows, + seg_rows) and has s.seg_rows windows
struct Wins {
    Segs s;
    const long long *delta;
    long long base_row, seg_rows;
};

// first row of global window w of segment seg
__device__ __forceinline__ long long first_row(const Wins &w, long long seg, long long win, int stride) {
    const long long d = w.delta ? w.delta[seg] : w.base_row + seg * (w.seg_rows - w.s.seg_rows * stride);
    return d + win * stride;
}

__global__ __launch_bounds__(kThreads) void gate_power_kernel(const int16_t *__restrict__ x, Wins w, Geo g,
                                                              long long threshold, long long *__restrict__ power,
                                                              unsigned char *__restrict__ gate,
                                                              unsigned char *__restrict__ gate_ref) {
    __shared__ long long pre[kSpan + 8];
    __shared__ long long wtot[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long b = blockIdx.x; b < w.s.n_blocks; b += gridDim.x) {
        long long win0, seg;
        int nw;
        mfcc_norm::tile_of(w.s, b, win0, nw, seg);
        // entry i is frame f0 + i of the tile's first window; the last one read is the last summed frame of its last
        const int16_t *col = x + (first_row(w, seg, win0, g.stride) + g.f0) * g.n_cep + g.c0;
        const int span = (nw - 1) * g.stride + g.K;
        for (int i = t; i <= span; i += kThreads) {
            long long sq = 0;                                     // entry `span` is the slot of the total
            if (i < span) {
                const int v = col[(long long)i * g.n_cep];
                sq = (long long)(v * v);
            }
            pre[i] = sq;
        }
        __syncthreads();
        // exclusive prefix in place: thread t owns entries [a, e)
        const int per = (span + kThreads) / kThreads;
        const int a = t * per < span + 1 ? t * per : span + 1, e = a + per < span + 1 ? a + per : span + 1;
        long long sum = 0;
        for (int i = a; i < e; ++i) sum += pre[i];
        long long inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        long long acc = inc - sum;
        for (int k = 0; k < wave; ++k) acc += wtot[k];
        for (int i = a; i < e; ++i) {
            const long long v = pre[i];
            pre[i] = acc;
            acc += v;
        }
        __syncthreads();
        for (int j = t; j < nw; j += kThreads) {
            const long long p = pre[j * g.stride + g.K] - pre[j * g.stride];
            const long long o = win0 + j;
            if (power) power[o] = p;
            if (gate) gate[o] = p >= threshold ? 1 : 0;
            if (gate_ref) gate_ref[o] = (long long)(int)(unsigned)p >= threshold ? 1 : 0;
        }
        __syncthreads();           // the next tile overwrites pre and wtot
    }
}

// n int16 from s to d by the 64 lanes of a wave: the body in units of T where both addresses are aligned to it (the
// caller has checked that s - d is a multiple of sizeof(T)), 2-byte head and tail
template <typename T>
__device__ __forceinline__ void copy_as(const int16_t *__restrict__ s, int16_t *__restrict__ d, long long n, int lane) {
    constexpr int kPer = int(sizeof(T) / sizeof(int16_t));
    const long long mis = (long long)((sizeof(T) - (reinterpret_cast<uintptr_t>(d) & (sizeof(T) - 1))) & (sizeof(T) - 1)) / 2;
    const long long head = mis < n ? mis : n, nv = (n - head) / kPer;
    const T *sv = reinterpret_cast<const T *>(s + head);
    T *dv = reinterpret_cast<T *>(d + head);
    for (long long i = lane; i < nv; i += 64) dv[i] = sv[i];
    if (lane < head) d[lane] = s[lane];                           // head < 8
    for (long long i = head + nv * kPer + lane; i < n; i += 64) d[i] = s[i];
}

__device__ __forceinline__ void copy_run(const int16_t *__restrict__ s, int16_t *__restrict__ d, long long n, int lane) {
    const unsigned rel = unsigned(reinterpret_cast<uintptr_t>(s) - reinterpret_cast<uintptr_t>(d)) & 15u;   // wave-uniform
    if (rel == 0)
        copy_as<u32x4>(s, d, n, lane);
    else if ((rel & 7u) == 0)
        copy_as<u32x2>(s, d, n, lane);
    else if ((rel & 3u) == 0)
        copy_as<unsigned>(s, d, n, lane);
    else
        for (long long i = lane; i < n; i += 64) d[i] = s[i];
}

// tile_off: vad_scan_kernel's exclusive prefix of the tiles' kept windows
__global__ __launch_bounds__(kThreads) void gate_gather_kernel(const int16_t *__restrict__ x,
                                                               const unsigned char *__restrict__ mask, Wins w, Geo g,
                                                               const long long *__restrict__ tile_off,
                                                               int16_t *__restrict__ y, long long *__restrict__ starts) {
    __shared__ unsigned short src[kSelTileWins];                  // src[q]: the tile window of the tile's q-th kept window
    __shared__ unsigned wtot[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long L = (long long)g.n_frames * g.n_cep;
    for (long long b = blockIdx.x; b < w.s.n_blocks; b += gridDim.x) {
        long long win0, seg;
        int nw;
        mfcc_norm::tile_of(w.s, b, win0, nw, seg);
        const long long out0 = tile_off[b];
        const int cnt = int(tile_off[b + 1] - out0);
        if (cnt == 0) continue;                                   // the whole workgroup: nothing of this tile is kept
        int run = 0;
        for (int base = 0; base < nw; base += kThreads) {
            const int r = base + t;
            const bool v = r < nw && mask[win0 + r] != 0;
            const unsigned long long m = __ballot(v);
            if (lane == 0) wtot[wave] = unsigned(__popcll(m));
            __syncthreads();
            int pre = run, tot = 0;
            for (int k = 0; k < kWaves; ++k) {
                if (k < wave) pre += int(wtot[k]);
                tot += int(wtot[k]);
            }
            if (v) src[pre + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)r;
            run += tot;
            __syncthreads();       // wtot is rewritten; src is complete after the last round
        }
        const int n = run < cnt ? run : cnt;                      // run == cnt: the counts are those of this mask
        for (int q = wave; q < n; q += kWaves) {
            const long long row = first_row(w, seg, win0 + src[q], g.stride);
            copy_run(x + row * g.n_cep, y + (out0 + q) * L, L, lane);
            if (starts && lane == 0) starts[out0 + q] = row;
        }
        __syncthreads();           // the next tile overwrites src
    }
}

// ---- the tracker ----------------------------------------------------------------------------------------------------
// One record per line that got fresh rows: the nf rows [seen, seen + nf) of `line` are rows row0 .. of the fresh buffer;
// they complete windows j0 .. j0 + nwin - 1 of the line, whose results go to entries out0 .. of the outputs
struct Rec {
    long long line, row0, seen, nf, j0, nwin, out0, pad;
};
constexpr int kRecLL = 8;                                  // a record as long longs in the pinned descriptor pool

// thread (record r, k) for k < nwmax, the most windows any line completes
__global__ __launch_bounds__(kThreads) void gate_live_kernel(const int16_t *__restrict__ ring,
                                                             const int16_t *__restrict__ fresh,
                                                             const Rec *__restrict__ rec, long long n_rec, long long nwmax,
                                                             Geo g, int D, long long threshold,
                                                             long long *__restrict__ power, unsigned char *__restrict__ gate,
                                                             unsigned char *__restrict__ gate_ref) {
    const long long total = n_rec * nwmax;
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (long long)gridDim.x * kThreads) {
        const long long r = idx / nwmax, k = idx - r * nwmax;
        const Rec q = rec[r];
        if (k >= q.nwin) continue;
        const int16_t *rg = ring + q.line * D * g.n_cep + g.c0, *fr = fresh + q.row0 * g.n_cep + g.c0;
        long long i = (q.j0 + k) * g.stride + g.f0;                // absolute frame; > seen - D (the window is incomplete at seen)
        int slot = int(i % D);
        long long p = 0;
        for (int kk = 0; kk < g.K; ++kk, ++i) {
            const int v = i < q.seen ? rg[(long long)slot * g.n_cep] : fr[(i - q.seen) * g.n_cep];
            p += (long long)(v * v);
            if (++slot == D) slot = 0;
        }
        const long long o = q.out0 + k;
        if (power) power[o] = p;
        if (gate) gate[o] = p >= threshold ? 1 : 0;
        if (gate_ref) gate_ref[o] = (long long)(int)(unsigned)p >= threshold ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void gate_carry_kernel(int16_t *__restrict__ ring, const int16_t *__restrict__ fresh,
                                                              const Rec *__restrict__ rec, long long n_rec, int n_cep, int D) {
    for (long long r = blockIdx.x; r < n_rec; r += gridDim.x) {
        const Rec q = rec[r];
        const long long m = q.nf < D ? q.nf : D, t0 = q.seen + q.nf - m;     // rows [t0, seen + nf): one per slot
        int16_t *rg = ring + q.line * D * n_cep;
        const int16_t *fr = fresh + (q.row0 + (t0 - q.seen)) * n_cep;
        const int n = int(m) * n_cep;
        for (int e = threadIdx.x; e < n; e += kThreads) {
            const int rr = e / n_cep, c = e - rr * n_cep;
            rg[((t0 + rr) % D) * n_cep + c] = fr[e];
        }
    }
}

// entry i: rows [start, start + n_frames) of `line` from its ring to y[i]
struct WinRec {
    long long line, start;
};

__global__ __launch_bounds__(kThreads) void gate_window_kernel(const int16_t *__restrict__ ring,
                                                               const WinRec *__restrict__ rec, long long n, Geo g, int D,
                                                               int16_t *__restrict__ y) {
    const int L = g.n_frames * g.n_cep;
    for (long long r = blockIdx.x; r < n; r += gridDim.x) {
        const WinRec q = rec[r];
        const int16_t *rg = ring + q.line * D * g.n_cep;
        for (int e = threadIdx.x; e < L; e += kThreads) {
            const int rr = e / g.n_cep, c = e - rr * g.n_cep;
            y[r * L + e] = rg[((q.start + rr) % D) * g.n_cep + c];
        }
    }
}

}  // namespace mfcc_gate
