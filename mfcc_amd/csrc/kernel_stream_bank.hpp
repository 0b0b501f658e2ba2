// Stream bank: N independent online sessions advanced by one launch (include/mfcc_hip.h: mfcc_hip_bank_*, DESIGN.md
// section 6c-bis).  These kernels only MOVE samples; the frames are computed by the library's frame kernels, unchanged.
//
// "nfft" below is the handle's frame length in samples: nfft itself on a plain handle, the shorter frame of one made by
// mfcc_hip_create_framed (the kernels take it as their `nfft` argument; it is only the extent of a state row).
// State: one row of nfft int16 per stream in one [n_streams][nfft] allocation.  Element 0 is the pre-emphasis history
// sample x[first - 1] (0 after reset), elements 1 .. 1 + pending are the samples of the frame in progress
// (pending < nfft between calls, so a row always fits).  The host mirrors pending[u]: it depends on lengths only.
//
// A push is planned on the host (bank_plan: total = pending + n_new, nf = frames completed, pending' = total - nf hop)
// and described by one record per stream that received samples, the ACTIVE streams (nf > 0) first, in stream order:
//   bank_advance_kernel, one workgroup per record (grid-stride):
//     active record r:  W[r] = history | pending | new chunk | zeros up to S     (S = 1 + the largest total; a halo-1
//                       channel of the frame kernels: they run ONCE over W as [active] channels of nfmax frames each)
//                       barrier
//                       state = W[r][nf hop .. nf hop + 1 + pending')            (the carry)
//     other records:    state[1 + pending ..] = new chunk                        (the frame is still in progress)
//   The carry's source and destination are the same samples nf hop apart; read from the state row they would overlap
//   whenever nf hop < 1 + pending' (the normal case at 512 / 170).  It therefore goes through W: the state row is only
//   read before the barrier and only written after it, and the part of W it reads was written by this workgroup.
//   bank_flush_kernel: W[r] = history | pending | zeros up to S (the zero-padded tail frame) when W is given, then the
//   stream's history := 0 (the reset state; the host sets pending := 0).
// The copies follow pack_utterances_kernel: the destination is brought to 16-byte alignment, then 16 bytes per lane, the
// source read as it lies (2-byte aligned; global memory takes unaligned vector loads).  Wave64, 256 threads, no LDS.
//
// Cost of a push: the frame kernels compute active x nfmax frames, nfmax = the most frames any stream completes.  With
// equal chunks (N lines in lockstep) that is exactly the frames returned, written straight to the caller's buffer; a
// mixed push pays active x nfmax and a row gather; a straggler pushed alone costs only its own frames.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bank_plan.hpp"                       // Rec, and the plan that fills it

namespace mfcc_bank {

constexpr int kThreads = 256;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(2))) Unaligned16 {
    u32x4 v;
};

// d0[0 .. n) = s0[0 .. n) by the whole workgroup; the ranges do not overlap
__device__ inline void copy_i16(int16_t *d0, const int16_t *s0, long long n) {
    long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(d0) & 15)) & 15) >> 1);
    if (head > n) head = n;
    for (long long i = threadIdx.x; i < head; i += blockDim.x) d0[i] = s0[i];
    const long long nvec = (n - head) >> 3;
    u32x4 *dv = reinterpret_cast<u32x4 *>(d0 + head);
    const Unaligned16 *sv = reinterpret_cast<const Unaligned16 *>(s0 + head);
    for (long long v = threadIdx.x; v < nvec; v += blockDim.x) dv[v] = sv[v].v;
    for (long long i = head + 8 * nvec + threadIdx.x; i < n; i += blockDim.x) d0[i] = s0[i];
}

// d0[0 .. n) = 0
__device__ inline void zero_i16(int16_t *d0, long long n) {
    long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(d0) & 15)) & 15) >> 1);
    if (head > n) head = n;
    for (long long i = threadIdx.x; i < head; i += blockDim.x) d0[i] = 0;
    const long long nvec = (n - head) >> 3;
    u32x4 *dv = reinterpret_cast<u32x4 *>(d0 + head);
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (long long v = threadIdx.x; v < nvec; v += blockDim.x) dv[v] = z;
    for (long long i = head + 8 * nvec + threadIdx.x; i < n; i += blockDim.x) d0[i] = 0;
}

// rec[0 .. n_active): the streams that complete frames, row r of W each; rec[n_active .. n_rec): those that only
// accumulate.  Every stream appears at most once, so a state row belongs to one workgroup.
__global__ __launch_bounds__(kThreads) void bank_advance_kernel(const int16_t *__restrict__ samples, int16_t *state,
                                                                 int16_t *W, const Rec *__restrict__ rec, long long n_rec,
                                                                 long long n_active, long long S, int nfft, int hop) {
    for (long long r = blockIdx.x; r < n_rec; r += gridDim.x) {
        const Rec c = rec[r];
        int16_t *st = state + c.stream * nfft;
        const int16_t *src = samples + c.src;
        if (r >= n_active) {                               // total < nfft: 1 + total samples fit the row
            copy_i16(st + 1 + c.pending, src, c.n_new);
            continue;
        }
        const long long total = c.pending + c.n_new, used = c.nf * hop;
        int16_t *w = W + r * S;
        copy_i16(w, st, 1 + c.pending);
        copy_i16(w + 1 + c.pending, src, c.n_new);
        zero_i16(w + 1 + total, S - 1 - total);
        __syncthreads();                                   // r depends on the workgroup alone: every thread gets here
        copy_i16(st, w + used, 1 + total - used);          // 1 + pending' <= nfft
    }
}

// rec[0 .. n): the streams to put back into the reset state; with W, their tail frames' samples first (row r, S >= nfft + 1)
__global__ __launch_bounds__(kThreads) void bank_flush_kernel(int16_t *state, int16_t *W, const Rec *__restrict__ rec,
                                                               long long n, long long S, int nfft) {
    for (long long r = blockIdx.x; r < n; r += gridDim.x) {
        const Rec c = rec[r];
        int16_t *st = state + c.stream * nfft;
        if (W) {
            int16_t *w = W + r * S;
            copy_i16(w, st, 1 + c.pending);
            zero_i16(w + 1 + c.pending, S - 1 - c.pending);
            __syncthreads();
        }
        if (threadIdx.x == 0) st[0] = 0;
    }
}

}  // namespace mfcc_bank
