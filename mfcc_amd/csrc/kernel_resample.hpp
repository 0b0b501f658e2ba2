// Sample-rate conversion (include/mfcc_hip.h: "sample rates"): the integer polyphase rule on the
// device.  The rule's integers and the tap table are resample_plan.hpp's, the same lines for the host
// (mfcc_hip_resample_host) and for this kernel.
//
// resample_rows_kernel / resample_segs_kernel<STAGED>: a workgroup of 256 lanes takes a tile of 2048 consecutive output slots of one segment, a
// lane 8 of them, stored with one 16-byte store.  The OUTPUT decides the alignment: slot 0 of a segment is the 16-byte
// boundary at or in front of its first output, so the first and the last group of a segment may be partly empty and
// go out one sample at a time.  STAGED: the samples the tile reads are copied to LDS first, with 16-byte loads where
// the whole group lies inside [0, n) and zeros outside it, so the tap loop has no bounds test.  It takes two taps per
// v_dot2c_i32_i16 (__builtin_amdgcn_sdot2): the tap pair is one aligned dword of the table, the sample pair is cut
// from two neighbouring LDS dwords with v_alignbit_b32, by 0 or 16 bits for an even or odd first sample.  !STAGED: a
// ratio whose tile does not fit kMaxSpan samples reads global memory with a bounds test per tap.  TLDS: the workgroup
// copies the tap table to LDS once, in front of the samples, where both fit (resample_plan.hpp: taps_in_lds); else
// the tap dwords come from global memory through the caches.
// The tile's first (q, p) is 64-bit, once per tile; everything behind it 32-bit.  Nothing outside [in, in + n) of a
// segment is read, nothing outside [out, out + n_out) written.  No atomics.
// A line of a live stream (mfcc_hip_resampler) is a segment with K - 1 samples of history in front of its chunk; the
// same launch writes the next history into the line's other buffer (a tile of its own in the list), so no workgroup
// reads what another writes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resample_plan.hpp"

namespace mfcc_rs {

struct Taps {
    const int16_t *t;          // L rows of K taps, on the device
    int L, M, H, K;
};

// One launch.  rows > 0 equal rows (row r reads in + r * in_stride, n samples, and writes out + r * out_stride, n_out
// samples), or, with recs, the segments and tiles of a CallPlan at d_recs (in, out and the strides unused).  in and
// out aligned to 2 bytes.  The kernels and this function are compiled in a translation unit of their own
// (resample.hip defines MFCC_RESAMPLE_DEFINE_KERNELS), a code object of their own.
void launch(const Taps &a, const int16_t *in, long long n, int16_t *out, long long n_out, long long rows, long long in_stride,
            long long out_stride, const long long *d_recs, long long n_tiles, int n_cu, hipStream_t stream);

#ifdef MFCC_RESAMPLE_DEFINE_KERNELS

typedef unsigned int rs_u32x4 __attribute__((ext_vector_type(4)));
typedef short rs_s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ rs_s16x2 as_pair(unsigned w) {
    union {
        unsigned u;
        rs_s16x2 v;
    } c;
    c.u = w;
    return c.v;
}

// a segment (resample_plan.hpp: SegIn) as the kernel holds it
struct Seg {
    const int16_t *in;
    long long n;
    int16_t *out;
    long long m0, m1, c0;
    const int16_t *hist;
    int16_t *hist_new;
};

// sample i of the chunk: the chunk itself, its history in front of it, zeros elsewhere
__device__ __forceinline__ unsigned sample_at(const Seg &g, long long i, int K) {
    if (i >= 0) return i < g.n ? unsigned(uint16_t(g.in[i])) : 0u;
    return g.hist && i >= 1 - K ? unsigned(uint16_t(g.hist[i + K - 1])) : 0u;
}

// the history tile of a segment: the K - 1 samples in front of the chunk's end, into the line's other buffer (the
// tiles of this launch read the old one)
__device__ __forceinline__ void resample_history(const Taps &a, const Seg &g) {
    for (int j = threadIdx.x; j < a.K - 1; j += kThreads) g.hist_new[j] = int16_t(sample_at(g, g.n - (a.K - 1) + j, a.K));
}

// tile t of a segment.  TLDS: the table lies in LDS at lt (the kernel put it there), else it is read from a.t
template <bool STAGED, bool TLDS>
__device__ __forceinline__ void resample_tile(const Taps &a, const Seg &sg, long long t, int16_t *lds, const int16_t *lt) {
    const int16_t *__restrict__ in = sg.in;
    int16_t *__restrict__ out = sg.out;
    const long long n = sg.n;
    const int lead = lead_of(reinterpret_cast<uintptr_t>(out)), tid = threadIdx.x;
    const TileSpan sp = tile_span(t, lead, sg.m0, sg.m1, sg.c0, reinterpret_cast<uintptr_t>(in), a.L, a.M, a.H);
    const long long ma = sp.ma, mb = sp.mb, base = STAGED ? sp.base : 0;
    if (ma >= mb) return;                                              // the whole workgroup
    const long long qa = phase_q(sg.m0 + ma, a.L, a.M) - sg.c0;          // in samples of the chunk
    const unsigned pa = unsigned(phase_p(sg.m0 + ma, a.L, a.M));
    if (STAGED) {
        const int groups = sp.groups;
        for (int g = tid; g < groups; g += kThreads) {
            const long long i0 = base + 8ll * g;
            rs_u32x4 v;
            if (i0 >= 0 && i0 + 8 <= n) {
                v = *reinterpret_cast<const rs_u32x4 *>(in + i0);
            } else {
                unsigned s[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] = sample_at(sg, i0 + k, a.K);
                v.x = s[0] | s[1] << 16; v.y = s[2] | s[3] << 16; v.z = s[4] | s[5] << 16; v.w = s[6] | s[7] << 16;
            }
            reinterpret_cast<rs_u32x4 *>(lds)[g] = v;
        }
        __syncthreads();
    }
    const long long m_first = t * kTile - lead + 8ll * tid;
    const int s_base = int(qa - a.H + 1 - base);                       // STAGED: the LDS index of x[qa - H + 1]
    const int half = a.K >> 1;
    int y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        long long m = m_first + j;
        if (m < ma || m >= mb) m = ma;                                 // an empty slot: computed, not stored
        const unsigned x = pa + unsigned(m - ma) * unsigned(a.M), dq = x / unsigned(a.L), p = x - dq * unsigned(a.L);
        int acc = 0;
        if (STAGED) {
            const int s = s_base + int(dq);
            const unsigned *w = reinterpret_cast<const unsigned *>(lds) + (s >> 1);
            const unsigned sh = (s & 1) << 4;
            auto mac = [&](const unsigned *tw) {
                unsigned w0 = w[0];
                for (int kk = 0; kk < half; ++kk) {
                    const unsigned w1 = w[kk + 1];
                    acc = __builtin_amdgcn_sdot2(as_pair(tw[kk]), as_pair(__builtin_amdgcn_alignbit(w1, w0, sh)), acc, false);
                    w0 = w1;
                }
            };
            if (TLDS) mac(reinterpret_cast<const unsigned *>(lt + size_t(p) * a.K));
            else mac(reinterpret_cast<const unsigned *>(a.t + size_t(p) * a.K));
        } else {
            const long long first = qa + (long long)dq - a.H + 1;
            const int16_t *tp = a.t + size_t(p) * a.K;
            for (int k = 0; k < a.K; ++k) acc += int(tp[k]) * int(int16_t(sample_at(sg, first + k, a.K)));
        }
        y[j] = finish(acc);
    }
    if (m_first >= ma && m_first + 8 <= mb) {
        rs_u32x4 v;
        v.x = (unsigned(y[0]) & 0xffffu) | unsigned(y[1]) << 16;
        v.y = (unsigned(y[2]) & 0xffffu) | unsigned(y[3]) << 16;
        v.z = (unsigned(y[4]) & 0xffffu) | unsigned(y[5]) << 16;
        v.w = (unsigned(y[6]) & 0xffffu) | unsigned(y[7]) << 16;
        *reinterpret_cast<rs_u32x4 *>(out + m_first) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (m_first + j >= ma && m_first + j < mb) out[m_first + j] = int16_t(y[j]);
    }
    if (STAGED) __syncthreads();                                       // the next tile of the grid loop restages
}

// equal rows: x strides over the tiles of a row, y over the rows
// TLDS: the workgroup copies the table to the front of its LDS once; the samples are staged behind it
template <bool TLDS>
__device__ __forceinline__ int16_t *stage_taps(const Taps &a, int16_t *lds) {
    if (!TLDS) return lds;
    const int words = a.L * a.K >> 1;
    for (int i = threadIdx.x; i < words; i += kThreads)
        reinterpret_cast<unsigned *>(lds)[i] = reinterpret_cast<const unsigned *>(a.t)[i];
    __syncthreads();
    return lds + taps_lds_samples(a.L, a.K);
}

template <bool STAGED, bool TLDS>
__global__ __launch_bounds__(kThreads) void resample_rows_kernel(Taps a, const int16_t *__restrict__ in, long long n,
                                                                 int16_t *__restrict__ out, long long n_out, long long rows,
                                                                 long long in_stride, long long out_stride) {
    extern __shared__ __attribute__((aligned(16))) int16_t rs_lds[];
    int16_t *span = stage_taps<TLDS>(a, rs_lds);
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const Seg g{in + r * in_stride, n, out + r * out_stride, 0, n_out, 0, nullptr, nullptr};
        const long long tiles = tiles_of(n_out, lead_of(reinterpret_cast<uintptr_t>(g.out)));
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) resample_tile<STAGED, TLDS>(a, g, t, span, rs_lds);
    }
}

// the segments of a CallPlan: x strides over its tile list
template <bool STAGED, bool TLDS>
__global__ __launch_bounds__(kThreads) void resample_segs_kernel(Taps a, const long long *__restrict__ recs, long long tile_off_ll,
                                                                 long long n_tiles) {
    extern __shared__ __attribute__((aligned(16))) int16_t rs_lds[];
    int16_t *span = stage_taps<TLDS>(a, rs_lds);
    for (long long i = blockIdx.x; i < n_tiles; i += gridDim.x) {
        const long long *tr = recs + tile_off_ll + i * kTileLL, *sr = recs + tr[0] * kSegLL;
        const Seg g{reinterpret_cast<const int16_t *>(sr[0]), sr[1], reinterpret_cast<int16_t *>(sr[2]), sr[3], sr[4], sr[5],
                    reinterpret_cast<const int16_t *>(sr[6]), reinterpret_cast<int16_t *>(sr[7])};
        if (tr[1] == kHistoryTile) resample_history(a, g);
        else resample_tile<STAGED, TLDS>(a, g, tr[1], span, rs_lds);
    }
}

void launch(const Taps &a, const int16_t *in, long long n, int16_t *out, long long n_out, long long rows, long long in_stride,
            long long out_stride, const long long *d_recs, long long n_tiles, int n_cu, hipStream_t stream) {
    const bool st = staged(a.L, a.M, a.K), tl = taps_in_lds(a.L, a.M, a.K);
    const size_t lds = lds_bytes(a.L, a.M, a.K);
    const dim3 block(kThreads);
    unsigned gx, gy;
    if (d_recs) {
        const long long tile_off_ll = rows * kSegLL;                   // rows: the segments in front of the tile list
        grid(n_tiles, 1, n_cu, gx, gy);
        const dim3 g(gx);
        if (tl) hipLaunchKernelGGL((resample_segs_kernel<true, true>), g, block, lds, stream, a, d_recs, tile_off_ll, n_tiles);
        else if (st) hipLaunchKernelGGL((resample_segs_kernel<true, false>), g, block, lds, stream, a, d_recs, tile_off_ll, n_tiles);
        else hipLaunchKernelGGL((resample_segs_kernel<false, false>), g, block, 0, stream, a, d_recs, tile_off_ll, n_tiles);
        return;
    }
    grid(tiles_of(n_out, 7), rows, n_cu, gx, gy);
    const dim3 g(gx, gy);
#define MFCC_RS_ROWS(S, T, B) \
    hipLaunchKernelGGL((resample_rows_kernel<S, T>), g, block, B, stream, a, in, n, out, n_out, rows, in_stride, out_stride)
    if (tl) MFCC_RS_ROWS(true, true, lds);
    else if (st) MFCC_RS_ROWS(true, false, lds);
    else MFCC_RS_ROWS(false, false, 0);
#undef MFCC_RS_ROWS
}

#endif  // MFCC_RESAMPLE_DEFINE_KERNELS

}  // namespace mfcc_rs
