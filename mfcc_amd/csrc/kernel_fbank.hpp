// The filterbank output (include/mfcc_hip.h: "filterbank"): rows of n_bands <= 128 values
// E[j] = sum_k W[j][k] P[k] (or c * log2(max(E, floor))) with the caller's matrix W and P the power-spectrum row of
// kernel_spectrum.hpp, contracted before anything leaves the chip.
//
//   mfcc_fbank512_kernel<HOP, LOG, WLDS>  nfft 512 at hop 170 (full frame) and hop 160 (any frame of 160 .. 512 samples)
//   mfcc_fbank_generic_kernel<N, LOG>     every other handle, and 512 too under MFCC_HIP_IMPL_GENERIC
//
// fbank_plan.hpp decides which one a handle runs and builds the table both read: the weights of every band from its
// first to its last non-zero bin, packed band after band, and per band (first bin, bins, offset into the packed
// weights).  The generic kernel and the fused one's fp32 form sum fmaf(W[j][k], P[k], acc) over that range in ascending k, starting from +0.0, in fp32: the
// bits of an element depend on its power row alone, an empty band and an all-zero frame give +0.0 exactly.
//
// mfcc_fbank_generic_kernel is mfcc_spectrum_generic_kernel with the power row kept in the wave's free Stockham buffer
// instead of stored; lane l then owns bands l and l + 64.
//
// mfcc_fbank512_kernel is mfcc_spectrum512_kernel up to barrier B2: the four-wave tile, the power of all 257 bins of
// its 16 frames in the LDS image R (pad 0).  Behind B2 the 256 lanes share the tile's 16 x n_bands elements: the 16
// lanes of a quarter of a wave hold the 16 frames of ONE band (lane & 15 is the frame, as in pass 2), the four quarters
// four consecutive bands, and wave w takes the band groups w, w + 4, ... (fbank_plan.hpp: tile_band).  A lane reads its
// band's range from the LDS copy of the band table, then per bin the weight and the frame's power from LDS, and stores
// one float.  A wave's store covers 16 rows x 16 bytes; the neighbouring 16 bytes of those rows come from the next band
// groups of the same tile, so L2 sees every 128-byte line completed within a tile's time.  WLDS: the packed weights
// fit the 12 KB that two workgroups per CU leave (kWLds floats: any bank of triangles does) and are staged once per
// workgroup.  A matrix with more non-zero spans (a dense 128 x 257 one has 32 896 weights) runs the MFMA form instead
// (WLDS = false): the bf16-split contraction of kernel_fused512_h160_mb.hpp over the same image, with the sets and
// operands fbank_plan.hpp lists (Sets: a set is a block of 16 bands x 32 consecutive bins); wave w contracts blocks w
// and w + 4 and stores four consecutive floats per lane and block.  Both forms were measured at 80 bands (DESIGN.md
// section 4.19): the fp32 form is the faster one where it fits.
//
// LDS banks of the contraction (ds_read_b32: the word address mod 32 inside a 32-lane half): a half holds two bands x
// 16 frames.  The weight reads are two words, broadcast.  The power reads are rows at stride 257 = 1 (mod 32): a
// band's 16 frames fall on 16 consecutive banks, conflict free; the two bands of a half start a few bins apart, so
// their bank runs overlap: 2-way on most reads.  A lane-per-output-element order (64 consecutive bands of one frame in
// a wave) was measured first: its weight reads scatter over the banks and a wave runs to its longest band's range --
// 2.74 ms against this order's figure at 80 bands.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fbank_plan.hpp"
#include "kernel_spectrum.hpp"

namespace mfcc_fbank {

// what both kernels read of a matrix (device pointers into one allocation) and of the scale
struct Tables {
    const float *w;        // packed weights: band j's bins first[j] .. first[j] + count[j] - 1 from word off[j] on
    const int4 *band;      // [n_bands] (first, count, off, 0)
    int n_bands;
    int w_total;           // floats of w
    float c;               // the scale's factor (scale_factor)
    float floor;           // the log's floor
    // the MFMA form of the fused kernel (fbank_plan.hpp: Sets); a_bf NULL: the matrix runs the fp32 form
    const uint4 *a_bf;     // [n_sets][hi, lo][64 lanes]
    uint32_t mask[kMaxBlocks];
    int set_first[kMaxBlocks];
};

// The two launches.  The kernels and these functions are compiled in a translation unit of their own (fbank.hip defines
// MFCC_FBANK_DEFINE_KERNELS), as the decode and resample kernels are: they form a code object of their own, and the code
// object of the MFCC kernels is what it is without them.
// launch_generic: false for an nfft the library does not take.  launch_fused: false when the problem does not fit the
// kernel's 32-bit tile arithmetic (the caller runs the generic kernel)
bool launch_generic(const mfcc_k::StreamDesc &s, const mfcc_spec::GenericTables &t, const Tables &fb, bool log, int nfft,
                    float *out, int n_cu, hipStream_t stream);
bool launch_fused(const mfcc_k::StreamDesc &s, const mfcc_spec::FusedTables &t, const Tables &fb, bool log, float *out,
                  int n_cu, hipStream_t stream);

#ifdef MFCC_FBANK_DEFINE_KERNELS

// E -> the stored value
template <bool LOG>
__device__ __forceinline__ float scaled(float e, float c, float floor) {
    if constexpr (LOG) return c * __builtin_amdgcn_logf(fmaxf(e, floor));       // v_log_f32, as the mel kernels
    return e;
}

// ------------------------------------------------------------------------------ generic

template <int NFFT, bool LOG>
__global__ __launch_bounds__(mfcc_k::kBlock) void mfcc_fbank_generic_kernel(mfcc_k::StreamDesc s, mfcc_spec::GenericTables t,
                                                                          Tables fb, float *__restrict__ out) {
    using namespace mfcc_k;
    constexpr int M = NFFT / 2;
    __shared__ float2 bufA[kWavesPerBlock][M];
    __shared__ float2 bufB[kWavesPerBlock][M + 1];
    // the window and both twiddle tables in LDS up to 512 points, in global memory at 1024 (kernels_generic.hpp says why)
    constexpr bool kStage = NFFT <= 512;
    __shared__ float  winl[kStage ? NFFT : 1];
    __shared__ float2 twl[kStage ? M : 1];
    __shared__ float2 twsl[kStage ? M + 1 : 1];
    if constexpr (kStage) {
        for (int i = threadIdx.x; i < NFFT; i += kBlock) winl[i] = t.window[i];
        for (int i = threadIdx.x; i < M; i += kBlock) twl[i] = t.tw_fft[i];
        for (int i = threadIdx.x; i <= M; i += kBlock) twsl[i] = t.tw_split[i];
    }
    const float *const win_p = kStage ? winl : t.window;
    const float2 *const tw_p = kStage ? twl : t.tw_fft;
    const float2 *const tws_p = kStage ? twsl : t.tw_split;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // the lane's two bands: l and l + 64
    int4 b0 = make_int4(0, 0, 0, 0), b1 = make_int4(0, 0, 0, 0);
    if (lane < fb.n_bands) b0 = fb.band[lane];
    if (lane + 64 < fb.n_bands) b1 = fb.band[lane + 64];

    const long long waves_total = (long long)gridDim.x * kWavesPerBlock;
    const long long step_ch = waves_total / s.frames_per_ch, step_f = waves_total % s.frames_per_ch;
    long long fid = (long long)blockIdx.x * kWavesPerBlock + wave;
    long long ch = fid / s.frames_per_ch, f = fid % s.frames_per_ch;

    for (; fid < s.total_frames; fid += waves_total, ch += step_ch, f += step_f) {
        if (f >= s.frames_per_ch) {
            f -= s.frames_per_ch;
            ++ch;
        }
        const int16_t *base = s.pcm + ch * s.ch_stride;
        gen_stage_frame<NFFT>(s, base, f * (long long)s.hop, win_p, reinterpret_cast<float *>(bufA[wave]), lane);
        wave_sync();
        float2 *src = bufA[wave];
        float2 *dst = bufB[wave];
        gen_stockham<M>(src, dst, tw_p, lane);
        // the power row, as mfcc_spectrum_generic_kernel stores it, into the free buffer (2 M floats >= M + 1)
        float *P = reinterpret_cast<float *>(dst);
        for (int k = lane; k <= M; k += 64) P[k] = gen_split_power<M>(src, tws_p, k) * t.inv_scale2;
        wave_sync();
        float *row = out + fid * fb.n_bands;
        if (lane < fb.n_bands) {
            float acc = 0.0f;
            const float *w = fb.w + b0.z;
            for (int i = 0; i < b0.y; ++i) acc = fmaf(w[i], P[b0.x + i], acc);
            row[lane] = scaled<LOG>(acc, fb.c, fb.floor);
        }
        if (lane + 64 < fb.n_bands) {
            float acc = 0.0f;
            const float *w = fb.w + b1.z;
            for (int i = 0; i < b1.y; ++i) acc = fmaf(w[i], P[b1.x + i], acc);
            row[lane + 64] = scaled<LOG>(acc, fb.c, fb.floor);
        }
        wave_sync();                             // the next frame's staging overwrites what the split and the bands read
    }
}

bool launch_generic(const mfcc_k::StreamDesc &s, const mfcc_spec::GenericTables &t, const Tables &fb, bool log, int nfft,
                           float *out, int n_cu, hipStream_t stream) {
    long long blocks = (s.total_frames + mfcc_k::kWavesPerBlock - 1) / mfcc_k::kWavesPerBlock;
    const long long cap = (long long)n_cu * 128;         // the generic float kernel's grid (mfcc_hip.hip: launch)
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(mfcc_k::kBlock);
    switch (nfft) {
#define MFCC_FBANK_CASE(N)                                                                                            \
    case N:                                                                                                           \
        if (log) hipLaunchKernelGGL((mfcc_fbank_generic_kernel<N, true>), grid, block, 0, stream, s, t, fb, out);     \
        else hipLaunchKernelGGL((mfcc_fbank_generic_kernel<N, false>), grid, block, 0, stream, s, t, fb, out);        \
        break;
        MFCC_FBANK_CASE(64)
        MFCC_FBANK_CASE(128)
        MFCC_FBANK_CASE(256)
        MFCC_FBANK_CASE(512)
        MFCC_FBANK_CASE(1024)
#undef MFCC_FBANK_CASE
        default:
            return false;
    }
    return true;
}

// ------------------------------------------------------------------------------ fused 512

using mfcc_fused::bf16x8;
using mfcc_fused::kNfft;
using mfcc_fused::kSUsed;
using mfcc_fused::kTFrame;
using mfcc_fused::kTRow;
using mfcc_fused::kVStride;
using mfcc_fused::kWaves;
using mfcc_fc::f32x4;
using mfcc_fc::Cursor;
using mfcc_fc::LaunchGeom;
using mfcc_fc::Window;
using mfcc_spec::kFusedBins;

// LDS of the kernel: T | V | S | R | the packed weights | the band table.  Two workgroups per CU: 2 x 80 576 bytes of the
// 160 KB
constexpr int kLdsWords = kTile * kTFrame + kTile * kVStride + kSUsed + kImageWords + kWLds + 2 * kMaxBands;
static_assert(kTileThreads == 64 * kWaves, "fbank_plan.hpp restates the workgroup");
static_assert(kLdsWords * 4 <= 80 * 1024, "two workgroups per CU");

// The MFMA form's contraction of one block of 16 bands over its listed K steps is in the kernel; this is a K step's B
// operand: the eight powers of frame lo at bins 32 s + 8 q + j from the image (zero past bin 256), split into two
// bf16 terms as mfcc_fused::split_power does
__device__ __forceinline__ void step_power(const float *prow, int s, int q, mfcc_fused::u32x4 &ph, mfcc_fused::u32x4 &pl) {
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = set_bin(s, 16 * q, j) < kFusedBins ? prow[kStepBins * s + j] : 0.0f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        uint32_t h, l;
        mfcc_fused::split_bf16_pair(p[2 * d], p[2 * d + 1], h, l);
        ph[d] = h;
        pl[d] = l;
    }
}

// WLDS: the fp32 form with the packed weights staged in LDS; else the MFMA form
template <int HOP, bool LOG, bool WLDS>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfcc_fbank512_kernel(const mfcc_k::StreamDesc s, const mfcc_spec::FusedTables t, const Tables fb, const LaunchGeom g,
                          float *__restrict__ out) {
    using mfcc_codelets::v2f;
    using mfcc_fused::Fetch;
    __shared__ __attribute__((aligned(16))) float lds[kLdsWords];
    constexpr int kTileHopT = kTile * HOP;           // samples between consecutive tiles
    static_assert(7 + (kTile - 1) * HOP + kNfft <= kSUsed, "a tile's frames must lie inside the parked span");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = lane & 15;          // n2 in pass 1, frame in pass 2
    const int q = lane >> 4;           // quarter of the wave
    const int fr_id = wave + 8 * (q & 1) + 4 * (q >> 1);           // the frame this quarter transforms in pass 1

    float *const Tt = lds;                                         // [16 frames][584]
    float *const Vt = Tt + kTile * kTFrame;                        // [16 frames][18]
    float *const Sf = Vt + kTile * kVStride;                       // pre-emphasised sample span, fp32
    float *const Rt = Sf + kSUsed;                                 // [16 frames][257]: the tile's power rows
    float *const Wl = Rt + kImageWords;                            // the packed weights (WLDS)
    int2 *const Bl = reinterpret_cast<int2 *>(Wl + kWLds);         // [n_bands] (first | bins << 16, offset into the weights)

    // per-lane constants, resident for the whole kernel
    v2f wp[16], tw[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) wp[i] = reinterpret_cast<const v2f *>(t.win)[lo * 16 + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) tw[i] = reinterpret_cast<const v2f *>(t.tw)[lo * 16 + i];
    float ax[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ax[i] = t.a_col16[i * 64 + lane];
    const float inv = t.inv_scale2;
    if constexpr (WLDS) {
        for (int i = tid; i < fb.w_total; i += 64 * kWaves) Wl[i] = fb.w[i];      // w_total <= kWLds (launch_fused)
    }
    const int n_bands = fb.n_bands;
    for (int j = tid; j < n_bands; j += 64 * kWaves) {
        const int4 b = fb.band[j];
        Bl[j] = make_int2(pack_range(b.x, b.y), b.z);
    }
    const int steps = tile_steps(n_bands);

    const int lane_slot = fr_id * HOP + lo;
    const int fetcher = (wave - 1) * 64 + lane;
    const bool fetches = wave != 0;
    const int k1 = 4 * wave + q;

    Cursor cur;
    cur.ch = (int)(blockIdx.x / (unsigned)g.tiles_per_ch);
    cur.t_in = (int)(blockIdx.x - (unsigned)cur.ch * (unsigned)g.tiles_per_ch);
    cur.ptr = s.pcm + (long long)cur.ch * s.ch_stride + (long long)cur.t_in * kTileHopT;

    Fetch fx;
    int shift = 0;
    if (cur.ch < g.n_ch) {
        const Window w0 = mfcc_fc::window_of(cur, g);
        shift = w0.shift;
        if (fetches) {
            mfcc_fused::fetch_window<kTileHopT>(s, w0, fetcher, fx);
            mfcc_fused::park_window(Sf, fetcher, fx);
        }
    }
    __syncthreads();

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    while (cur.ch < g.n_ch) {
        // ---------------- pass 1: windowed real FFT-32 over n1 of the pre-emphasised samples
        v2f ep[16];
        {
            const float *sp = Sf + lane_slot + shift;
#pragma unroll
            for (int n1 = 0; n1 < 32; ++n1) ep[n1 >> 1][n1 & 1] = sp[16 * n1];
        }
        const Cursor me = cur;
        mfcc_fc::advance(cur, g);
        const bool more = cur.ch < g.n_ch;
        int next_shift = 0;
        if (more) {
            const Window wn = mfcc_fc::window_of(cur, g);
            next_shift = wn.shift;
            if (fetches) mfcc_fused::fetch_window<kTileHopT>(s, wn, fetcher, fx);
        }
        v2f ty[16];
        float y16;
        mfcc_codelets::rfft32_tw(ep, wp, tw, ty, y16);
        v2f *tcol0 = reinterpret_cast<v2f *>(Tt + fr_id * kTFrame) + lo;
#pragma unroll
        for (int c = 0; c < 16; ++c) tcol0[c * (kTRow / 2)] = ty[c];
        Vt[fr_id * kVStride + lo] = y16;
        mfcc_fc::lds_barrier();                // B1: T and V of all 16 frames are in LDS; S is consumed, and so is R: every
                                               // wave has contracted its part of the previous tile on its way here

        // the tile's span of the output (uniform)
        const long long fr0 = (long long)me.t_in * kTile;
        const long long rows_left = s.frames_per_ch - fr0;
        const int rows = rows_left < kTile ? (int)rows_left : kTile;
        const long long first = ((long long)me.ch * s.frames_per_ch + fr0) * n_bands;

        // ---------------- pass 2: complex FFT-16 over n2 for frame lo, column k1; the power goes to row lo of R
        {
            v2f x[16];
            const f32x4 *trow = reinterpret_cast<const f32x4 *>(Tt + lo * kTFrame + k1 * kTRow);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 a = trow[i];
                x[2 * i] = (v2f){a[0], a[1]};
                x[2 * i + 1] = (v2f){a[2], a[3]};
            }
            v2f pp[8];                               // (|z[k2]|^2, |z[k2 + 8]|^2)
            mfcc_codelets::cfft16_pow(x, pp);
            float *row = Rt + lo * kFusedBins;
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) row[k1 + 32 * k2] = pp[k2].x * inv;
            // k2 = 8 .. 15: bins 32 (16 - k2) - k1; column 0 repeats its own bins there except bin 256 (kernel_spectrum.hpp)
            row[256 - k1] = pp[0].y * inv;
            if (k1 != 0) {
#pragma unroll
                for (int k2 = 9; k2 < 16; ++k2) row[32 * (16 - k2) - k1] = pp[k2 - 8].y * inv;
            }
        }
        if (wave == 1) {
            // column 16 -> bins 16 + 32 j on four fp32 MFMAs (kernel_spectrum.hpp)
            const float v0 = Vt[lo * kVStride + 0 + q], v1 = Vt[lo * kVStride + 4 + q];
            const float v2 = Vt[lo * kVStride + 8 + q], v3 = Vt[lo * kVStride + 12 + q];
            f32x4 sp = zero, sp2 = zero;
            sp = MFCC_MFMA(ax[0], v0, sp);
            sp2 = MFCC_MFMA(ax[1], v1, sp2);
            sp = MFCC_MFMA(ax[2], v2, sp);
            sp2 = MFCC_MFMA(ax[3], v3, sp2);
            sp += sp2;
            float *row = Rt + lo * kFusedBins;
            row[16 + 64 * q] = fmaf(sp[0], sp[0], sp[1] * sp[1]) * inv;
            row[48 + 64 * q] = fmaf(sp[2], sp[2], sp[3] * sp[3]) * inv;
        }
        // park the next tile's sample span (every read of the current one happened before B1)
        if (more && fetches) mfcc_fused::park_window(Sf, fetcher, fx);
        shift = next_shift;
        mfcc_fc::lds_barrier();                // B2: R and S are in LDS, T and V may be overwritten

        // ---------------- contraction and store: lane (frame lo, quarter q) of wave w takes bands 4 (w + 4 i) + q.
        // Nothing waits for the stores: the next barrier orders LDS only
        float *o = out + first;
        if constexpr (WLDS) {
            for (int i = 0; i < steps; ++i) {
                const int j = tile_band(tid, i);
                if (j < n_bands && lo < rows) {
                    const int2 b = Bl[j];
                    const float *w = Wl + b.y;
                    const float *p = Rt + lo * kFusedBins + range_first(b.x);
                    const int n = range_count(b.x);
                    float acc = 0.0f;
#pragma unroll 4
                    for (int k = 0; k < n; ++k) acc = fmaf(w[k], p[k], acc);
                    o[lo * n_bands + j] = scaled<LOG>(acc, fb.c, fb.floor);
                }
            }
        } else {
            // the MFMA form (fbank_plan.hpp: Sets): this wave's blocks are wave and wave + 4; B column = frame lo, K
            // index = quarter q; register r of a block's sum is band 16 block + 4 q + r of frame lo.  Operands are
            // loaded right in front of their three MFMAs, as kernel_fused512_h160_mb.hpp: mel_sets does
            const uint32_t m0 = fb.mask[wave], m1 = fb.mask[wave + kTileWaves];
            const mfcc_fused::u32x4 *a0 = reinterpret_cast<const mfcc_fused::u32x4 *>(fb.a_bf) + (size_t)fb.set_first[wave] * 128 + lane;
            const mfcc_fused::u32x4 *a1 =
                reinterpret_cast<const mfcc_fused::u32x4 *>(fb.a_bf) + (size_t)fb.set_first[wave + kTileWaves] * 128 + lane;
            const float *prow = Rt + lo * kFusedBins + 8 * q;
            f32x4 acc0 = zero, acc1 = zero;
#pragma unroll
            for (int st = 0; st < kSteps; ++st) {
                if (!(((m0 | m1) >> st) & 1)) continue;                   // uniform
                mfcc_fused::u32x4 ph, pl;
                step_power(prow, st, q, ph, pl);
                if ((m0 >> st) & 1) {                                      // uniform
                    const mfcc_fused::u32x4 ah = a0[0], al = a0[64];
                    a0 += 128;
                    acc0 = MFCC_MFMA_BF(ah, ph, acc0);
                    acc0 = MFCC_MFMA_BF(ah, pl, acc0);
                    acc0 = MFCC_MFMA_BF(al, ph, acc0);
                }
                if ((m1 >> st) & 1) {                                      // uniform
                    const mfcc_fused::u32x4 ah = a1[0], al = a1[64];
                    a1 += 128;
                    acc1 = MFCC_MFMA_BF(ah, ph, acc1);
                    acc1 = MFCC_MFMA_BF(ah, pl, acc1);
                    acc1 = MFCC_MFMA_BF(al, ph, acc1);
                }
            }
            if (lo < rows) {
                float *ob = o + lo * n_bands + kBlockBands * wave + 4 * q;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (kBlockBands * wave + 4 * q + r < n_bands) ob[r] = scaled<LOG>(acc0[r], fb.c, fb.floor);
                    if (kBlockBands * (wave + kTileWaves) + 4 * q + r < n_bands)
                        ob[kBlockBands * kTileWaves + r] = scaled<LOG>(acc1[r], fb.c, fb.floor);
                }
            }
        }
    }
}

bool launch_fused(const mfcc_k::StreamDesc &s, const mfcc_spec::FusedTables &t, const Tables &fb, bool log, float *out,
                         int n_cu, hipStream_t stream) {
    LaunchGeom g;
    unsigned grid;
    if (!mfcc_fc::launch_geom(s, n_cu, {kTile, kTile * s.hop, kSUsed}, mfcc_fc::GridRule::kTwoPerCu, 31, g, grid)) return false;
    if (s.hop != 170 && s.hop != 160) return false;
    const bool wlds = fb.a_bf == nullptr;
    if (wlds && !weights_in_lds(size_t(fb.w_total))) return false;          // no operands for the MFMA form: generic
    const dim3 gr(grid), bl(64 * kWaves);
#define MFCC_FBANK_GO(HOP, LOG, WL) hipLaunchKernelGGL((mfcc_fbank512_kernel<HOP, LOG, WL>), gr, bl, 0, stream, s, t, fb, g, out)
#define MFCC_FBANK_HOP(HOP)                     \
    do {                                        \
        if (log && wlds) MFCC_FBANK_GO(HOP, true, true);         \
        else if (log) MFCC_FBANK_GO(HOP, true, false);           \
        else if (wlds) MFCC_FBANK_GO(HOP, false, true);          \
        else MFCC_FBANK_GO(HOP, false, false);                   \
    } while (0)
    if (s.hop == 170) MFCC_FBANK_HOP(170);
    else MFCC_FBANK_HOP(160);
#undef MFCC_FBANK_HOP
#undef MFCC_FBANK_GO
    return true;
}

#endif  // MFCC_FBANK_DEFINE_KERNELS

}  // namespace mfcc_fbank
