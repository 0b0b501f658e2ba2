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
// mfcc_fbank_generic_kernel is mfcc_spectrum_generic_kernel's frame loop (kernels_generic.hpp: gen_power_row) with the
// power row kept in the wave's free Stockham buffer instead of stored; lane l then owns bands l and l + 64.
//
// mfcc_fbank512_kernel is mfcc_spectrum512_kernel up to barrier B2, the same code (kernel_spectrum.hpp:
// power_tile_loop): the four-wave tile, the power of all 257 bins of its 16 frames in the LDS image R (pad 0).  The
// kernel itself is the staging of the weights and the band table, and the tail behind B2.  There the 256 lanes share the tile's 16 x n_bands elements: the 16
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
bool launch_generic(const mfcc_k::StreamDesc &s, const mfcc_k::PowerTables &t, const Tables &fb, bool log, int nfft,
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
__global__ __launch_bounds__(mfcc_k::kBlock) void mfcc_fbank_generic_kernel(mfcc_k::StreamDesc s, mfcc_k::PowerTables t,
                                                                          Tables fb, float *__restrict__ out) {
    using namespace mfcc_k;
    constexpr int M = NFFT / 2;
    __shared__ float2 bufA[kWavesPerBlock][M];
    __shared__ float2 bufB[kWavesPerBlock][M + 1];
    const GenTables p = gen_stage_tables<NFFT>(t.window, t.tw_fft, t.tw_split, t.pe_num, t.pe_den);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // the lane's two bands: l and l + 64
    int4 b0 = make_int4(0, 0, 0, 0), b1 = make_int4(0, 0, 0, 0);
    if (lane < fb.n_bands) b0 = fb.band[lane];
    if (lane + 64 < fb.n_bands) b1 = fb.band[lane + 64];

    for (FrameCursor c(s, wave); c.fid < s.total_frames; c.next()) {
        c.carry(s);
        // the power row, as mfcc_spectrum_generic_kernel stores it, kept in the free Stockham buffer
        const float *P = gen_power_row<NFFT>(s, c, p, t.inv_scale2, bufA[wave], bufB[wave], lane, [](float *buf) { return buf; });
        wave_sync();
        float *row = out + c.fid * fb.n_bands;
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

bool launch_generic(const mfcc_k::StreamDesc &s, const mfcc_k::PowerTables &t, const Tables &fb, bool log, int nfft,
                           float *out, int n_cu, hipStream_t stream) {
    const dim3 grid(mfcc_k::generic_grid(s, n_cu)), block(mfcc_k::kBlock);
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
using mfcc_fused::kSUsed;
using mfcc_fused::kWaves;
using mfcc_fc::f32x4;
using mfcc_fc::Cursor;
using mfcc_fc::LaunchGeom;
using mfcc_spec::kFusedBins;

// LDS of the kernel: T | V | S | R | the packed weights | the band table.  Two workgroups per CU: 2 x 80 576 bytes of the
// 160 KB
constexpr int kLdsWords = mfcc_spec::kTileWords + kImageWords + kWLds + 2 * kMaxBands;
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
    __shared__ __attribute__((aligned(16))) float lds[kLdsWords];
    float *const Wl = lds + mfcc_spec::kTileWords + kImageWords;   // the packed weights (WLDS), behind the power tile's T | V | S | R
    int2 *const Bl = reinterpret_cast<int2 *>(Wl + kWLds);         // [n_bands] (first | bins << 16, offset into the weights)
    // staged once per workgroup; the power tile's first barrier publishes them
    if constexpr (WLDS) {
        for (int i = threadIdx.x; i < fb.w_total; i += 64 * kWaves) Wl[i] = fb.w[i];      // w_total <= kWLds (launch_fused)
    }
    const int n_bands = fb.n_bands;
    for (int j = threadIdx.x; j < n_bands; j += 64 * kWaves) {
        const int4 b = fb.band[j];
        Bl[j] = make_int2(pack_range(b.x, b.y), b.z);
    }
    const int steps = tile_steps(n_bands);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // the image is [16 frames][257] from word 0 of R on
    mfcc_spec::power_tile_loop<HOP>(s, t, g, lds, [](const Cursor &, int) { return 0; },
                                    [&](const Cursor &me, int rows, int tid, int lo, int q, int wave, const float *Rt) {
        const int lane = tid & 63;
        // ---------------- contraction and store: lane (frame lo, quarter q) of wave w takes bands 4 (w + 4 i) + q.
        // Nothing waits for the stores: the next barrier orders LDS only
        float *o = out + mfcc_spec::tile_row0(s, me) * n_bands;
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
    });
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
