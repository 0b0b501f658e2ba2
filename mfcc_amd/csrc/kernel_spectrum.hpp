// The power-spectrum output (include/mfcc_hip.h: "power spectrum"): rows of nfft / 2 + 1 floats
// |FFT(w . y)[k] / power_scale|^2, the intermediate every float kernel computes and drops.
//
//   mfcc_spectrum512_kernel<HOP>    nfft 512 at hop 170 (full frame) and hop 160 (any frame of 160 .. 512 samples)
//   mfcc_spectrum_generic_kernel<N> every other handle: nfft 64 .. 1024, any hop, any frame length
//
// spectrum_plan.hpp decides which one a handle runs and holds the store geometry of the fused tile.
//
// mfcc_spectrum512_kernel is the four-wave tile of kernel_fused512.hpp without its mel, log and DCT phases: a workgroup
// of four waves owns 16 consecutive frames; the tile's sample span is fetched one tile ahead and parked in LDS with the
// exact integer pre-emphasis (fetch_window / park_window); pass 1 is the windowed real FFT-32 over n1 (rfft32_tw) into the
// transpose tile T and the column-16 tile V; barrier B1; pass 2 is the complex FFT-16 over n2 with the power in its last
// layer (cfft16_pow), which leaves lane (frame lo, k1 = 4 wave + q) with the 16 bins k1 + 32 k2 (k2 < 8) and
// 32 (16 - k2) - k1 (k2 >= 8); wave 1 also turns column 16 into the bins 16 + 32 j with the 16 x 16 real DFT matrix on
// four fp32 MFMAs.
//
// What is new is where the power goes.  The fused MFCC kernels contract it out of registers; here all 257 bins of all 16
// frames leave the chip: 16 448 bytes per tile against 5 440 bytes of samples in.  The rows of a tile are ONE contiguous
// span of the dense output, but a row is 1028 bytes, so the span starts anywhere mod 16.  The tile is laid out row-major
// in the LDS image R (row stride 257 words, no padding between rows) behind a pad of (address / 4) mod 4 words, so that a
// float sits at the same offset from a 16-byte boundary in LDS and in HBM; after barrier B2 all 256 lanes stream the image
// out with ds_read_b128 + global_store_dwordx4 on 16-byte-aligned addresses on both sides, and at most three floats in
// front and three behind go one by one (mfcc_spec::store_geom).  The last tile of a channel stores its rows only.
//
// LDS banks (MI355X: ds_write_b32 banks are the word address mod 32, conflicts count inside a 32-lane half; ds_read_b128
// banks are mod 64 inside four groups of 16 lanes):
//   power -> R   lane (lo, q) writes word pad + 257 lo + bin; the two quarters of a half hold neighbouring bins
//                (k1 = 4 wave + q and + 1), so a half's 32 words fall on the banks lo + c and lo + c + 1: 2-way, which a
//                ds_write_b32 absorbs (its four issue cycles cover two LDS-array cycles).  A row stride of 2 (mod 32)
//                would be conflict free but breaks the contiguous image the aligned 16-byte reads need.
//   R -> HBM     lane l reads the aligned 16 bytes at word pad + lead + 4 (v0 + l).  The four lane groups of a
//                ds_read_b128 are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same plus 32: a group's lanes sit in
//                the 16-byte slots (l mod 16) = {0-3, 12-15, 4-11} resp. {4-11, 0-3, 12-15} of a 256-byte bank row, each
//                slot once, so its 16 x 4 words cover all 64 banks exactly once.  Conflict free.
// R is a buffer of its own, not the transpose tile T: T is read by pass 2 of every wave until B2, and a third barrier per
// tile would cost more than the 16 KB of LDS (67 KB per workgroup; two workgroups per CU still fit the 160 KB).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernel_fused512.hpp"
#include "kernels_generic.hpp"
#include "spectrum_plan.hpp"

namespace mfcc_spec {

// ------------------------------------------------------------------------------ generic

struct GenericTables {
    const float  *window;     // [NFFT]       the handle's window: periodic Hamming over the frame, zeros up to NFFT
    const float2 *tw_fft;     // [NFFT/2]     W_M^m, M = NFFT/2
    const float2 *tw_split;   // [NFFT/2 + 1] W_NFFT^k
    float inv_scale2;         // 1 / power_scale^2
};

// One frame per wave, four waves per workgroup: mfcc_float_generic_kernel's frame staging, Stockham FFT and real split
// (kernels_generic.hpp: gen_stage_frame, gen_stockham, gen_split_power), then P[k] / power_scale^2 straight to the row --
// lane l stores bins l, l + 64, ...: 256 contiguous bytes per store instruction.
template <int NFFT>
__global__ __launch_bounds__(mfcc_k::kBlock) void mfcc_spectrum_generic_kernel(mfcc_k::StreamDesc s, GenericTables t,
                                                                             float *__restrict__ out) {
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
        float *row = out + fid * (M + 1);
        for (int k = lane; k <= M; k += 64) row[k] = gen_split_power<M>(src, tws_p, k) * t.inv_scale2;
        wave_sync();                             // the next frame's staging overwrites what the split read
    }
}

inline const char *generic_name() { return name_of(Kernel::kGeneric); }

// false: an nfft the library does not take
#ifndef MFCC_NO_LAUNCHERS          // kernel_fused512.hpp: launch
inline bool launch_generic(const mfcc_k::StreamDesc &s, const GenericTables &t, int nfft, float *out, int n_cu,
                           hipStream_t stream) {
    long long blocks = (s.total_frames + mfcc_k::kWavesPerBlock - 1) / mfcc_k::kWavesPerBlock;
    const long long cap = (long long)n_cu * 128;         // the generic float kernel's grid (mfcc_hip.hip: launch)
    if (blocks > cap) blocks = cap;
    switch (nfft) {
#define MFCC_SPEC_CASE(N)                                                                                              \
    case N:                                                                                                            \
        hipLaunchKernelGGL((mfcc_spectrum_generic_kernel<N>), dim3((unsigned)blocks), dim3(mfcc_k::kBlock), 0, stream, \
                           s, t, out);                                                                                 \
        break;
        MFCC_SPEC_CASE(64)
        MFCC_SPEC_CASE(128)
        MFCC_SPEC_CASE(256)
        MFCC_SPEC_CASE(512)
        MFCC_SPEC_CASE(1024)
#undef MFCC_SPEC_CASE
        default:
            return false;
    }
    return true;
}
#endif

// ------------------------------------------------------------------------------ fused 512

using mfcc_fused::kNfft;
using mfcc_fused::kSUsed;
using mfcc_fused::kTFrame;
using mfcc_fused::kTRow;
using mfcc_fused::kVStride;
using mfcc_fused::kWaves;
using mfcc_fused::kFetchers;
using mfcc_fc::f32x4;
using mfcc_fc::Cursor;
using mfcc_fc::LaunchGeom;
using mfcc_fc::Window;

static_assert(kTile == mfcc_fused::kTile && kFusedNfft == kNfft, "spectrum_plan.hpp restates the fused tile");

// LDS of the kernel: T | V | S | R
constexpr int kLdsWords = kTile * kTFrame + kTile * kVStride + kSUsed + kRWords;

struct FusedTables {
    const float *win;     // [16 n2][32 n1]  window[16 n1 + n2] / 64 (pre-emphasis x32, real-FFT split x2)
    const float2 *tw;     // [16 n2][16 k1]  W512^(n2 k1)
    const float *a_col16; // [4][64 lanes]   the column-16 DFT matrix as MFMA A operands (mfcc_fused::col16_dft_rows)
    float inv_scale2;     // 1 / power_scale^2
};

constexpr size_t kBlobWin = 0, kBlobTw = kBlobWin + 4 * 16 * 32, kBlobCol16 = kBlobTw + 4 * 16 * 16 * 2,
                 kBlobBytes = kBlobCol16 + 4 * 4 * 64;

// host: the tables of a handle whose window is `window` (nfft doubles: zeros from the frame length on)
inline void build_tables(const std::vector<double> &window, std::vector<char> &blob) {
    const std::vector<float> win = mfcc_fused::window_rows<float>(window, 64.0), tw = mfcc_fused::twiddle_rows();
    float col16[4 * 64];
    mfcc_fused::col16_dft_rows(col16);
    blob.assign(kBlobBytes, 0);
    std::memcpy(blob.data() + kBlobWin, win.data(), win.size() * sizeof(float));
    std::memcpy(blob.data() + kBlobTw, tw.data(), tw.size() * sizeof(float));
    std::memcpy(blob.data() + kBlobCol16, col16, sizeof(col16));
}

// device pointer arithmetic only
inline void bind_tables(const char *b, double power_scale, FusedTables &t) {
    t.win = reinterpret_cast<const float *>(b + kBlobWin);
    t.tw = reinterpret_cast<const float2 *>(b + kBlobTw);
    t.a_col16 = reinterpret_cast<const float *>(b + kBlobCol16);
    t.inv_scale2 = float(1.0 / (power_scale * power_scale));
}

// The image R of a finished tile -> the tile's span of the output, by all 256 lanes (header: the store path).  o: the
// span's first float; g: its geometry (uniform)
__device__ __forceinline__ void store_tile(const float *R, float *__restrict__ o, const StoreGeom g, int tid) {
    if (tid < g.lead) o[tid] = R[lds_word(g, tid)];
    const f32x4 *rv = reinterpret_cast<const f32x4 *>(R + lds_vec_word(g, 0));
    f32x4 *ov = reinterpret_cast<f32x4 *>(o + g.lead);
    for (int v = tid; v < g.nvec; v += 64 * kWaves) ov[v] = rv[v];
    const int t0 = g.lead + 4 * g.nvec;
    if (tid < g.tail) o[t0 + tid] = R[lds_word(g, t0 + tid)];
}

template <int HOP>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfcc_spectrum512_kernel(const mfcc_k::StreamDesc s, const FusedTables t, const LaunchGeom g, float *__restrict__ out) {
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
    float *const Rt = Sf + kSUsed;                                 // pad + [16 frames][257]: the tile's rows

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

    const int lane_slot = fr_id * HOP + lo;
    // three waves fetch and park the span, as in the MFCC kernel (its 192 fetchers cover the 3072 slots); wave 0 does
    // not, and has the head and the tail of the store in exchange
    const int fetcher = (wave - 1) * 64 + lane;
    const bool fetches = wave != 0;
    // the lane's 16 bins of frame lo in pass 2, as words of a row: k1 + 32 k2 going up, 32 (16 - k2) - k1 going down
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

    const unsigned long long out_word = reinterpret_cast<uintptr_t>(out) >> 2;
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
                                               // wave has read its part of the previous tile's image on its way here

        // the tile's span of the output (uniform)
        const long long fr0 = (long long)me.t_in * kTile;
        const long long rows_left = s.frames_per_ch - fr0;
        const int rows = rows_left < kTile ? (int)rows_left : kTile;
        const long long first = ((long long)me.ch * s.frames_per_ch + fr0) * kFusedBins;
        const StoreGeom sg = store_geom(out_word + (unsigned long long)first, rows, kFusedBins);

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
            float *row = Rt + sg.pad + lo * kFusedBins;
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) row[k1 + 32 * k2] = pp[k2].x * inv;
            // k2 = 8 .. 15: bins 32 (16 - k2) - k1.  Column 0 is real-input symmetric there: bin 256 (k2 = 8) is its
            // own, the others repeat bins k2' = 16 - k2 and are not stored
            row[256 - k1] = pp[0].y * inv;
            if (k1 != 0) {
#pragma unroll
                for (int k2 = 9; k2 < 16; ++k2) row[32 * (16 - k2) - k1] = pp[k2 - 8].y * inv;
            }
        }
        if (wave == 1) {
            // column 16 -> bins 16 + 32 j: a 16 x 16 real DFT matrix on four fp32 MFMAs; lane (lo, q) ends with
            // (Re, Im) of bins 16 + 64 q and 48 + 64 q of frame lo
            const float v0 = Vt[lo * kVStride + 0 + q], v1 = Vt[lo * kVStride + 4 + q];
            const float v2 = Vt[lo * kVStride + 8 + q], v3 = Vt[lo * kVStride + 12 + q];
            f32x4 sp = zero, sp2 = zero;
            sp = MFCC_MFMA(ax[0], v0, sp);
            sp2 = MFCC_MFMA(ax[1], v1, sp2);
            sp = MFCC_MFMA(ax[2], v2, sp);
            sp2 = MFCC_MFMA(ax[3], v3, sp2);
            sp += sp2;
            float *row = Rt + sg.pad + lo * kFusedBins;
            row[16 + 64 * q] = fmaf(sp[0], sp[0], sp[1] * sp[1]) * inv;
            row[48 + 64 * q] = fmaf(sp[2], sp[2], sp[3] * sp[3]) * inv;
        }
        // park the next tile's sample span (every read of the current one happened before B1)
        if (more && fetches) mfcc_fused::park_window(Sf, fetcher, fx);
        shift = next_shift;
        mfcc_fc::lds_barrier();                // B2: R and S are in LDS, T and V may be overwritten

        // ---------------- store: the image -> HBM.  Nothing waits for the stores: the next barrier orders LDS only
        store_tile(Rt, out + first, sg, tid);
    }
}

inline const char *fused_name() { return name_of(Kernel::kFused512); }

// false: the problem does not fit the kernel's 32-bit tile arithmetic (the caller runs the generic kernel)
#ifndef MFCC_NO_LAUNCHERS
inline bool launch_fused(const mfcc_k::StreamDesc &s, const FusedTables &t, float *out, int n_cu, hipStream_t stream) {
    LaunchGeom g;
    unsigned grid;
    if (!mfcc_fc::launch_geom(s, n_cu, {kTile, kTile * s.hop, kSUsed}, mfcc_fc::GridRule::kTwoPerCu, 31, g, grid)) return false;
    if (s.hop == 170)
        hipLaunchKernelGGL((mfcc_spectrum512_kernel<170>), dim3(grid), dim3(64 * kWaves), 0, stream, s, t, g, out);
    else if (s.hop == 160)
        hipLaunchKernelGGL((mfcc_spectrum512_kernel<160>), dim3(grid), dim3(64 * kWaves), 0, stream, s, t, g, out);
    else
        return false;
    return true;
}
#endif

}  // namespace mfcc_spec
