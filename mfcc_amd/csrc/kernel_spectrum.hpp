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
// four fp32 MFMAs.  That tile, up to the barrier B2 behind which the power lies in the LDS image R, is power_tile_loop
// below, written once for this kernel and for mfcc_fbank512_kernel (kernel_fbank.hpp) out of the helpers of
// kernel_fused512.hpp (first_tile, pass2_power, col16_power); a kernel adds where the image starts and what happens
// to it behind B2.  The generic kernel is the front end of kernels_generic.hpp with the output row as its target.
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

// One frame per wave, four waves per workgroup: the generic front end of kernels_generic.hpp (gen_stage_tables,
// FrameCursor, gen_power_row), with P[k] / power_scale^2 straight to the row -- lane l stores bins l, l + 64, ...: 256
// contiguous bytes per store instruction.
template <int NFFT>
__global__ __launch_bounds__(mfcc_k::kBlock) void mfcc_spectrum_generic_kernel(mfcc_k::StreamDesc s, mfcc_k::PowerTables t,
                                                                             float *__restrict__ out) {
    using namespace mfcc_k;
    constexpr int M = NFFT / 2;
    __shared__ float2 bufA[kWavesPerBlock][M];
    __shared__ float2 bufB[kWavesPerBlock][M + 1];
    const GenTables p = gen_stage_tables<NFFT>(t.window, t.tw_fft, t.tw_split, t.pe_num, t.pe_den);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (FrameCursor c(s, wave); c.fid < s.total_frames; c.next()) {
        c.carry(s);
        gen_power_row<NFFT>(s, c, p, t.inv_scale2, bufA[wave], bufB[wave], lane, [&](float *) { return out + c.fid * (M + 1); });
        wave_sync();                             // the next frame's staging overwrites what the split read
    }
}

inline const char *generic_name() { return name_of(Kernel::kGeneric); }

// false: an nfft the library does not take
#ifndef MFCC_NO_LAUNCHERS          // kernel_fused512.hpp: launch
inline bool launch_generic(const mfcc_k::StreamDesc &s, const mfcc_k::PowerTables &t, int nfft, float *out, int n_cu,
                           hipStream_t stream) {
    const dim3 grid(mfcc_k::generic_grid(s, n_cu));
    switch (nfft) {
#define MFCC_SPEC_CASE(N)                                                                                              \
    case N:                                                                                                            \
        hipLaunchKernelGGL((mfcc_spectrum_generic_kernel<N>), grid, dim3(mfcc_k::kBlock), 0, stream, s, t, out);       \
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
using mfcc_fc::f32x4;
using mfcc_fc::Cursor;
using mfcc_fc::LaunchGeom;
using mfcc_fc::Window;

static_assert(kTile == mfcc_fused::kTile && kFusedNfft == kNfft, "spectrum_plan.hpp restates the fused tile");

// LDS of the kernel: T | V | S | R
constexpr int kTileWords = kTile * kTFrame + kTile * kVStride + kSUsed;       // T | V | S: where the image R starts
constexpr int kLdsWords = kTileWords + kRWords;

struct FusedTables {
    const float *win;     // [16 n2][32 n1]  window[16 n1 + n2] / (2 den) (pre-emphasis x den, real-FFT split x2)
    const float2 *tw;     // [16 n2][16 k1]  W512^(n2 k1)
    const float *a_col16; // [4][64 lanes]   the column-16 DFT matrix as MFMA A operands (mfcc_fused::col16_dft_rows)
    float inv_scale2;     // 1 / power_scale^2
    int preemph;          // the pre-emphasis pair (int16 -num, int16 den), num + den <= 127 (fused_common.hpp: preemph8)
};

constexpr size_t kBlobWin = 0, kBlobTw = kBlobWin + 4 * 16 * 32, kBlobCol16 = kBlobTw + 4 * 16 * 16 * 2,
                 kBlobBytes = kBlobCol16 + 4 * 4 * 64;

// host: the tables of a handle whose window is `window` (nfft doubles: zeros from the frame length on) and whose
// pre-emphasis pair has the denominator den
inline void build_tables(const std::vector<double> &window, std::vector<char> &blob, int den = 32) {
    const std::vector<float> win = mfcc_fused::window_rows<float>(window, 2.0 * double(den)), tw = mfcc_fused::twiddle_rows();
    float col16[4 * 64];
    mfcc_fused::col16_dft_rows(col16);
    blob.assign(kBlobBytes, 0);
    std::memcpy(blob.data() + kBlobWin, win.data(), win.size() * sizeof(float));
    std::memcpy(blob.data() + kBlobTw, tw.data(), tw.size() * sizeof(float));
    std::memcpy(blob.data() + kBlobCol16, col16, sizeof(col16));
}

// device pointer arithmetic only
inline void bind_tables(const char *b, double power_scale, FusedTables &t, int pair = mfcc_tables::packed_preemph(31, 32)) {
    t.preemph = pair;
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

// first row of tile `me` among the output's rows (uniform)
__device__ __forceinline__ long long tile_row0(const mfcc_k::StreamDesc &s, const Cursor &me) {
    return (long long)me.ch * s.frames_per_ch + (long long)me.t_in * kTile;
}

// The power tile of mfcc_spectrum512_kernel and mfcc_fbank512_kernel (kernel_fbank.hpp), written once: the header's
// tile up to barrier B2, behind which the power of the tile's 16 frames x 257 bins lies in the LDS image R.  lds: T | V
// | S | R, and behind them whatever the kernel keeps of its own.  The two kernels give their difference as callables,
// the way mfcc_fused::mel_bf_all takes its After:
//   image_base(me, rows) -> the word of R at which the tile's row 0 starts (uniform; called between B1 and pass 2)
//   tail(me, rows, tid, lo, q, wave, R)  what happens to the image behind B2; nothing waits for its stores, and the
//                                        next tile's B1 is what lets R be rewritten
// me: the tile's cursor; rows: its frames inside the channel (16, fewer in a channel's last tile).  Plain template
// parameters and the arguments by value, as mfcc_fused::tile_loop_w4 takes them.
template <int HOP, typename ImageBase, typename Tail>
__device__ __forceinline__ void power_tile_loop(const mfcc_k::StreamDesc s, const FusedTables t, const LaunchGeom g,
                                                float *lds, ImageBase image_base, Tail tail) {
    using mfcc_codelets::v2f;
    using mfcc_fused::Fetch;
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
    float *const Rt = Sf + kSUsed;                                 // image_base + [16 frames][257]: the tile's rows

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
    // not, and has the head and the tail of the spectrum's store in exchange
    const int fetcher = (wave - 1) * 64 + lane;
    const bool fetches = wave != 0;
    // the lane's 16 bins of frame lo in pass 2, as words of a row: k1 + 32 k2 going up, 32 (16 - k2) - k1 going down
    const int k1 = 4 * wave + q;

    Fetch fx;
    int shift;
    Cursor cur = mfcc_fused::first_tile<kTileHopT>(s, g, Sf, fetcher, fetches, fx, shift, t.preemph);

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
                                               // wave has run its part of the previous tile's tail on its way here

        // the tile's rows (uniform)
        const long long rows_left = s.frames_per_ch - (long long)me.t_in * kTile;
        const int rows = rows_left < kTile ? (int)rows_left : kTile;
        float *const row = Rt + image_base(me, rows) + lo * kFusedBins;

        // ---------------- pass 2: complex FFT-16 over n2 for frame lo, column k1; the power goes to row lo of R
        {
            v2f pp[8];
            mfcc_fused::pass2_power(Tt, lo, k1, pp);
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
            float s0, s1;
            mfcc_fused::col16_power(Vt, ax, lo, q, s0, s1);
            row[16 + 64 * q] = s0 * inv;
            row[48 + 64 * q] = s1 * inv;
        }
        // park the next tile's sample span (every read of the current one happened before B1)
        if (more && fetches) mfcc_fused::park_window(Sf, fetcher, fx, t.preemph);
        shift = next_shift;
        mfcc_fc::lds_barrier();                // B2: R and S are in LDS, T and V may be overwritten

        tail(me, rows, tid, lo, q, wave, Rt);
    }
}

template <int HOP>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfcc_spectrum512_kernel(const mfcc_k::StreamDesc s, const FusedTables t, const LaunchGeom g, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsWords];
    // the tile's span of the output starts at float first(me); its store geometry (uniform)
    const unsigned long long out_word = reinterpret_cast<uintptr_t>(out) >> 2;
    auto first = [&](const Cursor &me) { return tile_row0(s, me) * kFusedBins; };
    auto geom = [&](const Cursor &me, int rows) { return store_geom(out_word + (unsigned long long)first(me), rows, kFusedBins); };
    // the image starts behind the geometry's pad; behind B2 it goes to HBM.  Nothing waits for the stores: the next
    // barrier orders LDS only
    power_tile_loop<HOP>(s, t, g, lds, [&](const Cursor &me, int rows) { return geom(me, rows).pad; },
                         [&](const Cursor &me, int rows, int tid, int, int, int, const float *R) {
                             store_tile(R, out + first(me), geom(me, rows), tid);
                         });
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
