// What the four fused 1024/341/40 kernels share (kernel_fused1024.hpp, kernel_fused1024_f32.hpp and the two twelve-wave
// forms of kernel_fused1024_w12.hpp): the geometry of a 16-frame tile, the bin map of pass 2, the host code of the tables
// that do not depend on the mel contraction (window rows, twiddles, DCT rows, column 16's DFT rows), the fetch / park of
// a tile's sample window for the eight-wave and for the twelve-wave staging, and the tail's log2 and DCT store.  One
// namespace; the forms `using` it.  What a form keeps is its contraction: the set lists or schedules, the mel operand
// tables, its Tables struct and blob layout, the MFMA window.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "codelets_gen.hpp"
#include "fused_common.hpp"
#include "kernel_fused512.hpp"
#include "kernels_generic.hpp"
#include "tables.hpp"

namespace mfcc_f1k {

constexpr int kNfft = 1024, kHop = 341, kMel = 40, kMaxCep = 40;   // all of them: the reference tops keep nceptrums = nfilters
constexpr int kTile = 16, kWaves = 8;
constexpr int kTileHop = kTile * kHop;            // 5456 samples between consecutive tiles
constexpr int kTRow = 64;                         // words per k1 row of the transpose tile T[frame][k1][n2]: 32 complex
constexpr int kTFrame = 16 * kTRow + 4;           // 1028 words per frame: pass 2 reads a column's 32 values -- contiguous --
                                                  // with 16 ds_read_b128 (256 B/clk; round 2: T[frame][n2][k1], 16 ds_read2_b64 at
                                                  // 128); (row, frame) strides of (16, 257) 16-byte units make every one of
                                                  // them conflict free (brute-forced over the lane groups)
constexpr int kVStride = 34;                      // words per frame in the column-16 tile
constexpr int kBlocks = 3;                        // 16-filter blocks of the 40 filters
constexpr int kQWords = kWaves * kBlocks * 256;   // partial mel sums of the eight-wave forms: [wave][block][lane * 4]
constexpr int kFetchers = 64 * (kWaves - 1);      // eight waves: roles 1..7 fetch and park the sample window
constexpr int kPieces = (7 + (kTile - 1) * kHop + kNfft + 7) / 8;       // 769 pieces of 8 samples are read
constexpr int kSecond = kPieces - kFetchers;      // fetchers that take a second piece (321)
constexpr int kSUsed = 8 * kPieces;               // 6152 fp32 slots

// K slots of the two bf16 MFMAs of a lane: K index 8 q + i  <->  output m = kGrpM[grp][i] of lane group q
constexpr int kGrpM[2][8] = {{0, 1, 2, 3, 12, 13, 14, 15}, {4, 5, 6, 7, 8, 9, 10, 11}};

using mfcc_fc::f32x4;
using mfcc_fc::i32x4;
using mfcc_fc::Cursor;
using mfcc_fc::LaunchGeom;
using mfcc_fc::Window;
using mfcc_fc::advance;
using mfcc_fc::window_of;
using mfcc_fc::preemph8;
using mfcc_fc::lds_barrier;
using mfcc_codelets::v2f;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

inline bool supported(int nfft, int hop, int n_mel, int n_cep) {
    return nfft == kNfft && hop == kHop && n_mel == kMel && n_cep >= 1 && n_cep <= kMaxCep;
}

// bin of output m of the (k1, h) lane; -1: a duplicate that another lane supplies
inline int bin_of(int k1, int h, int m) {
    const int k2 = 2 * m + h;
    if (k2 < 16) return k1 + 32 * k2;
    if (k1 == 0 && k2 > 16) return -1;
    return 32 * (32 - k2) - k1;
}

// ---- host: the tables every form's blob holds (the bf16 round / split of the mel operands is mfcc_fused::bf16_split8)

// [32 n2][32 n1]  hamming[32 n1 + n2] / 64
inline std::vector<float> window_rows() {
    std::vector<float> win(32 * 32);
    const std::vector<double> w = mfcc_tables::hamming_periodic(kNfft);
    for (int n2 = 0; n2 < 32; ++n2)
        for (int n1 = 0; n1 < 32; ++n1) win[n2 * 32 + n1] = float(w[32 * n1 + n2] / 64.0);
    return win;
}

// [32 n2][16 k1] W1024^(n2 k1) as (cos, sin)
inline std::vector<float> twiddle_rows() {
    std::vector<float> tw(32 * 16 * 2);
    for (int n2 = 0; n2 < 32; ++n2)
        for (int k1 = 0; k1 < 16; ++k1) {
            const double a = -2.0 * mfcc_tables::kPi * double(n2 * k1) / 1024.0;
            tw[(n2 * 16 + k1) * 2 + 0] = float(std::cos(a));
            tw[(n2 * 16 + k1) * 2 + 1] = float(std::sin(a));
        }
    return tw;
}

// DCT rows of M tile `tile` (coefficients 16 tile .. 16 tile + 15) as 12 MFMA A operands e[4 blk + r][64 lanes]: lane
// (coeff = l & 15, g = l >> 4) holds D[16 tile + coeff][16 blk + 4 g + r].  dd: mfcc_tables::dct_rows, [n_cep][40]
inline void dct_tile_rows(const std::vector<double> &dd, int n_cep, int tile, float *e) {
    for (int blk = 0; blk < kBlocks; ++blk)
        for (int r = 0; r < 4; ++r)
            for (int l = 0; l < 64; ++l) {
                const int coeff = 16 * tile + (l & 15), filt = 16 * blk + 4 * (l >> 4) + r;
                e[(4 * blk + r) * 64 + l] = (coeff < n_cep && filt < kMel) ? float(dd[size_t(coeff) * kMel + filt]) : 0.0f;
            }
}

// column 16: X[16 + 32 j'] = sum_n2 v[n2] W1024^(n2 (16 + 32 j')), j' = 8 mb + 0..7 (mb = role - 1); MFMA row i = 4 g + r
// holds r = 0: Re j' = 8 mb + 2 g, r = 1: Im (same j'), r = 2: Re j' + 1, r = 3: Im; K step t covers n2 = 4 t + (l >> 4).
// e: the role's operands 0..7, [8][64 lanes]
inline void col16_dft_rows(int mb, float *e) {
    for (int t = 0; t < 8; ++t)
        for (int l = 0; l < 64; ++l) {
            const int i = l & 15, n2 = 4 * t + (l >> 4);
            const int g = i >> 2, r = i & 3, jp = 8 * mb + 2 * g + (r >> 1);
            const double th = 2.0 * mfcc_tables::kPi * double(n2 * (16 + 32 * jp)) / 1024.0;
            e[t * 64 + l] = float((r & 1) ? -std::sin(th) : std::cos(th));
        }
}

// appends a table to a blob
template <class T>
inline void put(std::vector<char> &blob, const std::vector<T> &v) {
    const size_t off = blob.size();
    blob.resize(off + v.size() * sizeof(T));
    std::memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
}

// ---- device

#define MFCC1K_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define MFCC1K_MFMA_BF(a, b, c)                                                                                         \
    __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mfcc_f1k::bf16x8, (a)), __builtin_bit_cast(mfcc_f1k::bf16x8, (b)), \
                                            (c), 0, 0, 0)

struct Fetch {
    i32x4 v0, v1;
    int p0, p1;
};

// fetcher u (0..447) takes pieces u and 448 + u (< 769) of the window, plus the dword in front of each
__device__ __forceinline__ void fetch_window(const mfcc_k::StreamDesc &s, const Window &w, int u, Fetch &f) {
    if (w.inside) {
        const i32x4 *g = reinterpret_cast<const i32x4 *>(w.ptr - w.shift);
        const int *g32 = reinterpret_cast<const int *>(g);
        f.v0 = g[u];
        f.p0 = g32[4 * u - 1];
        f.v1 = (i32x4){0, 0, 0, 0};
        f.p1 = 0;
        if (u < kSecond) {
            f.v1 = g[kFetchers + u];
            f.p1 = g32[4 * (kFetchers + u) - 1];
        }
    } else {
        const long long first = (long long)w.t_in * kTileHop;
        const int16_t *base = w.ptr - first;
        int h[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const long long i = first + (k < 8 ? 0 : 8 * kFetchers) + 8 * u + (k & 7);
            h[k] = mfcc_k::sample_at_i(s, base, i) & 0xFFFF;
        }
        f.v0 = (i32x4){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
        f.v1 = (i32x4){h[8] | (h[9] << 16), h[10] | (h[11] << 16), h[12] | (h[13] << 16), h[14] | (h[15] << 16)};
        f.p0 = mfcc_k::sample_at_i(s, base, first + 8 * u - 1) << 16;
        f.p1 = mfcc_k::sample_at_i(s, base, first + 8 * (kFetchers + u) - 1) << 16;
    }
}

__device__ __forceinline__ void park_window(float *Sf, int u, const Fetch &f) {
    preemph8(f.p0, f.v0, Sf + 8 * u);
    if (u < kSecond) preemph8(f.p1, f.v1, Sf + 8 * (kFetchers + u));
}

// (a, b) -> their bf16 roundings packed in one dword (a low) and the bf16 roundings of what the first rounding lost
__device__ __forceinline__ void split_bf16_pair(float a, float b, uint32_t &hi, uint32_t &lo) {
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(lo) : "v"(ra), "v"(rb));
}

// summed mel energies of a finished tile of the eight-wave forms and their log2; register r of block b is filter
// 16 b + 4 q + r of frame lo.  Filters 40..47 do not exist: their (zero) sums must not reach the DCT as -inf * 0
__device__ __forceinline__ void mel_log2(const float *Qt, int lane, int q, f32x4 (&lm)[kBlocks]) {
    const f32x4 *Q4 = reinterpret_cast<const f32x4 *>(Qt) + lane;
#pragma unroll
    for (int b = 0; b < kBlocks; ++b) {
        f32x4 m = Q4[(0 * kBlocks + b) * 64];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) m += Q4[(w * kBlocks + b) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) lm[b][r] = __builtin_amdgcn_logf(m[r]);
    }
    if (q >= 2) lm[2] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// d[0] + d[1] + d[2] = coefficients 0..15 of a finished tile (their 12 MFMAs are issued by the caller); 16..31 and
// 32..39 are further M tiles whose A operands are fetched here (uniform branches; 12 coalesced dwords per lane out of
// L2).  tab, by value like n_cep, holds groups of [12][64] floats; the rows of M tile `tile` are group GROUP0 + tile:
// GROUP0 = -1 for the bf16 forms' a_dct_hi, 2 for the fp32 forms, which keep them behind the three roles of a_extra
template <int GROUP0>
__device__ __forceinline__ void dct_store(const mfcc_k::StreamDesc &s, int n_cep, const float *tab, const f32x4 (&d)[kBlocks],
                                          const f32x4 (&lm)[kBlocks], const Cursor &c, int lo, int q, int lane,
                                          int lane_off, float *__restrict__ out) {
    const long long fr0 = (long long)c.t_in * kTile;
    const long long rows_left = s.frames_per_ch - fr0;
    float *o = out + ((long long)c.ch * s.frames_per_ch + fr0) * n_cep + lane_off;
    const bool mine = lo < rows_left;
    if (mine) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * q + r < n_cep) o[r] = (d[0][r] + d[1][r]) + d[2][r];
    }
    for (int tile = 1; 16 * tile < n_cep; ++tile) {
        // (-1 + tile and tile - 1 are not the same to the compiler: four instructions of this loop's induction variables
        // depend on the spelling; each form keeps the one it had)
        const float *hi = tab + (GROUP0 == -1 ? (size_t)(tile - 1) : (size_t)(GROUP0 + tile)) * 12 * 64 + lane;
        asm volatile("" : "+v"(hi));                   // not hoisted out of the tile loop: no registers to hold it
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 e[kBlocks] = {zero, zero, zero};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < kBlocks; ++b) e[b] = MFCC1K_MFMA(hi[(4 * b + r) * 64], lm[b][r], e[b]);
        if (mine) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * tile + 4 * q + r < n_cep) o[16 * tile + r] = (e[0][r] + e[1][r]) + e[2][r];
        }
    }
}

// ---- the twelve-wave staging (kernel_fused1024_w12.hpp)

constexpr int kW12Waves = 12;
constexpr int kQSlots = 5;                                   // 4 workers + column 16
constexpr int kQGroupWords = kQSlots * kBlocks * 256;
constexpr int kGroupWords = kTile * kVStride + kQGroupWords + kSUsed;
constexpr int kCRow = 36;                                    // words per n2 row of the constant tables in LDS (9 x 16 B: the 16
                                                             // lanes of a ds_read_b128 group hit 16 different units mod 16)
constexpr int kConstWords = 2 * 32 * kCRow;
constexpr int kW12LdsWords = kTile * kTFrame + 2 * kGroupWords + kConstWords + 4;
static_assert(kW12LdsWords * 4 <= 160 * 1024, "LDS");
constexpr int kParkers = 128, kParkPieces = (kPieces + kParkers - 1) / kParkers;      // 7: the 7th is piece 768 alone

struct FetchN {
    i32x4 v[kParkPieces];
    int p[kParkPieces];          // dword in front of v[k]: its high half is the piece's predecessor sample
};

__device__ __forceinline__ void fetch_window_n(const mfcc_k::StreamDesc &s, const Window &w, int u, FetchN &f) {
    if (w.inside) {
        const i32x4 *g = reinterpret_cast<const i32x4 *>(w.ptr - w.shift);
        const int *g32 = reinterpret_cast<const int *>(g);
#pragma unroll
        for (int k = 0; k < kParkPieces; ++k)
            if (k * kParkers + u < kPieces) {
                f.v[k] = g[k * kParkers + u];
                f.p[k] = g32[4 * (k * kParkers + u) - 1];
            }
    } else {
        const long long first = (long long)w.t_in * kTileHop;      // channel-relative
        const int16_t *base = w.ptr - first;
#pragma unroll
        for (int k = 0; k < kParkPieces; ++k)
            if (k * kParkers + u < kPieces) {
                int h[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = mfcc_k::sample_at_i(s, base, first + 8 * (k * kParkers + u) + j) & 0xFFFF;
                f.v[k] = (i32x4){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
                f.p[k] = mfcc_k::sample_at_i(s, base, first + 8 * (k * kParkers + u) - 1) << 16;
            }
    }
}

__device__ __forceinline__ void park_window_n(float *Sf, int u, const FetchN &f) {
#ifdef MFCC_1K12_EXP_NOPARK
    if (u == 0) Sf[0] = (float)(f.v[0][0] + f.p[0] + f.v[5][1]);
    return;
#endif
#pragma unroll
    for (int k = 0; k < kParkPieces; ++k)
        if (k * kParkers + u < kPieces) preemph8(f.p[k], f.v[k], Sf + 8 * (k * kParkers + u));
}

__device__ __forceinline__ Cursor cursor_of(const mfcc_k::StreamDesc &s, const LaunchGeom &g, unsigned v) {
    Cursor c;
    c.ch = (int)(v / (unsigned)g.tiles_per_ch);
    c.t_in = (int)(v - (unsigned)c.ch * (unsigned)g.tiles_per_ch);
    c.ptr = s.pcm + (long long)c.ch * s.ch_stride + (long long)c.t_in * kTileHop;
    return c;
}

}  // namespace mfcc_f1k
