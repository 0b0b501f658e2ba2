// Fused 512-point float kernel at hop 160 with the window taken from the handle's frame length: the ASR framing
// (25 ms window, 10 ms hop, 512-point FFT at 16 kHz = 400 / 160 / 512), DESIGN.md section 4.11.
//
// This is the four-wave form of kernel_fused512.hpp -- a 16-frame tile per workgroup, the tile's sample span parked in
// LDS with the integer pre-emphasis, a windowed real FFT-32 over n1, a complex FFT-16 over n2, the bf16-split mel
// MFMAs straight from registers, the column-16 role, the fp32 DCT tail one tile behind -- with three differences:
//
//  hop     consecutive tiles are 16 * 160 = 2560 samples apart and frame fr of a tile starts at slot 160 fr of the
//          parked span.  A tile reads slots up to 7 + 15 * 160 + 511 = 2918 of the 3072 it parks.
//  window  a frame owns L samples (160 <= L <= 511) and is zero-padded to 512: FusedTables::win holds the periodic
//          Hamming window of length L in its first L entries and zeros behind them (set_window, below).  The kernel
//          still reads 512 slots per frame; slots L .. 511 are finite (pre-emphasised int16, or the zeros the edge path
//          supplies beyond the channel) and meet a zero weight, so whatever follows the frame -- the next frame, the next
//          utterance of a packed batch, the padding -- does not reach its result.
//  log-mel the tail of a log-mel handle stores the n_mel log2 values instead of running the DCT (LOGMEL).
//
// Everything hop independent is the code of kernel_fused512.hpp itself (namespace mfcc_fused: tables, parking, the mel
// contraction, log2, DCT and store); only what names the hop is repeated here.  That file is not touched: its kernels
// compile to the same instructions as before.
//
// LDS banks: a ds_read_b32 takes its bank from the dword address mod 32 and 160 = 0 (mod 32), so the two quarters of a
// 32-lane half (two frames, whatever their distance) read the same 16 banks: the 32 sample reads of pass 1 are 2-way
// conflicts here (at hop 170 the frame distance of 8 puts them 16 banks apart).  DESIGN.md section 4.11 has the account.
#pragma once

#include "kernel_fused512.hpp"

namespace mfcc_fused160 {

using namespace mfcc_fused;          // constants, FusedTables, Fetch and the device helpers shared with the hop-170 form

constexpr int kHop160 = 160;
constexpr int kTileHop160 = kTile * kHop160;   // 2560 samples (5120 bytes: a multiple of 16) between consecutive tiles
constexpr int kMinFrame = kHop160, kMaxFrame = kNfft - 1;
static_assert(7 + (kTile - 1) * kHop160 + kNfft <= kSUsed, "a tile's frames must lie inside the parked span");

// the parameters this kernel covers; frame_len is the handle's frame length (below nfft: a framed handle)
inline bool supported(int nfft, int hop, int frame_len, int n_mel, int n_cep) {
    return nfft == kNfft && hop == kHop160 && frame_len >= kMinFrame && frame_len <= kMaxFrame &&
           (n_mel == kMel || n_mel == 16) && n_cep >= 1 && n_cep <= n_mel;
}

// Puts the window of a frame of L samples into a blob made by mfcc_fused::build_tables<DENSE>: the fp32 rows the kernel
// keeps in registers and the double rows of the DC path, both [16 n2][32 n1] with zeros from sample L on.  The offsets
// follow mfcc_fused::bind_tables.
inline void set_window(std::vector<char> &blob, bool dense, int L) {
    std::vector<double> w = mfcc_tables::hamming_periodic(L);
    w.resize(kNfft, 0.0);
    std::vector<float> win(16 * 32);
    std::vector<double> wd(16 * 32);
    for (int n2 = 0; n2 < 16; ++n2)
        for (int n1 = 0; n1 < 32; ++n1) {
            win[n2 * 32 + n1] = float(w[16 * n1 + n2] / 64.0);
            wd[n2 * 32 + n1] = w[16 * n1 + n2] / 32.0;
        }
    const size_t n_abf = size_t(kWaves) * (dense ? SetsBf<true>::N : SetsBf<false>::N) * 2 * 4 * 64;
    const size_t o_wd = 4 * (size_t(16 * 32) + 16 * 16 * 2 + size_t(kWaves) * (dense ? kAmelDense : kAmelBanded) * 64 +
                             size_t(kWaves) * kAextra * 64 + n_abf);
    std::memcpy(blob.data(), win.data(), win.size() * sizeof(float));
    std::memcpy(blob.data() + o_wd, wd.data(), wd.size() * sizeof(double));
}

// fetch_window of kernel_fused512.hpp with this kernel's tile step in the edge path
__device__ __forceinline__ void fetch_window160(const mfcc_k::StreamDesc &s, const Window &w, int u, Fetch &f) {
    if (w.inside) {
        const i32x4 *g = reinterpret_cast<const i32x4 *>(w.ptr - w.shift);
        const int *g32 = reinterpret_cast<const int *>(g);
        f.v0 = g[u];
        f.p0 = g32[4 * u - 1];
        f.v1 = g[kFetchers + u];
        f.p1 = g32[4 * (kFetchers + u) - 1];
    } else {
        const long long first = (long long)w.t_in * kTileHop160;      // channel-relative
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

// log-mel tail: register r of block b is filter 16 b + 4 q + r of frame lo (mel_log2); lane_off = lo * n_mel + 4 q
__device__ __forceinline__ void logmel_store(const mfcc_k::StreamDesc &s, const FusedTables &t, const f32x4 &l0,
                                             const f32x4 &l1, const Cursor &c, int lo, int lane_off,
                                             float *__restrict__ out) {
    const long long fr0 = (long long)c.t_in * kTile;
    const long long rows_left = s.frames_per_ch - fr0;
    float *o = out + ((long long)c.ch * s.frames_per_ch + fr0) * t.n_mel + lane_off;
    if (lo < rows_left) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = l0[r];
        if (t.n_mel > 16) {                    // filters 16..31 (uniform branch)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[16 + r] = l1[r];
        }
    }
}

template <bool DENSE, bool DCX, bool LOGMEL>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfcc_fused512_h160_kernel(mfcc_k::StreamDesc s, FusedTables t, LaunchGeom g, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsWords + (DCX ? kDcxWords : 0)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int role = wave;             // which extra job the wave has in the MFMA window (kernel_fused512.hpp)
    const int lo = lane & 15;          // n2 in pass 1, k1 in pass 2, frame column in the MFMA phase
    const int q = lane >> 4;           // quarter of the wave; K index g in the MFMA phase
    const int fr_id = wave + 8 * (q & 1) + 4 * (q >> 1);   // frame of the tile this quarter transforms

    float *const Tt = lds;                                         // [16 frames][584]
    float *const Vt = Tt + kTile * kTFrame;                        // [16 frames][18]
    float *const Qt = Vt + kTile * kVStride;                       // [4 waves][2 blocks][256]
    float *const Sf = Qt + kQWords;                                // pre-emphasised sample span, fp32
    double *const Wd = reinterpret_cast<double *>(Sf + kSUsed);    // DCX: double window rows, [16][kWdRow]
    double *const Dc = Wd + 16 * kWdRow;                           // DCX: partial DC sums, [16 frames][kDcRow]
    if constexpr (DCX) {
        for (int i = tid; i < 16 * 32; i += 64 * kWaves) Wd[(i >> 5) * kWdRow + (i & 31)] = t.win_dc[i];
    }

    // per-lane constants, resident for the whole kernel
    using mfcc_codelets::v2f;
    v2f wp[16];                                    // window pairs of this lane's samples: zero from sample L on
#pragma unroll
    for (int i = 0; i < 16; ++i) wp[i] = reinterpret_cast<const v2f *>(t.win)[lo * 16 + i];
    v2f tw[16];                                    // W512^(n2 k1) as (cos, sin)
#pragma unroll
    for (int i = 0; i < 16; ++i) tw[i] = reinterpret_cast<const v2f *>(t.tw)[lo * 16 + i];
    float ax[kAextra];
    constexpr int kSets = SetsBf<DENSE>::N;
    u32x4 ah[kSets], al[kSets];
#pragma unroll
    for (int st = 0; st < kSets; ++st)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            ah[st][d] = t.a_mel_bf[((wave * kSets + st) * 2 + 0) * 256 + d * 64 + lane];
            al[st][d] = t.a_mel_bf[((wave * kSets + st) * 2 + 1) * 256 + d * 64 + lane];
        }
#pragma unroll
    for (int i = 0; i < kAextra; ++i) ax[i] = t.a_extra[(role * kAextra + i) * 64 + lane];

    // slot of this lane's sample n1 = 0 in the span, before the per-tile alignment shift
    const int lane_slot = fr_id * kHop160 + lo;
    const int fetcher = (role - 1) * 64 + lane;     // 0..191 in roles 1..3
    const bool fetches = role != 0;
    const int lane_off = lo * (LOGMEL ? t.n_mel : t.n_cep) + 4 * q;

    Cursor cur;
    cur.ch = (int)(blockIdx.x / (unsigned)g.tiles_per_ch);
    cur.t_in = (int)(blockIdx.x - (unsigned)cur.ch * (unsigned)g.tiles_per_ch);
    cur.ptr = s.pcm + (long long)cur.ch * s.ch_stride + (long long)cur.t_in * kTileHop160;

    // first tile: fetch and park the sample span
    Fetch fx;
    int shift = 0;
    if (cur.ch < g.n_ch) {
        const Window w0 = window_of(cur, g);
        shift = w0.shift;
        if (fetches) {
            fetch_window160(s, w0, fetcher, fx);
            park_window(Sf, fetcher, fx);
        }
    }
    __syncthreads();

    // the role-0 wave finishes tile t (log2, DCT or log-mel store) during tile t + 1
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 lm0 = zero, lm1 = zero;
    Cursor prev = cur;
    bool have_prev = false;

    while (cur.ch < g.n_ch) {
        // ---------------- pass 1: windowed real FFT-32 over n1 of the pre-emphasised samples
        v2f ep[16];                                // (e[2m], e[2m+1]) of this lane's samples i = 16 n1 + n2
        {
            const float *sp = Sf + lane_slot + shift;
#pragma unroll
            for (int n1 = 0; n1 < 32; ++n1) ep[n1 >> 1][n1 & 1] = sp[16 * n1];
        }
        if constexpr (DCX) {
            // bin 0 of this lane's 32 samples in double (the window rows are zero from sample L on)
            const double *wr = Wd + lo * kWdRow;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int m = 0; m < 16; m += 2) {
                a0 = __builtin_fma(wr[2 * m + 0], (double)ep[m][0], a0);
                a1 = __builtin_fma(wr[2 * m + 1], (double)ep[m][1], a1);
                a2 = __builtin_fma(wr[2 * m + 2], (double)ep[m + 1][0], a2);
                a3 = __builtin_fma(wr[2 * m + 3], (double)ep[m + 1][1], a3);
            }
            Dc[fr_id * kDcRow + lo] = (a0 + a1) + (a2 + a3);
        }
        // next tile's samples fly while this tile is processed
        const Cursor me = cur;
        advance(cur, g);
        const bool more = cur.ch < g.n_ch;
        int next_shift = 0;
        if (more) {
            const Window wn = window_of(cur, g);
            next_shift = wn.shift;
            if (fetches) fetch_window160(s, wn, fetcher, fx);
        }
        if (role == 0 && have_prev) mel_log2(Qt, lane, t.n_mel, lm0, lm1);

        v2f ty[16];
        float y16;
        mfcc_codelets::rfft32_tw(ep, wp, tw, ty, y16);

        // transpose through LDS: T[frame][k1][n2]
        v2f *tcol0 = reinterpret_cast<v2f *>(Tt + fr_id * kTFrame) + lo;
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) tcol0[k1 * (kTRow / 2)] = ty[k1];
        Vt[fr_id * kVStride + lo] = y16;
        lds_barrier();                         // B1: T and V of all 16 frames are in LDS; S and Q are consumed

        // ---------------- pass 2: complex FFT-16 over n2 for frame lo, column k1 = 4 wave + q
        float pw[16];                            // |X|^2 at bin(wave, q, k2)
        {
            v2f x[16];
            const f32x4 *trow = reinterpret_cast<const f32x4 *>(Tt + lo * kTFrame + (4 * wave + q) * kTRow);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 a = trow[i];
                x[2 * i] = (v2f){a[0], a[1]};
                x[2 * i + 1] = (v2f){a[2], a[3]};
            }
            v2f pp[8];
            mfcc_codelets::cfft16_pow(x, pp);
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) pw[k2] = pp[k2].x, pw[k2 + 8] = pp[k2].y;
        }
        if constexpr (DCX) {
            if (wave == 0) {                     // lanes (frame lo, k1 = 0) hold bin 0 in pw[0]
                const double *dr = Dc + lo * kDcRow;
                double x0 = 0.0, x1 = 0.0;
#pragma unroll
                for (int n2 = 0; n2 < 16; n2 += 2) {
                    x0 += dr[n2];
                    x1 += dr[n2 + 1];
                }
                x0 += x1;
                if (q == 0) pw[0] = (float)(x0 * x0);
            }
        }

        // ---------------- MFMA window (frame column = lo, K index = q)
        f32x4 x0 = zero, y0 = zero, x1 = zero, y1 = zero;
        PowerBf pb;
        split_power(pw, pb);
        f32x4 acc[kSets];
#pragma unroll
        for (int st = 0; st < kSets; ++st) acc[st] = zero;
        if (role == 0) {
            if constexpr (LOGMEL) {
                mel_bf_all<DENSE, 0>(ah, al, pb, acc, [](auto) {});
                mel_bf_blocks<DENSE>(acc, x0, x1);
                if (have_prev) logmel_store(s, t, lm0, lm1, prev, lo, lane_off, out);
            } else {
                // this tile's mel MFMAs with the previous tile's DCT MFMAs (coefficients 0..15, fp32) in between
                f32x4 d0 = zero, d1 = zero;
                mel_bf_all<DENSE, 0>(ah, al, pb, acc, [&](auto i) {
                    constexpr int I = decltype(i)::value;
                    if constexpr (I < 8) {
                        constexpr int r = I >> 1;
                        if constexpr (I & 1) d1 = MFCC_MFMA(ax[4 + r], lm1[r], d1);
                        else d0 = MFCC_MFMA(ax[r], lm0[r], d0);
                    }
                });
                mel_bf_blocks<DENSE>(acc, x0, x1);
                if (have_prev) dct_store(s, t, lm0, lm1, d0, d1, ax, prev, lo, q, lane_off, out);
            }
        } else if (role == 1) {
            // column 16 -> bins 16 + 32 j of this tile, fed to both filter blocks from registers at the end
            const float v0 = Vt[lo * kVStride + 0 + q], v1 = Vt[lo * kVStride + 4 + q];
            const float v2 = Vt[lo * kVStride + 8 + q], v3 = Vt[lo * kVStride + 12 + q];
            f32x4 sp = zero, sp2 = zero;
            mel_bf_all<DENSE, 0>(ah, al, pb, acc, [&](auto i) {
                constexpr int I = decltype(i)::value;
                if constexpr (I == 0) sp = MFCC_MFMA(ax[0], v0, sp);
                if constexpr (I == 1) sp2 = MFCC_MFMA(ax[1], v1, sp2);
                if constexpr (I == 2) sp = MFCC_MFMA(ax[2], v2, sp);
                if constexpr (I == 3) sp2 = MFCC_MFMA(ax[3], v3, sp2);
            });
            mel_bf_blocks<DENSE>(acc, x0, x1);
            sp += sp2;
            const float s0 = fmaf(sp[0], sp[0], sp[1] * sp[1]);      // bin 16 + 64 q
            const float s1 = fmaf(sp[2], sp[2], sp[3] * sp[3]);      // bin 48 + 64 q
            x0 = MFCC_MFMA(ax[4], s0, x0);
            y0 = MFCC_MFMA(ax[5], s1, y0);
            x1 = MFCC_MFMA(ax[6], s0, x1);
            y1 = MFCC_MFMA(ax[7], s1, y1);
        } else {
            mel_bf_all<DENSE, 0>(ah, al, pb, acc, [](auto) {});
            mel_bf_blocks<DENSE>(acc, x0, x1);
        }
        *reinterpret_cast<f32x4 *>(Qt + (2 * wave + 0) * 256 + lane * 4) = x0 + y0;
        *reinterpret_cast<f32x4 *>(Qt + (2 * wave + 1) * 256 + lane * 4) = x1 + y1;
        prev = me;
        have_prev = true;
        // park the next tile's sample span (every read of the current one happened before B1)
        if (more && fetches) park_window(Sf, fetcher, fx);
        shift = next_shift;
        lds_barrier();                         // B2: partial sums and S are in LDS, T/V may be overwritten
    }
    // the last tile of this workgroup
    if (role == 0 && have_prev) {
        mel_log2(Qt, lane, t.n_mel, lm0, lm1);
        if constexpr (LOGMEL) {
            logmel_store(s, t, lm0, lm1, prev, lo, lane_off, out);
        } else {
            f32x4 d0 = zero, d1 = zero;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                d0 = MFCC_MFMA(ax[r], lm0[r], d0);
                d1 = MFCC_MFMA(ax[4 + r], lm1[r], d1);
            }
            dct_store(s, t, lm0, lm1, d0, d1, ax, prev, lo, q, lane_off, out);
        }
    }
}

inline const char *kernel_name() { return "mfcc_fused512_h160_kernel"; }

// returns false when the problem does not fit the kernel's 32-bit tile arithmetic
template <bool LOGMEL>
inline bool launch(const mfcc_k::StreamDesc &s, const FusedTables &t, bool dense, float *out, int n_cu,
                   hipStream_t stream) {
    const bool dcx = t.win_dc != nullptr;        // only ever set together with the dense schedule
    LaunchGeom g;
    unsigned grid;
    if (!mfcc_fc::launch_geom(s, n_cu, {kTile, kTileHop160, kSUsed}, mfcc_fc::GridRule::kTwoPerCu, 31, g, grid)) return false;
    if (dense && dcx)
        hipLaunchKernelGGL((mfcc_fused512_h160_kernel<true, true, LOGMEL>), dim3(grid), dim3(64 * kWaves), 0, stream, s, t, g, out);
    else if (dense)
        hipLaunchKernelGGL((mfcc_fused512_h160_kernel<true, false, LOGMEL>), dim3(grid), dim3(64 * kWaves), 0, stream, s, t, g, out);
    else
        hipLaunchKernelGGL((mfcc_fused512_h160_kernel<false, false, LOGMEL>), dim3(grid), dim3(64 * kWaves), 0, stream, s, t, g, out);
    return true;
}

}  // namespace mfcc_fused160
