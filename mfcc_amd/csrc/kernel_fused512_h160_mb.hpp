// Fused 512-point float kernel at hop 160 for a mel bank given as a matrix: one to four blocks of 16 filters
// (1 <= n_mel <= 64), the HTK-style banks of mfcc_hip_create_banked.  DESIGN.md section 4.12.
//
// This is the tile loop of kernel_fused512.hpp (tile_loop_w4) at hop 160 -- the 16-frame tile, the sample span parked in LDS with the integer
// pre-emphasis, the windowed real FFT-32 and the complex FFT-16, split_power, the two barriers, the tail one tile behind
// -- without the DC path and with the mel contraction driven by the handle's matrix instead of a compile-time list.
// fetch_window<TILE_HOP>, parking, split_power and the host table helpers are mfcc_fused's; the loop itself is repeated
// here (DESIGN.md section 4.1 says why), so a change to the passes, the barriers or the parking belongs in both.
// It restates all three of kernel_fused512.hpp's tile helpers -- first_tile (the cursor's start up to __syncthreads()),
// pass2_power (the T column and cfft16_pow) and col16_power (role 1's four fp32 MFMAs, issued here in front of mel_sets
// and summed behind it) -- because on each of them this kernel compiles to other instructions than on its own lines:
// 2 to 4 instructions more with first_tile, commuted v_pk_add_f32 operands with pass2_power, 310 reordered lines with
// t_column alone, 3 instructions fewer and another LDS read pattern with col16_power.
//
//  sets     the host walks the matrix with the bin <-> (wave, quarter, k2) map of mfcc_fused::build_tables and lists the
//           (filter block, K group) pairs that carry a non-zero weight (build_tables below; 4 to 6 of the 8 possible for
//           the banks of the speech front ends).  It builds the hi / lo bf16 operands for exactly those, in list order.
//           The kernel takes the list as a bit mask, one bit per pair: a wave-uniform branch per pair, every register
//           index a compile-time constant.
//  operands a set's two 16-byte operands are not resident: each lane loads them from the table (2 KB per wave and set,
//           48 KB at six sets: in L2 after the first tile of a CU) right before the set's three MFMAs.  The registers the resident form would
//           need are the accumulators of the four blocks here.
//  blocks   the partial sums meet in Q[wave][block][256]; role 0 takes log2 of up to four blocks; the DCT runs over up to
//           64 K slots (coefficients 0..15: n_cep <= 16); role 1 feeds column 16 to every block present (two fp32 MFMAs
//           per block).
//  padding  filter rows at or beyond n_mel have zero weights, a zero sum and a log of -inf: their log-mel value is set
//           to zero before the DCT (their DCT weight is zero too: no -inf * 0) and is not stored by the log-mel tail.
//  bin 0    a bank with weight on the DC bin is refused by build_tables (an HTK bank with low >= 0 has none): there is
//           no double-precision DC path here.
#pragma once

#include "kernel_fused512_h160.hpp"

namespace mfcc_fused160mb {

using namespace mfcc_fused160;       // and, through it, mfcc_fused

constexpr int kMaxBlocks = 4;                              // filter blocks of 16: n_mel <= 64
constexpr int kMaxPairs = 2 * kMaxBlocks;                  // (block, K group) pairs; pair index = 2 block + group
constexpr int kMaxCepMb = 16;                              // one M tile of DCT coefficients
constexpr int kQWordsMb = kWaves * kMaxBlocks * 256;       // partial mel sums: [wave][block][lane * 4]
static_assert(lds_words(kQWordsMb, false) * 4 <= 80 * 1024, "two workgroups per CU");

// the parameters this kernel covers (the bank itself is checked by build_tables)
inline bool supported(int nfft, int hop, int frame_len, int n_mel, int n_cep, bool logmel) {
    return nfft == kNfft && hop == kHop160 && frame_len >= kMinFrame && frame_len <= kMaxFrame && n_mel >= 1 &&
           n_mel <= 16 * kMaxBlocks && n_cep >= 1 && n_cep <= n_mel && (logmel || n_cep <= kMaxCepMb);
}

struct Tables {
    const float *win;          // [16 n2][32 n1]  window of the frame length / (2 den), zeros from sample L on
    const float2 *tw;          // [16 n2][16 k1]  W512^(n2 k1)
    const u32x4 *a_bf;         // [4 waves][n_sets][hi, lo][64 lanes] bf16 pairs of the listed sets, in pair order
    const float *a_extra;      // [4 roles][16][64]  role 0: DCT rows, index 4 block + r; role 1: column-16 DFT (0..3)
                               // and its mel weights, index 4 + 2 block + step
    uint32_t set_mask;         // bit 2 block + group: the pair is in the list
    int n_sets;                // popcount(set_mask)
    int n_blocks;              // (n_mel + 15) / 16
    int n_cep;
    int n_mel;
    int preemph;               // the pre-emphasis pair (int16 -num, int16 den), num + den <= 127 (fused_common.hpp: preemph8)
};

// ---- host.  md: the handle's matrix [n_mel][257] (float64 holding the weights as the contract rounds them), before the
// power scale.  Returns false when a filter has weight on bin 0 or (never, by construction) a weight is not covered.
// blob layout: win | tw | a_extra | a_bf; sets: the listed pairs in order (for the record in DESIGN.md and the tests).
// w: the handle's window over kNfft samples (zeros from the frame length on); den: of the pre-emphasis pair, folded into
// the window rows (the pair itself goes through bind_tables).
inline bool build_tables(const std::vector<double> &md, int n_mel, int n_cep, const std::vector<double> &w, int den,
                         double power_scale, double lifter, std::vector<char> &blob, uint32_t &set_mask) {
    using namespace mfcc_tables;
    const int nb = (n_mel + 15) / 16;
    if (n_mel < 1 || nb > kMaxBlocks || md.size() != size_t(n_mel) * 257) return false;
    if (w.size() != size_t(kNfft) || den < 1 || den > kMaxFusedPreemphSum) return false;
    for (int f = 0; f < n_mel; ++f)
        if (md[size_t(f) * 257] != 0.0) return false;                 // bin 0 is real-valued: no DC path here
    const double inv = 1.0 / (power_scale * power_scale);
    auto W = [&](int filt, int bin) -> float { return filt < n_mel ? float(md[size_t(filt) * 257 + bin] * inv) : 0.0f; };
    auto bin_of = [](int k1, int k2) { return k2 < 8 ? k1 + 32 * k2 : 32 * (16 - k2) - k1; };

    const std::vector<float> win = window_rows<float>(w, 2.0 * double(den)), tw = twiddle_rows();
    std::vector<float> aext(size_t(kWaves) * kAextra * 64, 0.0f);
    // the set list: pair (block, group) is needed when any wave has a non-zero weight in it
    set_mask = 0;
    for (int blk = 0; blk < nb; ++blk)
        for (int grp = 0; grp < 2; ++grp)
            for (int m = 0; m < 16; ++m)
                for (int k1 = 0; k1 < 16; ++k1)
                    for (int j = 0; j < 8; ++j) {
                        const int k2 = kGrpK2[grp][j];
                        if (k1 == 0 && k2 > 8) continue;               // bins 32 (16 - k2): supplied by k2' = 16 - k2
                        if (W(16 * blk + m, bin_of(k1, k2)) != 0.0f) set_mask |= 1u << (2 * blk + grp);
                    }
    int n_sets = 0;
    for (int p = 0; p < kMaxPairs; ++p) n_sets += (set_mask >> p) & 1;
    auto E = [&](int role, int idx, int lane) -> float & { return aext[(size_t(role) * kAextra + idx) * 64 + lane]; };
    // role 0 -- DCT rows: lane (coeff = l & 15, g = l >> 4) holds D[coeff][16 blk + 4 g + r] at index 4 blk + r
    std::vector<double> dd = dct_rows(n_cep, n_mel, lifter);                   // [n_cep][n_mel]
    for (int blk = 0; blk < nb; ++blk)
        for (int r = 0; r < 4; ++r)
            for (int l = 0; l < 64; ++l) {
                const int coeff = l & 15, filt = 16 * blk + 4 * (l >> 4) + r;
                E(0, 4 * blk + r, l) = (coeff < n_cep && filt < n_mel) ? float(dd[size_t(coeff) * n_mel + filt]) : 0.0f;
            }
    // role 1 -- column 16 ...
    col16_dft_rows(&E(1, 0, 0));
    std::vector<char> covered(size_t(16 * kMaxBlocks) * 257, 0);
    // ... and those bins as a K step: lane g supplies bin 16 + 64 g (step 0) / 48 + 64 g (step 1)
    for (int blk = 0; blk < nb; ++blk)
        for (int step = 0; step < 2; ++step)
            for (int l = 0; l < 64; ++l) {
                const int filt = blk * 16 + (l & 15), bin = 16 + 64 * (l >> 4) + 32 * step;
                E(1, 4 + 2 * blk + step, l) = W(filt, bin);
                covered[size_t(filt) * 257 + bin] = 1;
            }
    // bf16 split of the listed sets: lane l of wave wv holds row m = l & 15 of the set's filter block at K slots
    // j = 0..7 <-> bin(wv, l >> 4, kGrpK2[grp][j]); dword d = slots (2 d, 2 d + 1); one u32x4 per lane and term
    std::vector<uint32_t> abf(size_t(kWaves) * (n_sets ? n_sets : 1) * 2 * 64 * 4, 0u);
    for (int wv = 0; wv < kWaves; ++wv) {
        int st = 0;
        for (int p = 0; p < kMaxPairs; ++p) {
            if (!((set_mask >> p) & 1)) continue;
            const int blk = p >> 1, grp = p & 1;
            for (int l = 0; l < 64; ++l) {
                float wgt[8];
                for (int j = 0; j < 8; ++j) {
                    const int k2 = kGrpK2[grp][j], filt = blk * 16 + (l & 15), k1 = 4 * wv + (l >> 4);
                    wgt[j] = 0.0f;
                    if (!(k1 == 0 && k2 > 8)) {
                        wgt[j] = W(filt, bin_of(k1, k2));
                        covered[size_t(filt) * 257 + bin_of(k1, k2)] = 1;
                    }
                }
                uint32_t vh[4], vl[4];
                bf16_split8(wgt, vh, vl);
                std::memcpy(&abf[(((size_t(wv) * n_sets + st) * 2 + 0) * 64 + l) * 4], vh, sizeof vh);
                std::memcpy(&abf[(((size_t(wv) * n_sets + st) * 2 + 1) * 64 + l) * 4], vl, sizeof vl);
            }
            ++st;
        }
    }
    // every non-zero weight must be reached by a listed set or by column 16
    for (int f = 0; f < n_mel; ++f)
        for (int k = 0; k < 257; ++k)
            if (W(f, k) != 0.0f && !covered[size_t(f) * 257 + k]) return false;
    blob.clear();
    auto put = [&](const void *p, size_t bytes) {
        const size_t off = blob.size();
        blob.resize(off + bytes);
        std::memcpy(blob.data() + off, p, bytes);
    };
    put(win.data(), win.size() * 4);
    put(tw.data(), tw.size() * 4);
    put(aext.data(), aext.size() * 4);
    put(abf.data(), abf.size() * 4);          // 16-byte aligned: everything before is a multiple of 16 bytes
    return true;
}

// the reference's front: the periodic Hamming window over frame_len samples and 31/32
inline bool build_tables(const std::vector<double> &md, int n_mel, int n_cep, int frame_len, double power_scale,
                         double lifter, std::vector<char> &blob, uint32_t &set_mask) {
    std::vector<double> w = mfcc_tables::hamming_periodic(frame_len);
    w.resize(kNfft, 0.0);
    return build_tables(md, n_mel, n_cep, w, 32, power_scale, lifter, blob, set_mask);
}

// device pointer arithmetic only; b must be 16-byte aligned.  pair: mfcc_tables::packed_preemph of the handle's pair
inline void bind_tables(const char *b, int n_cep, int n_mel, uint32_t set_mask, Tables &t,
                        int pair = mfcc_tables::packed_preemph(31, 32)) {
    const float *f = reinterpret_cast<const float *>(b);
    t.win = f;                                  f += 16 * 32;
    t.tw = reinterpret_cast<const float2 *>(f); f += 16 * 16 * 2;
    t.a_extra = f;                              f += kWaves * kAextra * 64;
    t.a_bf = reinterpret_cast<const u32x4 *>(f);
    t.set_mask = set_mask;
    t.n_sets = 0;
    for (int p = 0; p < kMaxPairs; ++p) t.n_sets += (set_mask >> p) & 1;
    t.n_blocks = (n_mel + 15) / 16;
    t.n_cep = n_cep;
    t.n_mel = n_mel;
    t.preemph = pair;
}

// ---- device

// The summed mel energies of a finished tile, then log2: register r of block b is filter 16 b + 4 q + r of frame lo.
// Rows at or beyond n_mel (padding) become 0; blocks at or beyond n_blocks are not read and stay 0.
__device__ __forceinline__ void mel_log2_mb(const float *Qt, int lane, int q, int n_blocks, int n_mel,
                                            f32x4 (&lm)[kMaxBlocks]) {
    const f32x4 *Q4 = reinterpret_cast<const f32x4 *>(Qt) + lane;
#pragma unroll
    for (int b = 0; b < kMaxBlocks; ++b) {
        lm[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (b < n_blocks) {                                              // uniform
            const f32x4 m = (Q4[(0 * kMaxBlocks + b) * 64] + Q4[(1 * kMaxBlocks + b) * 64]) +
                            (Q4[(2 * kMaxBlocks + b) * 64] + Q4[(3 * kMaxBlocks + b) * 64]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float l = __builtin_amdgcn_logf(m[r]);             // v_log_f32, as mfcc_fused::mel_log2
                lm[b][r] = (16 * b + 4 * q + r < n_mel) ? l : 0.f;
            }
        }
    }
}

// DCT-II over the blocks present (coefficients 0..15) and store; lane_off = lo * n_cep + 4 q
__device__ __forceinline__ void dct_store_mb(const mfcc_k::StreamDesc &s, const Tables &t, const f32x4 (&lm)[kMaxBlocks],
                                             const float (&ax)[kAextra], const Cursor &c, int lo, int q, int lane_off,
                                             float *__restrict__ out) {
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
#pragma unroll
    for (int b = 0; b < kMaxBlocks; ++b)
        if (b < t.n_blocks) {                                            // uniform
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r & 1) d1 = MFCC_MFMA(ax[4 * b + r], lm[b][r], d1);
                else d0 = MFCC_MFMA(ax[4 * b + r], lm[b][r], d0);
            }
        }
    const long long fr0 = (long long)c.t_in * kTile;
    const long long rows_left = s.frames_per_ch - fr0;
    float *o = out + ((long long)c.ch * s.frames_per_ch + fr0) * t.n_cep + lane_off;
    if (lo < rows_left) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * q + r < t.n_cep) o[r] = d0[r] + d1[r];
    }
}

// log-mel tail: lane_off = lo * n_mel + 4 q; padding rows are not stored
__device__ __forceinline__ void logmel_store_mb(const mfcc_k::StreamDesc &s, const Tables &t, const f32x4 (&lm)[kMaxBlocks],
                                                const Cursor &c, int lo, int q, int lane_off, float *__restrict__ out) {
    const long long fr0 = (long long)c.t_in * kTile;
    const long long rows_left = s.frames_per_ch - fr0;
    float *o = out + ((long long)c.ch * s.frames_per_ch + fr0) * t.n_mel + lane_off;
    if (lo < rows_left) {
#pragma unroll
        for (int b = 0; b < kMaxBlocks; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * b + 4 * q + r < t.n_mel) o[16 * b + r] = lm[b][r];
    }
}

// the listed sets of this wave: operands from the table, three MFMAs each (Wh Ph, Wh Pl, Wl Ph) into the block's sum
__device__ __forceinline__ void mel_sets(const Tables &t, int wave, int lane, const PowerBf &pb, f32x4 (&acc)[kMaxBlocks]) {
    const u32x4 *a = t.a_bf + (size_t)wave * t.n_sets * 128 + lane;
#pragma unroll
    for (int p = 0; p < kMaxPairs; ++p) {
        if (t.set_mask & (1u << p)) {                                    // uniform
            const u32x4 ah = a[0], al = a[64];
            a += 128;
            const int b = p >> 1, g = p & 1;
            acc[b] = MFCC_MFMA_BF(ah, pb.hi[g], acc[b]);
            acc[b] = MFCC_MFMA_BF(ah, pb.lo[g], acc[b]);
            acc[b] = MFCC_MFMA_BF(al, pb.hi[g], acc[b]);
        }
    }
}

template <bool LOGMEL>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfcc_fused512_h160_mb_kernel(mfcc_k::StreamDesc s, Tables t, LaunchGeom g, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[lds_words(kQWordsMb, false)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int role = wave;             // which extra job the wave has in the MFMA window (kernel_fused512.hpp)
    const int lo = lane & 15;          // n2 in pass 1, k1 in pass 2, frame column in the MFMA phase
    const int q = lane >> 4;           // quarter of the wave; K index g in the MFMA phase
    const int fr_id = wave + 8 * (q & 1) + 4 * (q >> 1);   // frame of the tile this quarter transforms

    float *const Tt = lds;                                         // [16 frames][584]
    float *const Vt = Tt + kTile * kTFrame;                        // [16 frames][18]
    float *const Qt = Vt + kTile * kVStride;                       // [4 waves][4 blocks][256]
    float *const Sf = Qt + kQWordsMb;                              // pre-emphasised sample span, fp32

    // per-lane constants, resident for the whole kernel
    using mfcc_codelets::v2f;
    v2f wp[16];                                    // window pairs of this lane's samples: zero from sample L on
#pragma unroll
    for (int i = 0; i < 16; ++i) wp[i] = reinterpret_cast<const v2f *>(t.win)[lo * 16 + i];
    v2f tw[16];                                    // W512^(n2 k1) as (cos, sin)
#pragma unroll
    for (int i = 0; i < 16; ++i) tw[i] = reinterpret_cast<const v2f *>(t.tw)[lo * 16 + i];
    float ax[kAextra];
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
            fetch_window<kTileHop160>(s, w0, fetcher, fx);
            park_window(Sf, fetcher, fx, t.preemph);
        }
    }
    __syncthreads();

    // the role-0 wave finishes tile t (log2, DCT or log-mel store) during tile t + 1
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 lm[kMaxBlocks] = {zero, zero, zero, zero};
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
        // next tile's samples fly while this tile is processed
        const Cursor me = cur;
        advance(cur, g);
        const bool more = cur.ch < g.n_ch;
        int next_shift = 0;
        if (more) {
            const Window wn = window_of(cur, g);
            next_shift = wn.shift;
            if (fetches) fetch_window<kTileHop160>(s, wn, fetcher, fx);
        }
        if (role == 0 && have_prev) mel_log2_mb(Qt, lane, q, t.n_blocks, t.n_mel, lm);

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

        // ---------------- MFMA window (frame column = lo, K index = q)
        PowerBf pb;
        split_power(pw, pb);
        f32x4 acc[kMaxBlocks] = {zero, zero, zero, zero};
        if (role == 1) {
            // column 16 -> bins 16 + 32 j of this tile, fed to every filter block present
            const float v0 = Vt[lo * kVStride + 0 + q], v1 = Vt[lo * kVStride + 4 + q];
            const float v2 = Vt[lo * kVStride + 8 + q], v3 = Vt[lo * kVStride + 12 + q];
            f32x4 sp = zero, sp2 = zero;
            sp = MFCC_MFMA(ax[0], v0, sp);
            sp2 = MFCC_MFMA(ax[1], v1, sp2);
            sp = MFCC_MFMA(ax[2], v2, sp);
            sp2 = MFCC_MFMA(ax[3], v3, sp2);
            mel_sets(t, wave, lane, pb, acc);
            sp += sp2;
            const float s0 = fmaf(sp[0], sp[0], sp[1] * sp[1]);      // bin 16 + 64 q
            const float s1 = fmaf(sp[2], sp[2], sp[3] * sp[3]);      // bin 48 + 64 q
#pragma unroll
            for (int b = 0; b < kMaxBlocks; ++b)
                if (b < t.n_blocks) {                                  // uniform
                    f32x4 c = MFCC_MFMA(ax[4 + 2 * b], s0, zero);
                    c = MFCC_MFMA(ax[5 + 2 * b], s1, c);
                    acc[b] += c;
                }
        } else {
            mel_sets(t, wave, lane, pb, acc);
            if (role == 0 && have_prev) {
                if constexpr (LOGMEL) logmel_store_mb(s, t, lm, prev, lo, q, lane_off, out);
                else dct_store_mb(s, t, lm, ax, prev, lo, q, lane_off, out);
            }
        }
#pragma unroll
        for (int b = 0; b < kMaxBlocks; ++b)
            if (b < t.n_blocks)                                        // uniform
                *reinterpret_cast<f32x4 *>(Qt + (kMaxBlocks * wave + b) * 256 + lane * 4) = acc[b];
        prev = me;
        have_prev = true;
        // park the next tile's sample span (every read of the current one happened before B1)
        if (more && fetches) park_window(Sf, fetcher, fx, t.preemph);
        shift = next_shift;
        lds_barrier();                         // B2: partial sums and S are in LDS, T/V may be overwritten
    }
    // the last tile of this workgroup
    if (role == 0 && have_prev) {
        mel_log2_mb(Qt, lane, q, t.n_blocks, t.n_mel, lm);
        if constexpr (LOGMEL) logmel_store_mb(s, t, lm, prev, lo, q, lane_off, out);
        else dct_store_mb(s, t, lm, ax, prev, lo, q, lane_off, out);
    }
}

inline const char *kernel_name() { return "mfcc_fused512_h160_mb_kernel"; }

// returns false when the problem does not fit the kernel's 32-bit tile arithmetic; the geometry is the hop-160 form's
template <bool LOGMEL>
inline bool launch(const mfcc_k::StreamDesc &s, const Tables &t, float *out, int n_cu, hipStream_t stream) {
    LaunchGeom g;
    unsigned grid;
    if (!mfcc_fc::launch_geom(s, n_cu, {kTile, kTileHop160, kSUsed}, mfcc_fc::GridRule::kTwoPerCu, 31, g, grid)) return false;
    hipLaunchKernelGGL((mfcc_fused512_h160_mb_kernel<LOGMEL>), dim3(grid), dim3(64 * kWaves), 0, stream, s, t, g, out);
    return true;
}

}  // namespace mfcc_fused160mb
