// The filterbank output (include/mfcc_hip.h: "filterbank"): everything the host decides, with no
// HIP in it -- which kernel a handle's filterbank calls run, whether a matrix and its parameters are taken, the bin
// range of every band, the scale's factor, the LDS of the fused tile and the limits of a call.
// tests/fbank_plan_driver.cpp prints all of it for tests/test_fbank_host.py.
//
// The functions the kernels need too are constexpr: hipcc compiles those for both sides.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "spectrum_plan.hpp"

namespace mfcc_fbank {

constexpr int kMaxBands = 128;                 // MFCC_HIP_MAX_FBANK_BANDS
constexpr int kTile = mfcc_spec::kTile;        // frames of a fused tile

// ---- which kernel.  mfcc_fbank512_kernel serves the shapes of the fused spectrum kernel (mfcc_spec::fused_supported);
// generic_impl: the handle asks for the generic kernels (MFCC_HIP_IMPL_GENERIC)
enum class Kernel { kGeneric = 0, kFused512 = 1 };
constexpr Kernel choose(int nfft, int hop, int frame_len, bool generic_impl) {
    return !generic_impl && mfcc_spec::fused_supported(nfft, hop, frame_len) ? Kernel::kFused512 : Kernel::kGeneric;
}
constexpr const char *name_of(Kernel k) { return k == Kernel::kFused512 ? "mfcc_fbank512_kernel" : "mfcc_fbank_generic_kernel"; }

// ---- the scale of a row (enum mfcc_hip_fbank_scale): y = E, or c * log2(max(E, floor))
constexpr int kEnergy = 0, kLog2 = 1, kLn = 2, kLog10 = 3;
constexpr bool valid_scale(int scale) { return scale >= kEnergy && scale <= kLog10; }
// c of the scale: 1, (float)ln 2, (float)log10 2; 0 for ENERGY (no log)
constexpr float scale_factor(int scale) {
    return scale == kLog2 ? 1.0f : scale == kLn ? float(0.693147180559945309417) : scale == kLog10 ? float(0.301029995663981195214) : 0.0f;
}
// finite and >= 0 (-0.0 counts as 0; NaN fails every comparison)
inline bool valid_floor(float v) { return v >= 0.0f && std::isfinite(v); }
inline bool valid_bands(long long n_bands) { return n_bands >= 1 && n_bands <= kMaxBands; }

// ---- the matrix.  Every weight finite and not negative; -0.0 counts as 0.  Returns the index of the first weight that
// is refused, or -1
inline long long first_bad_weight(const float *w, int n_bands, int bins) {
    for (long long i = 0; i < (long long)n_bands * bins; ++i)
        if (!(w[i] >= 0.0f) || !std::isfinite(w[i])) return i;
    return -1;
}

// What the kernels read: per band the first non-zero bin and the number of bins up to the last non-zero one (0 bins,
// first 0: an empty band), and the weights of exactly those bins, packed band after band, every zero inside a range a
// +0.0.  The generic kernel and the fused one both sum fmaf(W[j][k], P[k], acc) over that range, ascending
struct Table {
    int n_bands = 0, bins = 0;
    std::vector<float> packed;            // band j: packed[off[j] + i] = W[j][first[j] + i], i < count[j]
    std::vector<int> first, count, off;   // [n_bands]
    std::vector<int> nnz;                 // [n_bands] non-zero weights of the band (the error bound's count)
};
// w: a matrix first_bad_weight() passes
inline Table build_table(const float *w, int n_bands, int bins) {
    Table t;
    t.n_bands = n_bands;
    t.bins = bins;
    t.first.assign(n_bands, 0);
    t.count.assign(n_bands, 0);
    t.off.assign(n_bands, 0);
    t.nnz.assign(n_bands, 0);
    for (int j = 0; j < n_bands; ++j) {
        const float *row = w + size_t(j) * bins;
        int lo = bins, hi = -1;
        for (int k = 0; k < bins; ++k)
            if (row[k] != 0.0f) {
                if (k < lo) lo = k;
                hi = k;
                ++t.nnz[j];
            }
        t.off[j] = int(t.packed.size());
        if (hi < lo) continue;
        t.first[j] = lo;
        t.count[j] = hi - lo + 1;
        for (int k = lo; k <= hi; ++k) t.packed.push_back(row[k] != 0.0f ? row[k] : 0.0f);       // -0.0 -> +0.0
    }
    return t;
}
// the device blob of a table: the packed weights, then [n_bands] x (first, count, off, 0) int32, 16-byte aligned
constexpr size_t align16(size_t n) { return (n + 15) & ~size_t(15); }
constexpr size_t blob_bands(size_t n_packed) { return align16(n_packed * 4); }
constexpr size_t blob_bytes(size_t n_packed, int n_bands) { return blob_bands(n_packed) + size_t(n_bands) * 16; }
inline std::vector<char> build_blob(const Table &t) {
    std::vector<char> blob(blob_bytes(t.packed.size(), t.n_bands), 0);
    float *wp = reinterpret_cast<float *>(blob.data());
    for (size_t i = 0; i < t.packed.size(); ++i) wp[i] = t.packed[i];
    int32_t *bp = reinterpret_cast<int32_t *>(blob.data() + blob_bands(t.packed.size()));
    for (int j = 0; j < t.n_bands; ++j) {
        bp[4 * j + 0] = t.first[j];
        bp[4 * j + 1] = t.count[j];
        bp[4 * j + 2] = t.off[j];
    }
    return blob;
}

// ---- the fused tile.  Its 16 rows of n_bands values are one contiguous span of the dense output (mfcc_spec::store_geom
// takes the row width); every lane stores its own float (tile_frame, tile_band below), so no alignment beyond the float's
// own is needed.  Its LDS is that of mfcc_spectrum512_kernel -- T | V | S | the power image of the tile -- for
// every band count (the image is read, not stored, and its pad is 0) plus kWLds floats of packed weights: a matrix whose
// packed weights fit is staged there once per workgroup, a larger one runs the MFMA form below; and the band table,
// two words per band
constexpr int kImageWords = mfcc_spec::kTileElems;
constexpr int kWLds = 3072;
constexpr bool weights_in_lds(size_t n_packed) { return n_packed <= size_t(kWLds); }
constexpr int tile_elems(int rows, int n_bands) { return rows * n_bands; }
constexpr int kTileThreads = 256, kTileWaves = 4;
// Who computes what of a tile: the 16 lanes of a quarter of a wave hold the 16 frames of ONE band (lane & 15 is the
// frame, as in pass 2), the four quarters four consecutive bands, and wave w takes the band groups w, w + 4, ...: a
// quarter's weight reads are one LDS word (a broadcast), its power reads 16 words at stride 257, one bank each, and the
// four bands of a wave have ranges of about the same length.  Step i of thread tid: band tile_band(tid, i), or past
// n_bands
constexpr int tile_frame(int tid) { return tid & 15; }
constexpr int tile_band(int tid, int i) { return 4 * ((tid >> 6) + kTileWaves * i) + ((tid >> 4) & 3); }
constexpr int tile_steps(int n_bands) { return (n_bands + 4 * kTileWaves - 1) / (4 * kTileWaves); }
// a band's (first bin, bins) as one word of the kernel's LDS copy of the band table
constexpr int pack_range(int first, int count) { return first | (count << 16); }
constexpr int range_first(int packed) { return packed & 0xffff; }
constexpr int range_count(int packed) { return packed >> 16; }

// ---- the MFMA form of the fused tile: what a matrix whose packed weights do not fit kWLds runs (a dense or learned
// matrix, banks of long tails).  The contraction is the bf16-split one of kernel_fused512_h160_mb.hpp -- W = Wh + Wl,
// P = Ph + Pl, three 16 x 16 x 32 MFMAs (Wh Ph, Wh Pl, Wl Ph) per set into fp32 -- over the tile's power image, so a K
// step is 32 CONSECUTIVE bins (step s: bins 32 s .. 32 s + 31; nine steps, bins past 256 carry no weight and a zero
// power) and a set is a (block of 16 bands, K step) pair.  The host lists the sets that hold a non-zero weight as one
// 9-bit mask per block and builds the operands of exactly those, blocks ascending, steps ascending inside a block.
// Wave w contracts blocks w and w + 4 over all their listed steps, so no partial sums meet anywhere.
// Operand of a set, two terms (hi, lo): lane l holds band 16 block + (l & 15) at K slots j = 0 .. 7 <-> bin
// 32 s + 8 (l >> 4) + j; dword d = slots (2 d, 2 d + 1), the even one low (mfcc_fused::bf16_split8's layout)
constexpr int kBlockBands = 16, kMaxBlocks = kMaxBands / kBlockBands, kStepBins = 32, kSteps = 9;
constexpr int blocks_of(int n_bands) { return (n_bands + kBlockBands - 1) / kBlockBands; }
constexpr int set_bin(int step, int lane, int j) { return kStepBins * step + 8 * (lane >> 4) + j; }
constexpr int set_band(int block, int lane) { return kBlockBands * block + (lane & 15); }
inline uint32_t bf16_round(float v) {                    // round to nearest even, like v_cvt_pk_bf16_f32
    uint32_t u;
    std::memcpy(&u, &v, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
inline float bf16_val(uint32_t h) {
    const uint32_t u = h << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
struct Sets {
    uint32_t mask[kMaxBlocks] = {};       // bit s of mask[b]: set (b, s) is listed
    int first[kMaxBlocks] = {};           // sets listed in front of block b
    int n_sets = 0;
    std::vector<uint32_t> a_bf;           // [n_sets][hi, lo][64 lanes][4 dwords]
    std::vector<int> covered;             // [n_bands][bins]: how many listed operand slots hold the weight
};
// w: a matrix first_bad_weight() passes, bins <= kSteps * kStepBins.  Returns false when a non-zero weight is not held
// by exactly one slot of a listed set (never, by construction: the check of kernel_fused512_h160_mb.hpp, kept)
inline bool build_sets(const float *w, int n_bands, int bins, Sets &st) {
    st = Sets{};
    if (bins > kSteps * kStepBins || n_bands > kMaxBands) return false;
    auto W = [&](int band, int bin) { return band < n_bands && bin < bins ? w[size_t(band) * bins + bin] : 0.0f; };
    for (int b = 0; b < blocks_of(n_bands); ++b) {
        st.first[b] = st.n_sets;
        for (int s = 0; s < kSteps; ++s) {
            bool any = false;
            for (int m = 0; m < kBlockBands && !any; ++m)
                for (int k = 0; k < kStepBins && !any; ++k) any = W(kBlockBands * b + m, kStepBins * s + k) != 0.0f;
            if (any) st.mask[b] |= 1u << s, ++st.n_sets;
        }
    }
    for (int b = blocks_of(n_bands); b < kMaxBlocks; ++b) st.first[b] = st.n_sets;
    st.a_bf.assign(size_t(st.n_sets) * 2 * 64 * 4, 0u);
    st.covered.assign(size_t(n_bands) * bins, 0);
    int i = 0;
    for (int b = 0; b < blocks_of(n_bands); ++b)
        for (int s = 0; s < kSteps; ++s) {
            if (!((st.mask[b] >> s) & 1)) continue;
            for (int l = 0; l < 64; ++l) {
                uint32_t hi[8], lo[8];
                for (int j = 0; j < 8; ++j) {
                    const int band = set_band(b, l), bin = set_bin(s, l, j);
                    const float v = W(band, bin);
                    hi[j] = bf16_round(v);
                    lo[j] = bf16_round(v - bf16_val(hi[j]));
                    if (band < n_bands && bin < bins) ++st.covered[size_t(band) * bins + bin];
                }
                for (int d = 0; d < 4; ++d) {
                    st.a_bf[((size_t(i) * 2 + 0) * 64 + l) * 4 + d] = hi[2 * d] | (hi[2 * d + 1] << 16);
                    st.a_bf[((size_t(i) * 2 + 1) * 64 + l) * 4 + d] = lo[2 * d] | (lo[2 * d + 1] << 16);
                }
            }
            ++i;
        }
    for (int j = 0; j < n_bands; ++j)
        for (int k = 0; k < bins; ++k)
            if (W(j, k) != 0.0f && st.covered[size_t(j) * bins + k] != 1) return false;
    return true;
}

// the device blob of a matrix that runs the MFMA form: build_blob's, then the operands (16-byte aligned)
inline std::vector<char> build_blob(const Table &t, const Sets &st) {
    std::vector<char> blob = build_blob(t);
    const size_t at = blob.size();
    blob.resize(at + st.a_bf.size() * 4);
    if (!st.a_bf.empty()) std::memcpy(blob.data() + at, st.a_bf.data(), st.a_bf.size() * 4);
    return blob;
}

// ---- limits: those of the spectrum output with the row width n_bands
constexpr bool call_fits(size_t n_samples, size_t n_ch, size_t n_bands) { return mfcc_spec::call_fits(n_samples, n_ch, n_bands); }
constexpr bool ragged_fits(size_t span_samples, size_t n_utt, size_t n_bands) {
    return mfcc_spec::ragged_fits(span_samples, n_utt, n_bands);
}

}  // namespace mfcc_fbank
