// The power-spectrum output (include/mfcc_hip.h: "power spectrum"): everything the host decides,
// with no HIP in it -- which kernel a handle's spectrum calls run, the store geometry of a fused tile and the limits of
// a call.  tests/spectrum_plan_driver.cpp prints all of it for tests/test_spectrum_host.py.
//
// The functions the kernel needs too are constexpr: hipcc compiles those for both sides, so the host and the device
// run the same lines.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mfcc_spec {

constexpr int kTile = 16;                      // frames of a fused tile (kernel_fused512.hpp: kTile)
constexpr int kFusedNfft = 512, kFusedBins = kFusedNfft / 2 + 1;
constexpr int kTileElems = kTile * kFusedBins; // 4112 floats: a full tile's rows, contiguous in the dense output
constexpr int kRWords = kTileElems + 4;        // the tile's LDS image: the rows behind a pad of 0..3 words (store_geom)

// bins of a row: nfft / 2 + 1
constexpr int bins(int nfft) { return nfft / 2 + 1; }

// ---- which kernel
enum class Kernel { kGeneric = 0, kFused512 = 1 };

// mfcc_spectrum512_kernel serves nfft 512 at hop 170 with the full frame, and at hop 160 with any frame of 160 .. 512
// samples; generic_impl: the handle asks for the generic kernels (MFCC_HIP_IMPL_GENERIC)
constexpr bool fused_supported(int nfft, int hop, int frame_len) {
    return nfft == kFusedNfft && ((hop == 170 && frame_len == kFusedNfft) || (hop == 160 && frame_len >= 160 && frame_len <= kFusedNfft));
}
constexpr Kernel choose(int nfft, int hop, int frame_len, bool generic_impl) {
    return !generic_impl && fused_supported(nfft, hop, frame_len) ? Kernel::kFused512 : Kernel::kGeneric;
}
constexpr const char *name_of(Kernel k) { return k == Kernel::kFused512 ? "mfcc_spectrum512_kernel" : "mfcc_spectrum_generic_kernel"; }

// ---- the store geometry of a fused tile.  The `rows` rows of a tile (16, fewer in the last tile of a channel) are
// rows * 257 consecutive floats of the dense output.  A row is only 4-byte aligned, so the span starts `pad` floats
// behind a 16-byte boundary: the kernel lays the rows out in LDS behind a pad of as many words, which makes a float's
// offset from a 16-byte boundary the same in LDS and in the output, and streams the image out as
//   head  floats [0, lead) one by one                (lead <= 3: up to the first boundary)
//   nvec  16-byte stores of floats [lead + 4 v, lead + 4 v + 4), every one 16-byte aligned on both sides
//   tail  floats [lead + 4 nvec, count) one by one   (tail <= 3)
// word: the float index of the span's first element, address / 4 (any 64-bit count of floats with the right low bits)
struct StoreGeom {
    int pad, lead, nvec, tail, count;
};
constexpr StoreGeom store_geom(unsigned long long word, int rows, int n_bins) {
    const int count = rows * n_bins;
    const int pad = int(word & 3ull);
    const int want = (4 - pad) & 3;
    const int lead = want < count ? want : count;
    const int nvec = (count - lead) / 4;
    return StoreGeom{pad, lead, nvec, count - lead - 4 * nvec, count};
}
// LDS word of element e of the span (row e / bins, bin e % bins), and of the span's vector v
constexpr int lds_word(const StoreGeom &g, int e) { return g.pad + e; }
constexpr int lds_vec_word(const StoreGeom &g, int v) { return g.pad + g.lead + 4 * v; }

// ---- limits.  The kernels index the output with 64-bit element counts; the host refuses what does not fit size_t
constexpr size_t kMaxElems = size_t(1) << 62;
// rows * bins floats (frames of all channels, or of all utterances): false when the count would pass kMaxElems
constexpr bool fits(size_t rows, size_t n_bins) { return n_bins == 0 || rows <= kMaxElems / n_bins; }
// a dense call of n_ch channels of n_samples each: no framing makes more than n_samples + 1 frames of a channel (hop >= 1)
constexpr bool call_fits(size_t n_samples, size_t n_ch, size_t n_bins) {
    return n_ch == 0 || (n_samples < kMaxElems && fits(n_ch, n_bins) && fits(n_samples + 1, n_ch * n_bins));
}
// a ragged call of n_utt utterances over span_samples samples in all: no framing makes more than n + 2 frames of an
// utterance of n samples (hop >= 1; the padded last frame of the stream framing), so span + 2 n_utt bounds the rows
constexpr bool ragged_fits(size_t span_samples, size_t n_utt, size_t n_bins) {
    return span_samples < kMaxElems / 4 && n_utt < kMaxElems / 4 && fits(span_samples + 2 * n_utt, n_bins);
}

}  // namespace mfcc_spec
