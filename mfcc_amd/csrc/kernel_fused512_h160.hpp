// Fused 512-point float kernel at hop 160 with the window taken from the handle's frame length: the ASR framing
// (25 ms window, 10 ms hop, 512-point FFT at 16 kHz = 400 / 160 / 512), DESIGN.md section 4.11.
//
// This is the four-wave form of kernel_fused512.hpp -- a 16-frame tile per workgroup, the tile's sample span parked in
// LDS with the integer pre-emphasis, a windowed real FFT-32 over n1, a complex FFT-16 over n2, the bf16-split mel
// MFMAs straight from registers, the column-16 role, the fp32 DCT tail one tile behind -- with three differences:
//
//  hop     consecutive tiles are 16 * 160 = 2560 samples apart and frame fr of a tile starts at slot 160 fr of the
//          parked span.  A tile reads slots up to 7 + 15 * 160 + 511 = 2918 of the 3072 it parks.
//  window  a frame owns L samples (160 <= L <= 511) and is zero-padded to 512: FusedTables::win holds the handle's
//          window (periodic Hamming by default) of length L in its first L entries and zeros behind them (mfcc_fused::set_window).  The kernel
//          still reads 512 slots per frame; slots L .. 511 are finite (pre-emphasised int16, or the zeros the edge path
//          supplies beyond the channel) and meet a zero weight, so whatever follows the frame -- the next frame, the next
//          utterance of a packed batch, the padding -- does not reach its result.
//  log-mel the tail of a log-mel handle stores the n_mel log2 values instead of running the DCT (LOGMEL).
//
// The kernel is mfcc_fused::tile_loop_w4<160, DENSE, DCX, LOGMEL> of kernel_fused512.hpp: the hop-170 kernel's loop with
// the hop as a template parameter; tables and set_window are that file's too.
//
// LDS banks: a ds_read_b32 takes its bank from the dword address mod 32 and 160 = 0 (mod 32), so the two quarters of a
// 32-lane half (two frames, whatever their distance) read the same 16 banks: the 32 sample reads of pass 1 are 2-way
// conflicts here (at hop 170 the two quarters are 8 frames = 1360 samples = 16 (mod 32) banks apart, so their
// ds_read_b32 of the span never collide).  DESIGN.md section 4.11 has the account.
#pragma once

#include "kernel_fused512.hpp"

namespace mfcc_fused160 {

using namespace mfcc_fused;          // constants, FusedTables, Fetch and the device helpers shared with the hop-170 form

constexpr int kHop160 = 160;
constexpr int kTileHop160 = kTile * kHop160;   // 2560 samples (5120 bytes: a multiple of 16) between consecutive tiles
constexpr int kMinFrame = kHop160, kMaxFrame = kNfft - 1;

// the parameters this kernel covers; frame_len is the handle's frame length (below nfft: a framed handle)
inline bool supported(int nfft, int hop, int frame_len, int n_mel, int n_cep) {
    return nfft == kNfft && hop == kHop160 && frame_len >= kMinFrame && frame_len <= kMaxFrame &&
           (n_mel == kMel || n_mel == 16) && n_cep >= 1 && n_cep <= n_mel;
}

template <bool DENSE, bool DCX, bool LOGMEL>
__global__ __launch_bounds__(64 * kWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfcc_fused512_h160_kernel(mfcc_k::StreamDesc s, W4Tables t, LaunchGeom g, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[lds_words(kQWords, DCX)];
    tile_loop_w4<kHop160, DENSE, DCX, LOGMEL>(s, t, g, out, lds);
}

inline const char *kernel_name() { return "mfcc_fused512_h160_kernel"; }

// returns false when the problem does not fit the kernel's 32-bit tile arithmetic
template <bool LOGMEL>
inline bool launch(const mfcc_k::StreamDesc &s, const W4Tables &t, bool dense, float *out, int n_cu,
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
