// The tile geometry of a fused float kernel's launch: the kernel argument LaunchGeom and the one host function that
// fills it.  No HIP in here: the host tests compile this header on its own (tests/test_launch_geom_host.py).
#pragma once

#include <stdint.h>

namespace mfcc_fc {

struct LaunchGeom {
    int tiles_per_ch, n_ch, grid_div, grid_mod;      // grid = grid_div * tiles_per_ch + grid_mod
    long long step_ptr, wrap_ptr;                    // samples: ptr step per grid stride / extra step on carry
    int t_lo, t_hi;                                  // tiles t_lo <= t_in <= t_hi have their window inside the channel
};

// a kernel's constants: frames per tile, samples between consecutive tiles, samples of a tile's parked span
struct TileShape {
    int tile, tile_hop, s_used;
};

// how many workgroups run and how far the cursor strides
enum class GridRule {
    kTwoPerCu,       // min(n_tiles, 2 n_cu) workgroups, stride = workgroups
    kOnePerCu,       // min(n_tiles, n_cu) workgroups, stride = workgroups
    kPairs,          // the twelve-wave forms: clamp((n_tiles + 1) / 2, 1, n_cu) workgroups of two virtual ones, stride twice that
};

// Fills g and the number of workgroups to launch.  Returns false when the problem does not fit the kernel's 32-bit tile
// arithmetic: n_tiles or n_ch >= 2^guard_bits, or tiles_per_ch >= 2^26.
inline bool launch_geom(long long frames_per_ch, long long total_frames, long long ch_stride, long long n_samples, int halo,
                        int n_cu, TileShape k, GridRule rule, int guard_bits, LaunchGeom &g, unsigned &workgroups) {
    const long long tiles_per_ch = (frames_per_ch + k.tile - 1) / k.tile;
    const long long n_ch = total_frames / frames_per_ch;
    const long long n_tiles = tiles_per_ch * n_ch;
    if (n_tiles >= (1ll << guard_bits) || tiles_per_ch >= (1ll << 26) || n_ch >= (1ll << guard_bits)) return false;
    long long wgs = rule == GridRule::kPairs ? (n_tiles + 1) / 2 : n_tiles;
    const long long cap = rule == GridRule::kTwoPerCu ? (long long)n_cu * 2 : (long long)n_cu;
    if (wgs > cap) wgs = cap;
    if (wgs < 1) wgs = 1;
    const long long grid = rule == GridRule::kPairs ? 2 * wgs : wgs;     // the cursor stride
    g.tiles_per_ch = (int)tiles_per_ch;
    g.n_ch = (int)n_ch;
    g.grid_div = (int)(grid / tiles_per_ch);
    g.grid_mod = (int)(grid % tiles_per_ch);
    g.step_ptr = (long long)g.grid_div * ch_stride + (long long)g.grid_mod * k.tile_hop;
    g.wrap_ptr = ch_stride - tiles_per_ch * (long long)k.tile_hop;
    // the span of tile t_in: samples [t_in * tile_hop - mis - 2, t_in * tile_hop - mis + s_used), mis <= 7.  Tiles
    // t_lo .. t_hi have it inside the channel and load it with aligned 16-byte loads; every other tile goes sample by
    // sample, with the history before the channel and zeros from n_samples on
    g.t_lo = (int)((9 - (long long)halo + k.tile_hop - 1) / k.tile_hop);
    if (g.t_lo < 0) g.t_lo = 0;
    const long long hi = (n_samples - k.s_used) / k.tile_hop;
    g.t_hi = n_samples < k.s_used ? -1 : (int)(hi < tiles_per_ch ? hi : tiles_per_ch);
    workgroups = (unsigned)wgs;
    return true;
}

// ---- the sample decode (kernel_decode.hpp): a streaming pass, grid-stride over groups of kDecodeGroup samples per lane.
// x strides over the groups of a row, y over the rows; the grid comes from the CU count -- at most kDecodeBlocksPerCu
// workgroups per CU over both axes (32 waves per CU, what a CU holds) -- and is only cut where there are fewer groups
// than that.  One trip of the grid covers gx * kDecodeThreads groups of every row
constexpr int kDecodeThreads = 256, kDecodeGroup = 8, kDecodeBlocksPerCu = 8, kDecodeMaxRowsY = 65535;

inline void decode_grid(long long groups_per_row, long long rows, int n_cu, unsigned &gx, unsigned &gy) {
    long long y = rows < kDecodeMaxRowsY ? rows : kDecodeMaxRowsY;
    if (y < 1) y = 1;
    long long cap = (long long)n_cu * kDecodeBlocksPerCu / y;
    if (cap < 1) cap = 1;
    long long x = (groups_per_row + kDecodeThreads - 1) / kDecodeThreads;
    if (x > cap) x = cap;
    if (x < 1) x = 1;
    gx = (unsigned)x;
    gy = (unsigned)y;
}

}  // namespace mfcc_fc
