// The tile sizes of the segment passes behind the float kernels, narrow (rows of 1 .. 64 floats: kernel_normalize.hpp,
// kernel_deltas.hpp, the kernels of mfcc_hip.hip) and wide (65 .. 128 floats: the same lines compiled into post_wide.hip
// for the filterbank post-passes), and the grid of the wide kernels.  Which form runs is decided
// by the row width alone (normalize_pass, deltas_pass).  No HIP in here: the host tests compile this header on its own
// (tests/test_fbank_post_host.py).
#pragma once

namespace mfcc_post {

constexpr int kThreads = 256;
constexpr int kNarrowWidth = 64;       // the widest row of the narrow kernels, and of every direct entry on rows
constexpr int kWideWidth = 128;        // ... of the wide ones: MFCC_HIP_MAX_FBANK_BANDS
constexpr bool wide_rows(int width) { return width > kNarrowWidth; }

// ---- per-segment normalization: a stats tile is kNormTileFloats of LDS whatever the width, and a workgroup's threads
// form G = 256 / W stripes of W columns (3 for 65 .. 85 floats, 2 for 86 .. 128).  Both forms: only the width-sized LDS
// arrays differ
constexpr int kNormTileFloats = 8192;
constexpr int norm_tile_rows(int width) { return kNormTileFloats / width; }
constexpr int norm_stripes(int width) { return kThreads / width; }

// ---- deltas: rows per tile, what fits in lds_floats with the halos.  K = 1: (T + 2N) W static + T 2W output floats;
// K = 2: (T + 4N) W static + (T + 2N) W delta + T 3W output floats; 8 floats of slack for the alignment of the output copy
constexpr int kDeltaLdsFloats = 4096;              // 16 KB: the narrow kernel, at least 3 rows for every W <= 64, N <= 8
#ifndef MFCC_POST_WIDE_LDS_FLOATS
#define MFCC_POST_WIDE_LDS_FLOATS 13312            // (a build for tools/fbank_post_rate.py sets a size that was rejected)
#endif
// 52 KB: the wide one, at least 11 rows for every W <= 128, N <= 8, and three workgroups on a CU's 160 KB.  Measured
// against 48 KB (9 rows) and 64 KB (15 rows, two workgroups): DESIGN.md section 4.22
constexpr int kDeltaWideLdsFloats = MFCC_POST_WIDE_LDS_FLOATS;
constexpr int kMaxDeltaWindow = 8;
constexpr int delta_tile_rows_of(int lds_floats, int width, int order, int window) {
    return order == 1 ? ((lds_floats - 8) / width - 2 * window) / 3 : ((lds_floats - 8) / width - 6 * window) / 5;
}
constexpr int delta_tile_rows(int width, int order, int window) {
    return delta_tile_rows_of(kDeltaLdsFloats, width, order, window);
}
constexpr int delta_wide_tile_rows(int width, int order, int window) {
    return delta_tile_rows_of(kDeltaWideLdsFloats, width, order, window);
}
// the floats a tile of `rows` rows takes of the delta kernel's LDS: static rows, D rows (order 2), the output copy rounded
// up to a float4 in front and moved by up to 3 floats (pad) behind
constexpr int delta_lds_floats(int rows, int width, int order, int window) {
    return (((rows + 2 * order * window) * width + (order == 2 ? (rows + 2 * window) * width : 0) + 3) & ~3) + 3 +
           rows * width * (1 + order);
}

// ---- the grid of a wide kernel over n tiles: a queue of eight workgroups per CU, which walk the tiles with the stride
// of the grid (three of the delta kernel's 52 KB, four of the stats kernel's 37 KB are resident on a CU at a time)
constexpr int kWideGroupsPerCu = 8;
inline unsigned wide_grid(long long n_tiles, int n_cu) {
    const long long cap = (long long)(n_cu > 0 ? n_cu : 1) * kWideGroupsPerCu;
    return unsigned(n_tiles < cap ? n_tiles : cap);
}

}  // namespace mfcc_post
