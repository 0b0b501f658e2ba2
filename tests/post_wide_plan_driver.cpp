// The host plan of the filterbank post-passes (tests/test_fbank_post_host.py): what mfcc_amd/csrc/post_plan.hpp makes of
// the tiles of the narrow and the wide kernels, and what seg_plan.hpp lays out for the scratch of a pass at their widths.
//   tiles              first the line
//                        kDeltaLdsFloats kDeltaWideLdsFloats kNarrowWidth kWideWidth kNormTileFloats kWideGroupsPerCu
//                      then for every width 1 .. 128, order 1 .. 2, window 1 .. 8 the line
//                        width order window delta_tile_rows delta_wide_tile_rows delta_lds_floats(of the wide tile)
//                        norm_tile_rows norm_stripes wide_rows
//   grid n_tiles n_cu  wide_grid(n_tiles, n_cu)
//   scratch            reads "width tile_rows n_segs off[0] .. off[n_segs]" and prints, for the areas of normalize_pass
//                      (W * 24 bytes per tile, W * 8 per segment) and then of pcen_pass (W * 4 per tile, twice), the line
//                        n_blocks n_segs table_ll off[0] off[1] table_off total
#include <stdio.h>
#include <string.h>

#include <vector>

#include "post_plan.hpp"
#include "seg_plan.hpp"

int main(int argc, char **argv) {
    using namespace mfcc_post;
    if (argc >= 2 && !strcmp(argv[1], "tiles")) {
        printf("%d %d %d %d %d %d\n", kDeltaLdsFloats, kDeltaWideLdsFloats, kNarrowWidth, kWideWidth, kNormTileFloats, kWideGroupsPerCu);
        for (int w = 1; w <= 128; ++w)
            for (int order = 1; order <= 2; ++order)
                for (int window = 1; window <= kMaxDeltaWindow; ++window) {
                    const int g = delta_wide_tile_rows(w, order, window);
                    printf("%d %d %d %d %d %d %d %d %d\n", w, order, window, delta_tile_rows(w, order, window), g,
                           delta_lds_floats(g, w, order, window), norm_tile_rows(w), norm_stripes(w), int(wide_rows(w)));
                }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "grid")) {
        long long n = 0;
        int n_cu = 0;
        if (sscanf(argv[2], "%lld", &n) != 1 || sscanf(argv[3], "%d", &n_cu) != 1) return 2;
        printf("%u\n", wide_grid(n, n_cu));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "scratch")) {
        using namespace mfcc_seg;
        int width, tile_rows;
        size_t n_segs;
        if (scanf("%d %d %zu", &width, &tile_rows, &n_segs) != 3) return 2;
        std::vector<size_t> off(n_segs + 1);
        for (size_t &v : off)
            if (scanf("%zu", &v) != 1) return 2;
        Plan pl;
        if (plan_count(span_offsets(off.data(), n_segs), width, tile_rows, nullptr, pl)) return 3;
        const size_t W = size_t(width);
        const Area norm[] = {{W * 24, 0, 0}, {0, W * 8, 0}}, pcen[] = {{W * 4, 0, 0}, {W * 4, 0, 0}};
        for (const Area *a : {norm, pcen}) {
            const Scratch l = lay_out(a, 2, pl);
            printf("%lld %lld %zu %zu %zu %zu %zu\n", pl.s.n_blocks, pl.s.n_segs, pl.table_ll, l.off[0], l.off[1], l.table_off, l.total);
        }
        return 0;
    }
    return 2;
}
