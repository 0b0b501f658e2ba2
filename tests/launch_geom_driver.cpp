// Prints what mfcc_fc::launch_geom makes of every case on stdin (tests/test_launch_geom_host.py).  A case is one line:
//   frames_per_ch total_frames ch_stride n_samples halo n_cu tile tile_hop s_used rule guard_bits
// and its answer one line: ok workgroups tiles_per_ch n_ch grid_div grid_mod step_ptr wrap_ptr t_lo t_hi
#include <stddef.h>
#include <stdio.h>

#include "launch_geom.hpp"

int main() {
    using namespace mfcc_fc;
    // the struct is a kernel argument: its layout first
    printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(LaunchGeom), offsetof(LaunchGeom, tiles_per_ch),
           offsetof(LaunchGeom, n_ch), offsetof(LaunchGeom, grid_div), offsetof(LaunchGeom, grid_mod),
           offsetof(LaunchGeom, step_ptr), offsetof(LaunchGeom, wrap_ptr), offsetof(LaunchGeom, t_lo),
           offsetof(LaunchGeom, t_hi));
    long long frames_per_ch, total_frames, ch_stride, n_samples;
    int halo, n_cu, tile, tile_hop, s_used, rule, guard_bits;
    while (scanf("%lld %lld %lld %lld %d %d %d %d %d %d %d", &frames_per_ch, &total_frames, &ch_stride, &n_samples, &halo,
                 &n_cu, &tile, &tile_hop, &s_used, &rule, &guard_bits) == 11) {
        LaunchGeom g = {};
        unsigned workgroups = 0;
        const bool ok = launch_geom(frames_per_ch, total_frames, ch_stride, n_samples, halo, n_cu,
                                    TileShape{tile, tile_hop, s_used}, GridRule(rule), guard_bits, g, workgroups);
        printf("%d %u %d %d %d %d %lld %lld %d %d\n", int(ok), workgroups, g.tiles_per_ch, g.n_ch, g.grid_div, g.grid_mod,
               g.step_ptr, g.wrap_ptr, g.t_lo, g.t_hi);
    }
    return 0;
}
