// Prints what mfcc_amd/csrc/resample_plan.hpp decides, for tests/test_resample_host.py.  One request per input line, one
// answer line each:
//   geom in_rate out_rate             -> rc L M H K staged span_cap lds_bytes
//   count L M H c                     -> count(c) emitted(c)
//   plan in_rate out_rate lim_len lim_tiles n_seg (in_addr n out_addr m0 m1 c0 hist_addr hist_new_addr)*
//        -> ok n_tiles seg_ll tile_off_ll total_ll bytes | the total_ll records | per tile: seg t ma mb base groups
//      (a limit of 0 is the default one; the history tile t = -1 prints zeros behind t).  The records are written into
//      a buffer of exactly total_ll entries.
//   run in_rate out_rate m0 m1 n x[0] .. x[n-1]   -> the outputs [m0, m1) of resample_host
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "resample_plan.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        std::ostringstream os;
        if (cmd == "geom") {
            long long a, b;
            is >> a >> b;
            mfcc_rs::Geometry g;
            const int rc = mfcc_rs::geometry(a, b, g);
            os << rc << ' ' << g.L << ' ' << g.M << ' ' << g.H << ' ' << g.K;
            if (!rc)
                os << ' ' << int(mfcc_rs::staged(g.L, g.M, g.K)) << ' ' << mfcc_rs::span_cap(g.L, g.M, g.K) << ' '
                   << mfcc_rs::lds_bytes(g.L, g.M, g.K);
        } else if (cmd == "count") {
            int L, M, H;
            unsigned long long c;
            is >> L >> M >> H >> c;
            os << mfcc_rs::count(c, L, M) << ' ' << mfcc_rs::emitted(c, L, M, H);
        } else if (cmd == "plan") {
            long long a, b;
            size_t lim_len, lim_tiles, n_seg;
            is >> a >> b >> lim_len >> lim_tiles >> n_seg;
            mfcc_rs::Geometry g;
            if (mfcc_rs::geometry(a, b, g)) return 2;
            std::vector<mfcc_rs::SegIn> segs(n_seg);
            for (auto &s : segs) is >> s.in >> s.n >> s.out >> s.m0 >> s.m1 >> s.c0 >> s.hist >> s.hist_new;
            mfcc_rs::Limits lim;
            if (lim_len) lim.len = lim_len;
            if (lim_tiles) lim.tiles = lim_tiles;
            mfcc_rs::CallPlan pl;
            const bool ok = mfcc_rs::plan_call(segs.data(), n_seg, pl, lim);
            os << int(ok);
            if (ok) {
                os << ' ' << pl.n_tiles << ' ' << pl.seg_ll << ' ' << pl.tile_off_ll << ' ' << pl.total_ll << ' ' << pl.bytes;
                std::vector<long long> d(pl.total_ll);
                mfcc_rs::fill_call(segs.data(), n_seg, pl, d.data());
                for (long long v : d) os << ' ' << v;
                for (size_t i = 0; i < pl.n_tiles; ++i) {
                    const long long s = d[pl.tile_off_ll + i * mfcc_rs::kTileLL], t = d[pl.tile_off_ll + i * mfcc_rs::kTileLL + 1];
                    const long long *sr = d.data() + s * mfcc_rs::kSegLL;
                    mfcc_rs::TileSpan sp{0, 0, 0, 0};
                    if (t != mfcc_rs::kHistoryTile)
                        sp = mfcc_rs::tile_span(t, mfcc_rs::lead_of(uintptr_t(sr[2])), sr[3], sr[4], sr[5], uintptr_t(sr[0]), g.L, g.M,
                                                g.H);
                    os << ' ' << s << ' ' << t << ' ' << sp.ma << ' ' << sp.mb << ' ' << sp.base << ' ' << sp.groups;
                }
            }
        } else if (cmd == "run") {
            long long a, b, m0, m1, n;
            is >> a >> b >> m0 >> m1 >> n;
            mfcc_rs::Geometry g;
            std::vector<int16_t> t;
            if (mfcc_rs::geometry(a, b, g) || !mfcc_rs::build_taps(g, t)) return 2;
            std::vector<int16_t> x(n), y(m1 - m0);
            for (auto &v : x) {
                int w;
                is >> w;
                v = int16_t(w);
            }
            mfcc_rs::resample_host(g, t.data(), x.data(), n, m0, m1, y.data());
            for (size_t i = 0; i < y.size(); ++i) os << (i ? " " : "") << y[i];
        } else {
            return 2;
        }
        std::puts(os.str().c_str());
    }
    return 0;
}
