// Prints what mfcc_amd/csrc/center_plan.hpp decides, for tests/test_center_plan_host.py.  One request per input line, one
// answer line each (mode: 1 reflect, 2 zeros):
//   geom nfft L hop mode n                  -> PL F N'
//   plan nfft L hop mode first n_utt len*   -> total n_live max_padded stride8 | own'[0 .. n_utt] | the n_utt records
//        (utterance u lies at first + the lengths before it; the records are written into a buffer of exactly
//        n_utt * kRecLL entries; stride8 = dense_stride(max_padded, 2))
//   run nfft L hop mode n x[0] .. x[n-1]    -> the N' samples of center_host (into a buffer of exactly N')
//   src nfft L hop mode n                   -> source(i) for every i in [0, N'): every index the kernel may read
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "center_plan.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        int nfft, L, hop, mode;
        is >> cmd >> nfft >> L >> hop >> mode;
        const mfcc_center::Geom g = mfcc_center::geometry(nfft, L, hop, mode);
        std::ostringstream os;
        if (cmd == "geom") {
            size_t n;
            is >> n;
            os << g.left << ' ' << mfcc_center::frames(g, n) << ' ' << mfcc_center::padded(g, n);
        } else if (cmd == "plan") {
            size_t first, n_utt;
            is >> first >> n_utt;
            std::vector<size_t> own(n_utt + 1, first), own2(n_utt + 1, 77);
            for (size_t u = 0; u < n_utt; ++u) {
                size_t len;
                is >> len;
                own[u + 1] = own[u] + len;
            }
            std::vector<long long> recs(n_utt * mfcc_center::kRecLL);
            const mfcc_center::Table t = mfcc_center::fill_table(g, own.data(), n_utt, 0, own2.data(), recs.data());
            os << t.total << ' ' << t.n_live << ' ' << t.max_padded << ' ' << mfcc_center::dense_stride(t.max_padded, 2);
            for (size_t v : own2) os << ' ' << v;
            for (long long v : recs) os << ' ' << v;
        } else if (cmd == "run") {
            size_t n;
            is >> n;
            std::vector<int16_t> x(n);
            for (auto &v : x) {
                int w;
                is >> w;
                v = int16_t(w);
            }
            std::vector<int16_t> p(mfcc_center::padded(g, n));
            mfcc_center::center_host(g, x.data(), n, p.data());
            for (size_t i = 0; i < p.size(); ++i) os << (i ? " " : "") << p[i];
        } else if (cmd == "src") {
            long long n;
            is >> n;
            const long long np = (long long)mfcc_center::padded(g, size_t(n));
            for (long long i = 0; i < np; ++i) os << (i ? " " : "") << mfcc_center::source(g, i, n);
        } else {
            return 2;
        }
        std::puts(os.str().c_str());
    }
    return 0;
}
