// Prints what mfcc_amd/csrc/spectrum_plan.hpp decides, for tests/test_spectrum_host.py.  One request per input line, one
// answer line each:
//   choose nfft hop frame_len generic_impl   -> kernel (0 generic, 1 fused) and its name, fused_supported
//   bins nfft                                -> nfft / 2 + 1
//   store word rows bins                     -> pad lead nvec tail count | the stores in the kernel's order:
//                                               "s e w" a float (element e of the span, LDS word w),
//                                               "v e w" a 16-byte store (elements e .. e + 3, LDS words w .. w + 3)
//   fits rows bins                           -> 0 / 1
//   callfits n_samples n_ch bins             -> 0 / 1
//   raggedfits span_samples n_utt bins       -> 0 / 1
//   limits                                   -> kMaxElems kTile kTileElems kRWords
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "spectrum_plan.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        std::ostringstream os;
        if (cmd == "choose") {
            int nfft, hop, L, gen;
            is >> nfft >> hop >> L >> gen;
            const mfcc_spec::Kernel k = mfcc_spec::choose(nfft, hop, L, gen != 0);
            os << int(k) << ' ' << mfcc_spec::name_of(k) << ' ' << int(mfcc_spec::fused_supported(nfft, hop, L));
        } else if (cmd == "bins") {
            int nfft;
            is >> nfft;
            os << mfcc_spec::bins(nfft);
        } else if (cmd == "store") {
            unsigned long long word;
            int rows, n_bins;
            is >> word >> rows >> n_bins;
            const mfcc_spec::StoreGeom g = mfcc_spec::store_geom(word, rows, n_bins);
            os << g.pad << ' ' << g.lead << ' ' << g.nvec << ' ' << g.tail << ' ' << g.count << " |";
            // kernel_spectrum.hpp: store_tile, every lane's part in turn
            for (int e = 0; e < g.lead; ++e) os << " s " << e << ' ' << mfcc_spec::lds_word(g, e);
            for (int v = 0; v < g.nvec; ++v) os << " v " << g.lead + 4 * v << ' ' << mfcc_spec::lds_vec_word(g, v);
            const int t0 = g.lead + 4 * g.nvec;
            for (int e = 0; e < g.tail; ++e) os << " s " << t0 + e << ' ' << mfcc_spec::lds_word(g, t0 + e);
        } else if (cmd == "fits") {
            size_t rows, n_bins;
            is >> rows >> n_bins;
            os << int(mfcc_spec::fits(rows, n_bins));
        } else if (cmd == "callfits") {
            size_t n, nch, n_bins;
            is >> n >> nch >> n_bins;
            os << int(mfcc_spec::call_fits(n, nch, n_bins));
        } else if (cmd == "raggedfits") {
            size_t span, n_utt, n_bins;
            is >> span >> n_utt >> n_bins;
            os << int(mfcc_spec::ragged_fits(span, n_utt, n_bins));
        } else if (cmd == "limits") {
            os << mfcc_spec::kMaxElems << ' ' << mfcc_spec::kTile << ' ' << mfcc_spec::kTileElems << ' ' << mfcc_spec::kRWords;
        } else {
            return 2;
        }
        std::puts(os.str().c_str());
    }
    return 0;
}
