// Prints what mfcc_amd/csrc/fbank_plan.hpp decides, for tests/test_fbank_host.py.  One request per input line, one answer
// line each:
//   choose nfft hop frame_len generic_impl   -> kernel (0 generic, 1 fused) and its name
//   scale s                                  -> valid (0 / 1) and the factor c (%.9g)
//   floor v                                  -> 0 / 1   (v: anything strtof takes, "nan", "inf", "-0" included)
//   bands n                                  -> 0 / 1
//   table n_bands bins w...                  -> index of the first refused weight or -1 | per band "first count off nnz" |
//                                               packed floats, weights-in-LDS (0 / 1), blob bytes | the packed weights (%.9g)
//   sets n_bands bins w...                   -> build_sets' result (0 / 1) | the 8 block masks | the 8 first-set indices | sets,
//                                               operand dwords | non-zero weights held by exactly one operand slot, weights
//                                               (zero ones included) held by more than one, non-zero slots that hold no
//                                               weight of the matrix | worst |hi + lo - w| / w of the operands (%.9g)
//   tile rows n_bands                        -> elements of the tile's span | per store "element thread frame band"
//   callfits n_samples n_ch n_bands          -> 0 / 1
//   raggedfits span_samples n_utt n_bands    -> 0 / 1
//   range first count                        -> the packed word, and first and count read back from it
//   limits                                   -> kMaxBands kTile kImageWords kWLds kMaxBlocks kSteps
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fbank_plan.hpp"

int main() {
    std::string line;
    char num[64];
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        std::ostringstream os;
        if (cmd == "choose") {
            int nfft, hop, L, gen;
            is >> nfft >> hop >> L >> gen;
            const mfcc_fbank::Kernel k = mfcc_fbank::choose(nfft, hop, L, gen != 0);
            os << int(k) << ' ' << mfcc_fbank::name_of(k);
        } else if (cmd == "scale") {
            int sc;
            is >> sc;
            std::snprintf(num, sizeof num, "%.9g", double(mfcc_fbank::scale_factor(sc)));
            os << int(mfcc_fbank::valid_scale(sc)) << ' ' << num;
        } else if (cmd == "floor") {
            std::string v;
            is >> v;
            os << int(mfcc_fbank::valid_floor(std::strtof(v.c_str(), nullptr)));
        } else if (cmd == "bands") {
            long long n;
            is >> n;
            os << int(mfcc_fbank::valid_bands(n));
        } else if (cmd == "table") {
            int n_bands, bins;
            is >> n_bands >> bins;
            std::vector<float> w;
            std::string v;
            while (is >> v) w.push_back(std::strtof(v.c_str(), nullptr));
            if (n_bands < 1 || bins < 1 || w.size() != size_t(n_bands) * size_t(bins)) return 3;
            const long long bad = mfcc_fbank::first_bad_weight(w.data(), n_bands, bins);
            os << bad << " |";
            if (bad < 0) {
                const mfcc_fbank::Table t = mfcc_fbank::build_table(w.data(), n_bands, bins);
                for (int j = 0; j < n_bands; ++j) os << ' ' << t.first[j] << ' ' << t.count[j] << ' ' << t.off[j] << ' ' << t.nnz[j];
                const std::vector<char> blob = mfcc_fbank::build_blob(t);
                if (blob.size() != mfcc_fbank::blob_bytes(t.packed.size(), n_bands)) return 4;
                os << " | " << t.packed.size() << ' ' << int(mfcc_fbank::weights_in_lds(t.packed.size())) << ' ' << blob.size() << " |";
                for (float p : t.packed) {
                    std::snprintf(num, sizeof num, " %.9g", double(p));
                    os << num;
                }
            }
        } else if (cmd == "sets") {
            int n_bands, bins;
            is >> n_bands >> bins;
            std::vector<float> w;
            std::string v;
            while (is >> v) w.push_back(std::strtof(v.c_str(), nullptr));
            if (n_bands < 1 || bins < 1 || w.size() != size_t(n_bands) * size_t(bins)) return 3;
            mfcc_fbank::Sets st;
            os << int(mfcc_fbank::build_sets(w.data(), n_bands, bins, st)) << " |";
            for (uint32_t m : st.mask) os << ' ' << m;
            os << " |";
            for (int f : st.first) os << ' ' << f;
            os << " | " << st.n_sets << ' ' << st.a_bf.size() << " |";
            // the operands read back the way the kernel walks them: blocks ascending, listed steps ascending
            std::vector<int> hits(w.size(), 0);
            int once = 0, many = 0, stray = 0, i = 0;
            double worst = 0.0;
            for (int b = 0; b < mfcc_fbank::kMaxBlocks; ++b)
                for (int s = 0; s < mfcc_fbank::kSteps; ++s) {
                    if (!((st.mask[b] >> s) & 1)) continue;
                    if (i != st.first[b] + __builtin_popcount(st.mask[b] & ((1u << s) - 1))) return 5;
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const uint32_t hi = st.a_bf[((size_t(i) * 2 + 0) * 64 + l) * 4 + j / 2] >> (16 * (j & 1)) & 0xffffu;
                            const uint32_t lo = st.a_bf[((size_t(i) * 2 + 1) * 64 + l) * 4 + j / 2] >> (16 * (j & 1)) & 0xffffu;
                            const double val = double(mfcc_fbank::bf16_val(hi)) + double(mfcc_fbank::bf16_val(lo));
                            const int band = mfcc_fbank::set_band(b, l), bin = mfcc_fbank::set_bin(s, l, j);
                            if (band >= n_bands || bin >= bins) {
                                stray += val != 0.0;
                                continue;
                            }
                            const double ref = w[size_t(band) * bins + bin];
                            ++hits[size_t(band) * bins + bin];
                            if (ref == 0.0) stray += val != 0.0;
                            else if (std::fabs(val - ref) / ref > worst) worst = std::fabs(val - ref) / ref;
                        }
                    ++i;
                }
            if (i != st.n_sets) return 6;
            for (size_t k = 0; k < w.size(); ++k) {
                once += w[k] != 0.0f && hits[k] == 1;
                many += hits[k] > 1;
            }
            std::snprintf(num, sizeof num, "%.9g", worst);
            os << ' ' << once << ' ' << many << ' ' << stray << " | " << num;
        } else if (cmd == "tile") {
            int rows, n_bands;
            is >> rows >> n_bands;
            const int count = mfcc_fbank::tile_elems(rows, n_bands);
            os << count << " |";
            // kernel_fbank.hpp: the contraction loop of mfcc_fbank512_kernel, every lane's part in turn
            for (int tid = 0; tid < mfcc_fbank::kTileThreads; ++tid)
                for (int i = 0; i < mfcc_fbank::tile_steps(n_bands); ++i) {
                    const int j = mfcc_fbank::tile_band(tid, i), fr = mfcc_fbank::tile_frame(tid);
                    if (j < n_bands && fr < rows) os << ' ' << fr * n_bands + j << ' ' << tid << ' ' << fr << ' ' << j;
                }
        } else if (cmd == "range") {
            int first, cnt;
            is >> first >> cnt;
            const int w = mfcc_fbank::pack_range(first, cnt);
            os << w << ' ' << mfcc_fbank::range_first(w) << ' ' << mfcc_fbank::range_count(w);
        } else if (cmd == "callfits") {
            size_t n, nch, nb;
            is >> n >> nch >> nb;
            os << int(mfcc_fbank::call_fits(n, nch, nb));
        } else if (cmd == "raggedfits") {
            size_t span, n_utt, nb;
            is >> span >> n_utt >> nb;
            os << int(mfcc_fbank::ragged_fits(span, n_utt, nb));
        } else if (cmd == "limits") {
            os << mfcc_fbank::kMaxBands << ' ' << mfcc_fbank::kTile << ' ' << mfcc_fbank::kImageWords << ' ' << mfcc_fbank::kWLds << ' '
               << mfcc_fbank::kMaxBlocks << ' ' << mfcc_fbank::kSteps;
        } else {
            return 2;
        }
        std::puts(os.str().c_str());
    }
    return 0;
}
