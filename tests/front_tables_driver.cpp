// Host driver of the four-wave table builders with a front (tests/test_front_host.py).  One case per input line:
//   window symmetric num den frame_len
// builds mfcc_fused::build_tables<true> (+ set_window when frame_len < 512) and mfcc_fused160mb::build_tables on the
// HTK bank of 40 filters from 20 Hz for the front's window and pair, and checks, entry by entry:
//   win      [16 n2][32 n1] == float(w[16 n1 + n2] / (2 den))       (both builders)
//   win_dc   [16 n2][32 n1] == w[16 n1 + n2] / den in double
//   the packed pair == (int16 -num, int16 den), as bind_tables hands it to the kernels
//   a pair with num + den = 128 is refused by both builders
// Prints "ok <entries checked>" or "FAIL <what>" per case.  No GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kernel_fused512_h160_mb.hpp"
#include "kernel_spectrum.hpp"

static const char *check_case(int window, int symmetric, int num, int den, int L, long &checked) {
    using namespace mfcc_tables;
    Front f;
    f.window = window, f.symmetric = symmetric, f.num = num, f.den = den;
    std::vector<double> w = front_window(f, L);
    w.resize(mfcc_fused::kNfft, 0.0);
    const std::vector<double> w512 = front_window(f, mfcc_fused::kNfft);

    std::vector<char> blob;
    if (!mfcc_fused::build_tables<true>(16000, 512.0, 0.0, 13, 32, w512, num, den, blob)) return "four-wave builder refused";
    if (L < mfcc_fused::kNfft) mfcc_fused160::set_window(blob, true, w, den);
    const mfcc_fused::BlobOffsets o = mfcc_fused::blob_offsets(true);
    const float *win = reinterpret_cast<const float *>(blob.data() + o.win);
    const double *wdc = reinterpret_cast<const double *>(blob.data() + o.win_dc);
    for (int n2 = 0; n2 < 16; ++n2)
        for (int n1 = 0; n1 < 32; ++n1) {
            const double v = w[16 * n1 + n2];
            if (win[n2 * 32 + n1] != float(v / (2.0 * double(den)))) return "four-wave win row";
            if (wdc[n2 * 32 + n1] != v / double(den)) return "four-wave win_dc row";
            checked += 2;
        }

    const std::vector<double> md = mel_dense_htk(512, 40, 16000.0, 20.0, 8000.0);
    std::vector<char> mb;
    uint32_t mask = 0;
    if (!mfcc_fused160mb::build_tables(md, 40, 13, w, den, 512.0, 0.0, mb, mask)) return "bank builder refused";
    const float *mwin = reinterpret_cast<const float *>(mb.data());
    for (int n2 = 0; n2 < 16; ++n2)
        for (int n1 = 0; n1 < 32; ++n1) {
            if (mwin[n2 * 32 + n1] != float(w[16 * n1 + n2] / (2.0 * double(den)))) return "bank win row";
            ++checked;
        }

    // the power tile's rows
    std::vector<char> sp;
    mfcc_spec::build_tables(w, sp, den);
    const float *swin = reinterpret_cast<const float *>(sp.data() + mfcc_spec::kBlobWin);
    for (int i = 0; i < 16 * 32; ++i, ++checked)
        if (swin[i] != mwin[i]) return "spectrum win row";

    // the pair as the kernels get it
    const int pair = packed_preemph(num, den);
    if (int16_t(pair & 0xffff) != int16_t(-num) || int16_t(uint32_t(pair) >> 16) != int16_t(den)) return "packed pair";
    mfcc_fused160mb::Tables tm{};
    mfcc_fused160mb::bind_tables(mb.data(), 13, 40, mask, tm, pair);
    mfcc_spec::FusedTables ts{};
    mfcc_spec::bind_tables(sp.data(), 512.0, ts, pair);
    if (tm.preemph != pair || ts.preemph != pair) return "bound pair";
    checked += 3;

    // num + den = 128 is beyond the biased dot product: refused
    std::vector<char> none;
    if (mfcc_fused::build_tables<true>(16000, 512.0, 0.0, 13, 32, w512, 63, 65, none)) return "63/65 accepted by the four-wave builder";
    if (mfcc_fused::build_tables<true>(16000, 512.0, 0.0, 13, 32, w512, 0, 128, none)) return "0/128 accepted by the four-wave builder";
    if (mfcc_fused160mb::build_tables(md, 40, 13, w, 128, 512.0, 0.0, none, mask)) return "den 128 accepted by the bank builder";
    if (!mfcc_fused::build_tables<true>(16000, 512.0, 0.0, 13, 32, w512, 63, 64, none)) return "63/64 refused";
    return nullptr;
}

// A line with seven fields, "window symmetric num den frame_len rate n_mel": the dense four-wave tables at that sample
// rate and filter count (32 or 16) under the front.  Checks
//   win_dc   [16 n2][32 n1] == w[16 n1 + n2] / den in double, behind set_window when frame_len < 512
//   every mel operand -- the fp32 and bf16 set lists, with and without bin 0, bin 0's weights, the column-16 rows and the
//   DCT rows -- is the default front's byte for byte: the bank does not depend on the front
// and prints "ok <needs_dc_exact> <entries checked>".
static const char *check_rate(int window, int symmetric, int num, int den, int L, int rate, int n_mel, long &checked) {
    using namespace mfcc_tables;
    Front f;
    f.window = window, f.symmetric = symmetric, f.num = num, f.den = den;
    std::vector<double> w = front_window(f, L);
    w.resize(mfcc_fused::kNfft, 0.0);
    const std::vector<double> w512 = front_window(f, mfcc_fused::kNfft);
    const int n_cep = n_mel < 13 ? n_mel : 13;
    std::vector<char> blob, plain;
    if (!mfcc_fused::build_tables<true>(rate, 512.0, 0.0, n_cep, n_mel, w512, num, den, blob)) return "dense builder refused";
    if (!mfcc_fused::build_tables<true>(rate, 512.0, 0.0, n_cep, n_mel, plain)) return "dense builder refused the default front";
    if (L < mfcc_fused::kNfft) mfcc_fused160::set_window(blob, true, w, den);
    const mfcc_fused::BlobOffsets o = mfcc_fused::blob_offsets(true);
    if (blob.size() != o.total || plain.size() != o.total) return "blob size";
    const double *wdc = reinterpret_cast<const double *>(blob.data() + o.win_dc);
    for (int n2 = 0; n2 < 16; ++n2)
        for (int n1 = 0; n1 < 32; ++n1, ++checked)
            if (wdc[n2 * 32 + n1] != w[16 * n1 + n2] / double(den)) return "win_dc row";
    const size_t same[][2] = {{o.tw, o.win_dc}, {o.a_mel_bf_nodc, o.a_dc_i8}, {o.a_dct_bf, o.total}};
    for (const auto &r : same) {
        if (memcmp(blob.data() + r[0], plain.data() + r[0], r[1] - r[0]) != 0) return "a mel operand differs from the default front's";
        checked += long(r[1] - r[0]) / 4;
    }
    return nullptr;
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int window, symmetric, num, den, L, rate, n_mel;
        const int fields = sscanf(line, "%d %d %d %d %d %d %d", &window, &symmetric, &num, &den, &L, &rate, &n_mel);
        if (fields == 7) {
            long checked = 0;
            const char *bad = check_rate(window, symmetric, num, den, L, rate, n_mel, checked);
            if (bad) printf("FAIL %s\n", bad);
            else printf("ok %d %ld\n", int(mfcc_fused::needs_dc_exact(rate, n_mel)), checked);
            continue;
        }
        if (fields != 5) continue;
        long checked = 0;
        const char *bad = check_case(window, symmetric, num, den, L, checked);
        if (bad) printf("FAIL %s\n", bad);
        else printf("ok %ld\n", checked);
    }
    return 0;
}
