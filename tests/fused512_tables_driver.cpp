// Prints the size and a hash of the table blobs of the four-wave fused 512 kernels for every case on stdin
// (tests/test_fused512_tables_host.py).  Host code only: nothing here touches a device.  A case is one line:
//   nb dense sample_rate n_mel n_cep frame_len lifter     mfcc_fused::build_tables<dense>, then -- frame_len > 0 --
//                                                        mfcc_fused160::set_window
//   mb sample_rate n_mel n_cep frame_len low high lifter  mfcc_fused160mb::build_tables on the HTK matrix (high 0: rate / 2)
// and its answer one line:
//   nb: ok needs_dc_exact bytes fnv1a64        mb: ok bytes fnv1a64 set_mask
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kernel_fused512_h160_mb.hpp"

static unsigned long long fnv1a64(const std::vector<char> &b) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (char c : b) {
        h ^= (unsigned char)c;
        h *= 0x100000001b3ull;
    }
    return h;
}

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        std::vector<char> blob;
        if (!strcmp(kind, "nb")) {
            int dense, rate, n_mel, n_cep, frame_len;
            double lifter;
            if (scanf("%d %d %d %d %d %lf", &dense, &rate, &n_mel, &n_cep, &frame_len, &lifter) != 6) return 2;
            const bool ok = dense ? mfcc_fused::build_tables<true>(rate, 512.0, lifter, n_cep, n_mel, blob)
                                  : mfcc_fused::build_tables<false>(rate, 512.0, lifter, n_cep, n_mel, blob);
            if (ok && frame_len > 0) mfcc_fused160::set_window(blob, dense != 0, frame_len);
            if (!ok) blob.clear();
            printf("%d %d %zu %016llx\n", int(ok), int(mfcc_fused::needs_dc_exact(rate, n_mel)), blob.size(), fnv1a64(blob));
        } else if (!strcmp(kind, "mb")) {
            int rate, n_mel, n_cep, frame_len;
            double low, high, lifter;
            if (scanf("%d %d %d %d %lf %lf %lf", &rate, &n_mel, &n_cep, &frame_len, &low, &high, &lifter) != 7) return 2;
            const std::vector<double> md = mfcc_tables::mel_dense_htk(512, n_mel, double(rate), low, high == 0.0 ? rate / 2.0 : high);
            uint32_t mask = 0;
            const bool ok = mfcc_fused160mb::build_tables(md, n_mel, n_cep, frame_len, 512.0, lifter, blob, mask);
            if (!ok) blob.clear();
            printf("%d %zu %016llx %u\n", int(ok), blob.size(), fnv1a64(blob), ok ? mask : 0u);
        } else {
            return 2;
        }
    }
    return 0;
}
