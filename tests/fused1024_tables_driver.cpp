// Prints the size and a hash of the table blobs of the fused 1024 kernels for every case on stdin
// (tests/test_fused1024_tables_host.py).  Host code only: nothing here touches a device.  A case is one line:
//   bf  sample_rate n_cep lifter power_scale     mfcc_fused1024::build_tables      (bf16-split set lists)
//   f32 sample_rate n_cep lifter power_scale     mfcc_fused1024_f32::build_tables  (one fp32 list per rate)
// and its answer one line:
//   ok variant-or-schedule bytes fnv1a64         (refused: 0 -1 0 and the hash of nothing)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kernel_fused1024_w12.hpp"

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
        int rate, n_cep, which = -1;
        double lifter, power_scale;
        if (scanf("%d %d %lf %lf", &rate, &n_cep, &lifter, &power_scale) != 4) return 2;
        bool ok;
        if (!strcmp(kind, "bf")) ok = mfcc_fused1024::build_tables(rate, power_scale, lifter, n_cep, blob, which);
        else if (!strcmp(kind, "f32")) ok = mfcc_fused1024_f32::build_tables(rate, power_scale, lifter, n_cep, blob, which);
        else return 2;
        if (!ok) {
            blob.clear();
            which = -1;
        }
        printf("%d %d %zu %016llx\n", int(ok), which, blob.size(), fnv1a64(blob));
    }
    return 0;
}
