// Prints what mfcc_amd/csrc/bank_plan.hpp makes of every case on stdin (tests/test_bank_plan_host.py).  A case is one
// line of numbers behind its kind:
//   push flen hop W elem S L order g norm pcen n  have_samples have_out cap shift  pending[n] seen[n] held[n] offsets[n + 1]
//   end  flen hop W elem S L order g norm pcen n  emit give have_out cap k         pending[n] seen[n] held[n] list[k]
// and its answer one line: rc, frame_offsets (n + 1, resp. k + 1; 12345 where the plan did not get to), then after
// MFCC_HIP_SUCCESS: (push only) pending_after[n] held_after[n] raw_offsets[n + 1]; the Layout -- (off, n) of the tables
// bank gather cmvn delta carry pcen, desc_ll n_rec n_active nfmax stride lockstep direct in_bytes out_bytes raw_off
// stat_off --; and the desc_ll long longs of the descriptor block, which starts out as -7777 everywhere.
// The block is allocated at exactly desc_ll long longs: under -fsanitize=address a record past its end is an error.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bank_plan.hpp"

static bool read_n(std::vector<size_t> &v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%zu", &v[i]) != 1) return false;
    return true;
}

static void print_n(const std::vector<size_t> &v) {
    for (size_t x : v) printf(" %zu", x);
}

int main() {
    using namespace mfcc_bank;
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        const bool push = !strcmp(kind, "push");
        Settings s{};
        int norm, pcen, f0, f1, f2 = 0;
        size_t n, cap, x;
        if (scanf("%zu %zu %zu %zu %zu %zu %d %zu %d %d %zu %d %d", &s.flen, &s.hop, &s.W, &s.elem, &s.S, &s.L, &s.order, &s.g,
                  &norm, &pcen, &n, &f0, &f1) != 13 ||
            (!push && scanf("%d", &f2) != 1) || scanf("%zu %zu", &cap, &x) != 2)
            return 2;
        s.norm = norm != 0;
        s.pcen = pcen != 0;
        std::vector<size_t> pending, seen, held, arg;
        if (!read_n(pending, n) || !read_n(seen, n) || !read_n(held, n) || !read_n(arg, push ? n + 1 : x)) return 2;
        const State st{pending.data(), seen.data(), held.data()};
        std::vector<size_t> fo(arg.size() + (push ? 0 : 1), 12345), pa(n, 12345), ha(n, 12345), rfo(n + 1, 12345);
        Layout l;
        const int rc = push ? push_plan(s, st, arg.data(), n, f0 != 0, f1 != 0, cap, fo.data(), pa.data(), ha.data(), rfo.data(), l)
                            : end_plan(s, st, arg.data(), arg.size(), f0 != 0, f1 != 0, f2 != 0, cap, fo.data(), l);
        printf("%d", rc);
        print_n(fo);
        if (rc == MFCC_HIP_SUCCESS) {
            if (push) {
                print_n(pa);
                print_n(ha);
                print_n(rfo);
            }
            for (const Table &t : {l.bank, l.gather, l.cmvn, l.delta, l.carry, l.pcen}) printf(" %zu %zu", t.off, t.n);
            printf(" %zu %zu %zu %zu %zu %d %d %zu %zu %zu %zu", l.desc_ll, l.n_rec, l.n_active, l.nfmax, l.stride, int(l.lockstep),
                   int(l.direct), l.in_bytes, l.out_bytes, l.raw_off, l.stat_off);
            if (l.n_rec) {
                long long *block = new long long[l.desc_ll];
                for (size_t i = 0; i < l.desc_ll; ++i) block[i] = -7777;
                if (push)
                    push_fill(s, st, arg.data(), x, n, fo.data(), rfo.data(), l, block);
                else
                    end_fill(s, st, arg.data(), fo.data(), l, block);
                for (size_t i = 0; i < l.desc_ll; ++i) printf(" %lld", block[i]);
                delete[] block;
            }
        }
        printf("\n");
    }
    return 0;
}
