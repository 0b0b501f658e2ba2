// Centred framing (include/mfcc_hip.h: "centring") on the host: the geometry, the rule itself, the
// stride of a dense call's padded rows and the table of a ragged call.  No HIP in here: tests/center_plan_driver.cpp
// compiles it with a plain host compiler, kernel_center.hpp reads the same records on the device.
//
// The rule.  L: the frame length, hop: the hop, n: the samples of one channel or utterance at the handle's own rate.
//     PL    = nfft / 2 - (nfft - L) / 2                      (integer divisions; = ceil(L / 2))
//     F(n)  = 0 if n <= PL (reflect) or n == 0 (zeros), else 1 + n / hop
//     N'(n) = (F - 1) * hop + L                              (0 when F = 0)
//     p[i], 0 <= i < N':  j = i - PL;  reflect: j < 0 -> -j, j >= n -> 2 (n - 1) - j;  zeros: 0 outside [0, n);  else x[j]
// With n > PL one reflection suffices on both sides: the left reach is PL <= n - 1, the right reach N' - PL - n is at most
// L - PL = floor(L / 2) <= n - 1.  Left pad, frame count and edge rule are values of Geom, not constants of the code, so
// that another convention (Kaldi's snip_edges=false) can follow as another Geom.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mfcc_center {

enum Edge { kOff = 0, kReflect = 1, kZeros = 2 };       // the values of enum mfcc_hip_center

constexpr bool known(int mode) { return mode >= kOff && mode <= kZeros; }

struct Geom {
    long long left;       // PL
    long long L, hop;
    int edge;             // kReflect or kZeros
};

inline Geom geometry(int nfft, int frame_len, int hop, int mode) {
    return Geom{(long long)(nfft / 2 - (nfft - frame_len) / 2), (long long)frame_len, (long long)hop, mode};
}

// F(n)
inline size_t frames(const Geom &g, size_t n) {
    if (g.edge == kReflect ? n <= size_t(g.left) : n == 0) return 0;
    return 1 + n / size_t(g.hop);
}

// N'(n)
inline size_t padded(const Geom &g, size_t n) {
    const size_t f = frames(g, n);
    return f ? (f - 1) * size_t(g.hop) + size_t(g.L) : 0;
}

// the source of p[i] in x[0, n): its index, or -1 for a zero.  frames(g, n) > 0
inline long long source(const Geom &g, long long i, long long n) {
    long long j = i - g.left;
    if (j >= 0 && j < n) return j;
    if (g.edge == kZeros) return -1;
    j = j < 0 ? -j : 2 * (n - 1) - j;
    return j >= 0 && j < n ? j : -1;                    // cannot happen with n > PL; never an index outside the row
}

// the rule on int16: out holds padded(g, n) samples
inline void center_host(const Geom &g, const int16_t *in, size_t n, int16_t *out) {
    const long long np = (long long)padded(g, n);
    for (long long i = 0; i < np; ++i) {
        const long long j = source(g, i, (long long)n);
        out[i] = j < 0 ? int16_t(0) : in[j];
    }
}

// the stride of `rows` padded rows of np samples: a multiple of 8, so that every row has the same alignment
inline size_t dense_stride(size_t np, size_t rows) { return rows <= 1 ? np : (np + 7) & ~size_t(7); }

// ---- the ragged table: one record per utterance, as the kernel reads it
constexpr size_t kRecLL = 4;       // source offset, n, destination offset, N' (samples)

struct Table {
    size_t total;         // sum of N': the samples of the padded corpus
    size_t n_live;        // utterances with F > 0
    size_t max_padded;    // the longest padded utterance
};

// The utterances own[u] .. own[u + 1] of one buffer (sample offsets, non-decreasing; own[0] is where the first one lies)
// -> own2[0 .. n_utt]: the padded utterances abut from 0, own2[u + 1] = own2[u] + N'_u; an utterance with F = 0 takes no
// room.  recs (n_utt * kRecLL entries, or NULL): source offsets from `base` (the offset the kernel's source pointer stands
// at), destination offsets as in own2
inline Table fill_table(const Geom &g, const size_t *own, size_t n_utt, size_t base, size_t *own2, long long *recs) {
    Table t{0, 0, 0};
    own2[0] = 0;
    for (size_t u = 0; u < n_utt; ++u) {
        const size_t n = own[u + 1] - own[u], np = padded(g, n);
        if (recs) {
            recs[kRecLL * u] = (long long)(own[u] - base);
            recs[kRecLL * u + 1] = (long long)n;
            recs[kRecLL * u + 2] = (long long)own2[u];
            recs[kRecLL * u + 3] = (long long)np;
        }
        own2[u + 1] = own2[u] + np;
        t.n_live += np != 0;
        if (np > t.max_padded) t.max_padded = np;
    }
    t.total = own2[n_utt];
    return t;
}

}  // namespace mfcc_center
