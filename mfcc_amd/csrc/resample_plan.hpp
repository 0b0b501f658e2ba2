// Sample-rate conversion (include/mfcc_hip.h: "sample rates"): everything the host decides, with
// no HIP in it -- the geometry of a ratio, the Q14 tap table, the output counts of the one-shot and the streaming
// form, the tile geometry of the kernel (kernel_resample.hpp) and the tile list and scratch layout of a call with
// several segments.  tests/resample_plan_driver.cpp prints all of it for tests/test_resample_host.py.
//
// The functions the kernel needs too are constexpr: hipcc compiles those for both sides, so the host and the device
// run the same lines.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mfcc_rs {

constexpr int kZero = 16;                      // zero crossings on each side, at the lower of the two rates
constexpr double kBeta = 7.5, kRolloff = 0.90;
constexpr int kOne = 16384, kShift = 14;       // Q14
constexpr int kMaxRatio = 1024;                // L and M
constexpr size_t kMaxTableBytes = 65536;
constexpr int kThreads = 256, kGroup = 8, kTile = kThreads * kGroup;          // outputs of a workgroup's tile
constexpr int kMaxSpan = 16384;                // staged input samples of a tile (32 KiB of LDS); above: the unstaged kernel
constexpr int kBlocksPerCu = 8;

struct Geometry {
    int L = 0, M = 0, H = 0, K = 0;
};

constexpr long long gcd_ll(long long a, long long b) {
    while (b) {
        const long long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// 0: fine; 1: a rate is not positive; 2: L, M or the table is over the limit
inline int geometry(long long in_rate, long long out_rate, Geometry &g) {
    if (in_rate <= 0 || out_rate <= 0) return 1;
    const long long d = gcd_ll(in_rate, out_rate), L = out_rate / d, M = in_rate / d;
    if (L > kMaxRatio || M > kMaxRatio) return 2;
    // H = ceil(Z / s), s = min(1, L / M): in integers
    const long long H = L >= M ? kZero : (kZero * M + L - 1) / L;
    if (size_t(L) * size_t(2 * H) * sizeof(int16_t) > kMaxTableBytes) return 2;
    g.L = int(L);
    g.M = int(M);
    g.H = int(H);
    g.K = int(2 * H);
    return 0;
}

// ---- the output rule's integers
// outputs of n input samples: ceil(n L / M)
constexpr unsigned long long count(unsigned long long n, int L, int M) {
    return (n * (unsigned long long)L + (unsigned long long)M - 1) / (unsigned long long)M;
}
// outputs a line has emitted after c input samples: it holds back the last H
constexpr unsigned long long emitted(unsigned long long c, int L, int M, int H) {
    return count(c > (unsigned long long)H ? c - (unsigned long long)H : 0, L, M);
}
// output m reads the K samples from q - H + 1 on with the taps of phase p
constexpr long long phase_q(long long m, int L, int M) { return m * M / L; }
constexpr int phase_p(long long m, int L, int M) { return int(m * M % L); }
// y = sat16((acc + 8192) >> 14), arithmetic shift
constexpr int finish(int acc) {
    const int v = (acc + (kOne >> 1)) >> kShift;
    return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
}
// n L does not overflow 64 bits, and n_out fits the kernel's 63-bit indices
constexpr size_t kMaxLen = size_t(1) << 40;

// ---- the table
inline double bessel_i0(double x) {
    const double y = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < 500; ++k) {
        term *= y / (double(k) * double(k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

inline double design(double d, double fc, int H) {
    const double r = d / H;
    if (r < -1 || r > 1) return 0;
    const double a = M_PI * fc * d, sinc = a == 0 ? 1 : sin(a) / a;
    const double w = 1 - r * r;
    return fc * sinc * bessel_i0(kBeta * sqrt(w > 0 ? w : 0)) / bessel_i0(kBeta);
}

// T[p][k], L rows of K taps.  false: a phase's sum of magnitudes is over 65535 (a 32-bit sum could wrap)
inline bool build_taps(const Geometry &g, std::vector<int16_t> &t) {
    const double s = g.L >= g.M ? 1.0 : double(g.L) / g.M, fc = kRolloff * s;
    t.assign(size_t(g.L) * g.K, 0);
    std::vector<double> row(g.K);
    for (int p = 0; p < g.L; ++p) {
        double sum = 0;
        for (int k = 0; k < g.K; ++k) sum += row[k] = design(k - g.H + 1 - double(p) / g.L, fc, g.H);
        int16_t *tp = t.data() + size_t(p) * g.K;
        long total = 0, mag = 0;
        int big = 0;
        for (int k = 0; k < g.K; ++k) {
            const long v = long(rint(kOne * (row[k] / sum)));
            tp[k] = int16_t(v);
            total += v;
            if (v > tp[big]) big = k;          // the first of the largest taps takes the residual
        }
        tp[big] = int16_t(tp[big] + (kOne - total));
        for (int k = 0; k < g.K; ++k) mag += tp[k] < 0 ? -long(tp[k]) : long(tp[k]);
        if (mag > 65535) return false;
    }
    return true;
}

// the rule on the host: outputs [m0, m1) of the n samples at x, zeros outside [0, n)
inline void resample_host(const Geometry &g, const int16_t *taps, const int16_t *x, long long n, long long m0, long long m1,
                          int16_t *y) {
    for (long long m = m0; m < m1; ++m) {
        const long long q = phase_q(m, g.L, g.M), first = q - g.H + 1;
        const int16_t *tp = taps + size_t(phase_p(m, g.L, g.M)) * g.K;
        int k0 = first < 0 ? int(-first) : 0, k1 = first + g.K > n ? int(n - first) : g.K, acc = 0;
        for (int k = k0; k < k1; ++k) acc += int(tp[k]) * int(x[first + k]);
        y[m - m0] = int16_t(finish(acc));
    }
}

// ---- the kernel's tile geometry
// a tile is kTile consecutive 16-byte-aligned output slots: slot v of a segment is output v - lead, where lead < 8 is
// the segment's output pointer in int16 modulo 8.  Slots in front of output 0 and behind the last are empty
constexpr int lead_of(uintptr_t out) { return int((out >> 1) & 7); }
constexpr long long tiles_of(long long n_out, int lead) { return n_out > 0 ? (n_out + lead + kTile - 1) / kTile : 0; }
// the staged samples of a tile, at most: its outputs' reach, up to 7 samples of alignment in front, one pair behind
// (the odd-start pairs read one word further), rounded up to a group of 8
constexpr long long span_cap(int L, int M, int K) {
    return ((((long long)(kTile - 1) * M + L - 1) / L + K + 7 + 2) + 7) & ~7ll;
}
constexpr bool staged(int L, int M, int K) { return span_cap(L, M, K) <= kMaxSpan; }
// The table lies in LDS too, in front of the samples (rounded up to 8 taps), where both fit kLdsBudget: measured against
// reading it from global memory, 1.06 to 5.5 times the rate
constexpr size_t kLdsBudget = 63 * 1024;
constexpr int taps_lds_samples(int L, int K) { return (L * K + 7) & ~7; }
constexpr bool taps_in_lds(int L, int M, int K) {
    return staged(L, M, K) && (size_t(span_cap(L, M, K)) + size_t(taps_lds_samples(L, K))) * sizeof(int16_t) <= kLdsBudget;
}
constexpr size_t lds_bytes(int L, int M, int K) {
    return staged(L, M, K) ? (size_t(span_cap(L, M, K)) + (taps_in_lds(L, M, K) ? taps_lds_samples(L, K) : 0)) * sizeof(int16_t) : 0;
}

// the samples [lo, hi) a tile's outputs [ma, mb) read, before clipping to [0, n)
constexpr long long reach_lo(long long ma, int L, int M, int H) { return phase_q(ma, L, M) - H + 1; }
constexpr long long reach_hi(long long mb, int L, int M, int H) { return phase_q(mb - 1, L, M) + H + 1; }

// A segment is what one launch converts for one row, utterance or line: the chunk of n samples at `in`, whose first
// sample is sample c0 of the line, K - 1 samples of history in front of it (hist; none: zeros) and zeros behind it; the
// outputs [m0, m1) of the line, stored from `out` on.  One-shot: c0 = 0, m0 = 0, m1 = count(n), no history.
//
// What the kernel does with tile t of a segment: its outputs [ma, mb), counted from m0 (empty: nothing), and, staged, LDS
// sample i is sample base + i of the CHUNK (negative: history) for i < 8 groups, where in + base is 16-byte aligned.
// The same lines on the device
struct TileSpan {
    long long ma, mb, base;
    int groups;
};
constexpr TileSpan tile_span(long long t, int lead, long long m0, long long m1, long long c0, uintptr_t in, int L, int M, int H) {
    const long long m_slot0 = t * kTile - lead, n_out = m1 - m0;       // the output of the tile's first slot
    const long long ma = m_slot0 > 0 ? m_slot0 : 0, mb = m_slot0 + kTile < n_out ? m_slot0 + kTile : n_out;
    if (ma >= mb) return TileSpan{ma, mb, 0, 0};
    const long long lo = reach_lo(m0 + ma, L, M, H) - c0, hi = reach_hi(m0 + mb, L, M, H) + 1 - c0;
    const long long base = lo - (((long long)(in >> 1) + lo) & 7);
    return TileSpan{ma, mb, base, int((hi - base + 7) >> 3)};
}

// ---- a call with several segments (ragged utterances, the lines of a push): one launch over a tile list
// a segment's record, kSegLL long longs: in, n, out, m0, m1, c0, hist, hist_new (addresses; 0: none).  A segment with
// hist_new has one more tile, t = -1 in the list, that writes the K - 1 samples in front of sample c0 + n there
constexpr int kSegLL = 8, kTileLL = 2;         // a tile's record: segment, tile of the segment
constexpr long long kHistoryTile = -1;
struct SegIn {
    uintptr_t in = 0, out = 0;
    unsigned long long n = 0, m0 = 0, m1 = 0, c0 = 0;
    uintptr_t hist = 0, hist_new = 0;
};
inline SegIn one_shot(const Geometry &g, uintptr_t in, unsigned long long n, uintptr_t out) {
    SegIn s;
    s.in = in;
    s.out = out;
    s.n = n;
    s.m1 = count(n, g.L, g.M);
    return s;
}
struct CallPlan {
    size_t n_tiles = 0, seg_ll = 0, tile_off_ll = 0, total_ll = 0, bytes = 0;
};
struct Limits {
    size_t len = kMaxLen, tiles = size_t(1) << 30;
};
// the tiles of a segment, at most, wherever its output lies
constexpr size_t max_tiles(unsigned long long n_out, bool history) { return size_t(tiles_of((long long)n_out, 7)) + (history ? 1 : 0); }
// false: a length or the tile count is over the limits
inline bool plan_call(const SegIn *segs, size_t n_seg, CallPlan &pl, const Limits &lim = Limits{}) {
    pl = CallPlan{};
    for (size_t s = 0; s < n_seg; ++s) {
        if (segs[s].n >= lim.len || segs[s].m1 < segs[s].m0 || segs[s].m1 - segs[s].m0 >= lim.len * kMaxRatio) return false;
        pl.n_tiles += size_t(tiles_of((long long)(segs[s].m1 - segs[s].m0), lead_of(segs[s].out))) + (segs[s].hist_new ? 1 : 0);
        if (pl.n_tiles >= lim.tiles) return false;
    }
    pl.seg_ll = n_seg * kSegLL;
    pl.tile_off_ll = pl.seg_ll;
    pl.total_ll = pl.tile_off_ll + pl.n_tiles * kTileLL;
    pl.bytes = pl.total_ll * sizeof(long long) + 64;
    return true;
}
// the records, total_ll long longs at d
inline void fill_call(const SegIn *segs, size_t n_seg, const CallPlan &pl, long long *d) {
    long long *t = d + pl.tile_off_ll;
    for (size_t s = 0; s < n_seg; ++s) {
        const SegIn &g = segs[s];
        const long long v[kSegLL] = {(long long)g.in, (long long)g.n,  (long long)g.out,  (long long)g.m0,
                                     (long long)g.m1, (long long)g.c0, (long long)g.hist, (long long)g.hist_new};
        for (int i = 0; i < kSegLL; ++i) d[s * kSegLL + i] = v[i];
        if (g.hist_new) {
            *t++ = (long long)s;
            *t++ = kHistoryTile;
        }
        for (long long i = 0, nt = tiles_of((long long)(g.m1 - g.m0), lead_of(g.out)); i < nt; ++i) {
            *t++ = (long long)s;
            *t++ = i;
        }
    }
}

// the grid of a launch over `tiles` tiles (x) of `rows` rows (y)
inline void grid(long long tiles, long long rows, int n_cu, unsigned &gx, unsigned &gy) {
    long long y = rows < 65535 ? rows : 65535;
    if (y < 1) y = 1;
    long long cap = (long long)n_cu * kBlocksPerCu / y;
    if (cap < 1) cap = 1;
    long long x = tiles < cap ? tiles : cap;
    if (x < 1) x = 1;
    gx = unsigned(x);
    gy = unsigned(y);
}

}  // namespace mfcc_rs
