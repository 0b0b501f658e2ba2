// Sliding-window mean / variance normalization of float rows already in HBM (include/mfcc_hip.h:
// mfcc_hip_normalize_sliding_dev).  A pass after the MFCC kernels, not a change to them; out of
// place, because the window of a row reaches into rows another workgroup has already written.
//
// in, out: float32 rows [R][W], W = 1..64, at the same row indices; a segment is a range of whole rows (one channel of
// a dense call, one utterance of a ragged one).  Row t of a segment of T rows is standardized with the statistics of
// rows [a, b) of the SAME segment (window_of below: Kaldi's SlidingWindowCmn rule), per column over the finite values:
// mu = mean, sigma = population std in float64, sigma' = 1 where sigma < 10 * 2^-52; y = (x - fl32(mu)) * fl32(1 /
// sigma') for finite x, x unchanged otherwise.
//
// The tiles are those of kernel_normalize.hpp (Segs / tile_of / BlockRec, counted from the segment's own first row);
// a tile is G = 256 / W runs of S consecutive rows (run_rows below: a function of the window alone).  One thread per
// (run, column): it streams the window of the run's first row into three float64 running sums of the finite values --
// n, sum(x - p), sum((x - p)^2), the pivot p = the first finite value it meets in that window -- and then slides: for
// every further row of the run, add the rows that entered [a, b), drop the ones that left, in row order.  The sums
// are window-local: they start over with every run, and whenever the window holds no finite value (which also chooses
// a new p) or has become small against what passed through it (kStale below: what large values leave behind in q when
// they are dropped would otherwise stay), so the q / n - m^2 cancellation is bounded by the spread inside the window
// and not by the segment's.  Nothing is parked in LDS: the halo is consumed as a stream, N is free up to
// MFCC_HIP_MAX_NORMALIZE_WINDOW.  The W lanes of a run read and write one contiguous row per step with scalar loads
// and stores (a lane's rows lie W floats apart, so there is no float4 body); the rows a run reads beyond its own are
// the neighbouring runs' and are expected in L2 (DESIGN.md section 4.8 says what was measured).  Every order of
// summation is a function of W, N, M, center and the segment's rows alone: a segment gives the same bits wherever it
// lies, at any alignment, in whatever call.  No atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_normalize.hpp"

namespace mfcc_slide {

constexpr int kThreads = 256;
constexpr int kMaxWidth = mfcc_norm::kMaxWidth;
constexpr int kMaxWindow = 16384;      // MFCC_HIP_MAX_NORMALIZE_WINDOW

// rows per run.  The first row of a run costs its whole window (about N additions), every further one an addition
// and a subtraction: N / S + 2 updates per element.  N / 4 rows per run make that 6 and leave 4 R W / N threads for
// the chip (at N = 600: one run per 150 rows); never fewer than 32 rows (a short window is cheap either way and a
// tile should not be tiny), never more than 256 (a tile of G runs stays a few thousand rows at any N; long windows
// then pay N / 256 + 2 updates per element: they need only be correct)
__host__ __device__ inline int run_rows(int window) {
    const int s = window / 4;
    return s < 32 ? 32 : (s > 256 ? 256 : s);
}

// rows per tile: G runs
__host__ __device__ inline int tile_rows(int width, int window) { return (kThreads / width) * run_rows(window); }

// rows [a, b) whose statistics standardize row t of a segment of T rows; a <= t < b, both non-decreasing in t
__host__ __device__ inline void window_of(long long t, long long T, int N, int M, int center, long long &a,
                                          long long &b) {
    if (center) {
        a = t - N / 2;
        b = a + N;
    } else {
        a = t - N;
        b = t + 1;
    }
    if (a < 0) {
        b -= a;
        a = 0;
    }
    if (!center && b > t) b = t + 1 > M ? t + 1 : M;
    if (b > T) {
        a -= b - T;
        b = T;
        if (a < 0) a = 0;
    }
}

// the running sums of one (run, column)
struct Sums {
    double s, q, p;
    double d2max;                      // the largest (x - p)^2 added since the sums were last started
    int n;
    bool have_p;
};

__device__ __forceinline__ void add(Sums &u, float v) {
    if (!mfcc_norm::finite(v)) return;
    if (!u.have_p) {
        u.p = double(v);
        u.have_p = true;
    }
    const double d = double(v) - u.p, d2 = d * d;
    u.s += d;
    u.q += d2;
    u.d2max = d2 > u.d2max ? d2 : u.d2max;
    u.n += 1;
}

__device__ __forceinline__ void drop(Sums &u, float v) {
    if (!mfcc_norm::finite(v)) return;
    const double d = double(v) - u.p;
    u.s -= d;
    u.q -= d * d;
    if (--u.n == 0) {                  // an empty window starts over: no residue, a new pivot
        u.s = u.q = u.d2max = 0.0;
        u.have_p = false;
    }
}

// Every addition and subtraction leaves up to 2^-53 d2max in q, so about 2^-43 d2max after the 2^10 updates of a run,
// and the window's sum of squared deviations n var is q - s^2 / n to that absolute error.  It is good to 2^-25 (a
// quarter of what the fp32 result resolves) while n var >= 2^-18 d2max.  Below that -- large values have left the
// window and small ones stayed, e.g. a step down from 1e4 to 1e-3 noise -- the sums are started over on the rows of
// the current window.  Then p is one of the window's values, so n var >= d2max / 2: one restart is enough
constexpr double kStale = 1.0 / 262144.0;      // 2^-18

// mode: 1 = mean only (r = 1), 2 = mean and variance
__global__ __launch_bounds__(kThreads) void normalize_sliding_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                                     mfcc_norm::Segs s, int S, int N, int M, int center,
                                                                     int mode) {
    const int W = s.width, G = kThreads / W, t = threadIdx.x, g = t / W, c = t - g * W;
    if (g >= G) return;
    for (long long b = blockIdx.x; b < s.n_blocks; b += gridDim.x) {
        long long row0, seg, lo, hi;
        int rows;
        mfcc_norm::tile_of(s, b, row0, rows, seg);
        if (!s.blk) {
            lo = s.base_row + seg * s.seg_rows;
            hi = lo + s.seg_rows;
        } else {
            const mfcc_norm::BlockRec f = s.blk[s.seg_blk0[seg]], l = s.blk[s.seg_blk0[seg + 1] - 1];
            lo = f.row0;
            hi = l.row0 + l.rows;
        }
        const long long T = hi - lo;
        const long long t0 = row0 - lo + (long long)g * S;              // rows of the segment this run owns
        const long long te = row0 - lo + rows, t1 = t0 + S < te ? t0 + S : te;
        if (t0 >= t1) continue;
        const float *xs = x + lo * W + c;                               // column c of the segment
        Sums u{0.0, 0.0, 0.0, 0.0, 0, false};
        long long ca, cb, wa, wb;
        window_of(t0, T, N, M, center, wa, wb);
        ca = cb = wa;
        const float *pa = xs + ca * W, *pb = pa, *px = xs + t0 * W;     // next row to drop, to add, to normalize
        float *py = y + (lo + t0) * W + c;
        // the first window, four loads in flight; the order of the additions is the rows'
        for (; cb + 4 <= wb; cb += 4, pb += 4 * W) {
            const float v0 = pb[0], v1 = pb[W], v2 = pb[2 * W], v3 = pb[3 * W];
            add(u, v0);
            add(u, v1);
            add(u, v2);
            add(u, v3);
        }
        int n_inv = 0;
        double inv = 0.0;
        for (long long r = t0; r < t1; ++r, px += W, py += W) {
            window_of(r, T, N, M, center, wa, wb);
            const float v = *px;
            for (; cb < wb; ++cb, pb += W) add(u, *pb);
            for (; ca < wa; ++ca, pa += W) drop(u, *pa);
            float out = v;
            if (mfcc_norm::finite(v) && u.n > 0) {
                if (u.n != n_inv) {                                     // n rarely changes from row to row
                    n_inv = u.n;
                    inv = 1.0 / double(u.n);
                }
                double m = u.s * inv, var = u.q * inv - m * m;
                if (var < kStale * u.d2max * inv) {                     // stale sums (see kStale): start over
                    u = Sums{0.0, 0.0, 0.0, 0.0, 0, false};
                    const float *pr = pa;
                    for (long long i = ca; i < cb; ++i, pr += W) add(u, *pr);
                    m = u.s * inv;                                      // n is what it was
                    var = u.q * inv - m * m;
                }
                float r32 = 1.0f;
                if (mode == 2) {
                    double sd = var > 0.0 ? sqrt(var) : 0.0;
                    if (sd < 10.0 * 2.220446049250313e-16) sd = 1.0;
                    r32 = float(1.0 / sd);
                }
                out = (v - float(u.p + m)) * r32;
            }
            *py = out;
        }
    }
}

}  // namespace mfcc_slide
