// The host side of a stream bank's push, flush and reset: everything they decide from lengths and settings -- the plan
// per stream, the records the kernels read, where each record table lies in the descriptor block, and how much scratch
// the operation needs ("The descriptor block").  No HIP in here: the host tests compile this
// header on its own (tests/test_bank_plan_host.py).  The record structs are the kernels' (kernel_stream_bank.hpp,
// kernel_stream_bank_online.hpp, kernel_pcen.hpp include this header for them).
#pragma once

#include <stddef.h>

#include "../../include/mfcc_hip.h"

namespace mfcc_bank {

// one stream of a push / flush / reset; `src` is the offset of its chunk in the samples buffer
struct Rec {
    long long stream, src, n_new, pending, nf;
};
constexpr int kRecLL = 5;                      // a record as long longs in the pinned descriptor pool
constexpr int kGatherLL = 3;                   // a row of the gather table: first row in, first row out, rows
static_assert(sizeof(Rec) == kRecLL * sizeof(long long), "record layout");

// The plan of one stream: frames a push of n_new samples completes and what stays pending (always < nfft)
inline void plan(size_t pending, size_t n_new, size_t nfft, size_t hop, size_t &nf, size_t &pending_after) {
    const size_t total = pending + n_new;
    nf = total >= nfft ? (total - nfft) / hop + 1 : 0;
    pending_after = total - nf * hop;
}

}  // namespace mfcc_bank

namespace mfcc_online {

constexpr long long kNoEdge = 0x7fffffffffffffffLL;        // `last` of a stream that goes on

// cmvn:   rows [t0, cnt) of `stream` (cnt = t1), row `seen` is written to row out_row of y
// deltas: rows [t0, t0 + cnt) of `stream` are emitted, row t0 to row out_row of y; indices clamp to [0, last]
// carry:  the nf fresh rows of `stream`
struct Rec {
    long long stream, row0, seen, nf, t0, cnt, out_row, last;
};
constexpr int kRecLL = 8;                                  // a record as long longs in the pinned descriptor pool
static_assert(sizeof(Rec) == kRecLL * sizeof(long long), "record layout");

// The delta kernels' tiles (kernel_stream_bank_online.hpp).  A tile of g emitted rows holds (g + 2L) W static floats,
// L = order * window, and at order 2 (g + 2 window) W delta floats as well.  Rows of up to kNarrowWidth floats -- every
// MFCC bank -- have 16 KB of LDS, as kernel_deltas.hpp: g >= 8 for every W <= 64, window <= 8.  The rows of 65 .. 128
// floats of a filterbank bank have 32 KB: g >= 8 for every W <= 128, order <= 2, window <= 8 (exactly 8 at 128 x 2 x 8),
// and five workgroups of a CU's 160 KB still run side by side
constexpr int kLdsFloats = 4096;
constexpr int kWideLdsFloats = 8192;
constexpr int kNarrowWidth = 64;
constexpr int tile_rows_of(int lds_floats, int width, int order, int window) {
    return order == 1 ? lds_floats / width - 2 * order * window
                      : (lds_floats / width - 2 * order * window - 2 * window) / 2;
}
constexpr int tile_rows(int width, int order, int window) { return tile_rows_of(kLdsFloats, width, order, window); }
constexpr int wide_tile_rows(int width, int order, int window) { return tile_rows_of(kWideLdsFloats, width, order, window); }
// ... of a bank whose rows are `width` floats: which kernel runs is decided by the width alone
constexpr bool wide_rows(size_t width) { return width > size_t(kNarrowWidth); }
constexpr int delta_tile_rows(int width, int order, int window) {
    return wide_rows(size_t(width)) ? wide_tile_rows(width, order, window) : tile_rows(width, order, window);
}

// The runs of the causal CMVN that cover the fresh rows [seen, seen + nf) of a stream: S rows each, counted from frame 0
inline size_t online_runs(size_t seen, size_t nf, size_t S) { return nf ? (seen + nf - 1) / S - seen / S + 1 : 0; }

}  // namespace mfcc_online

namespace mfcc_pcen {

// The nf fresh rows of `stream` start at row row0 of `raw`; their PCEN goes to row out_row of `dst` (dst == raw: in place)
struct OnlineRec {
    long long stream, row0, seen, nf, out_row;
};
constexpr int kOnlineRecLL = 5;                            // a record as long longs in the pinned descriptor pool
static_assert(sizeof(OnlineRec) == kOnlineRecLL * sizeof(long long), "record layout");

}  // namespace mfcc_pcen

namespace mfcc_bank {

// what a bank was created with
struct Settings {
    size_t flen, hop, W;                       // frame length and hop in samples, row width of the frame kernels
    size_t elem;                               // bytes of an element of a row: 2 (fixed) or 4
    size_t S, L;                               // online: rows of a CMVN run, lag = order * delta window
    int order;                                 // delta order: rows leave as [static | D | DD], W (1 + order) wide
    size_t g;                                  // emitted rows per tile of the delta kernel
    bool norm, pcen;
    bool online() const { return norm || order || pcen; }
    bool post() const { return norm || order; }            // passes behind PCEN: it then runs in place on the raw rows
    size_t out_width() const { return W * size_t(1 + order); }
};

// the host mirror of the streams: samples of the frame in progress, frames since reset, finished rows not yet returned
struct State {
    const size_t *pending, *seen, *held;
};

// a record table of the descriptor block: its first long long and its number of records
struct Table {
    size_t off, n;
};

// The descriptor block and the scratch of one push, flush or reset.  The block goes to the front of the handle's output
// scratch; the tables lie in it in this order, without gaps (which bank kinds have which: DESIGN.md section 6c-bis)
struct Layout {
    Table bank, gather, cmvn, delta, carry, pcen;
    size_t desc_ll;                            // long longs of the block
    size_t n_rec, n_active;                    // bank records; those of them that get a row of the work buffer (the first)
    size_t nfmax, stride;                      // frames per row of the work buffer, its row stride in samples
    bool lockstep;                             // every active stream completes nfmax frames
    bool direct;                               // the frame launch writes the result itself: no pass follows it
    size_t in_bytes, out_bytes;                // wanted of the work buffer (0: not used) and of the output scratch
    size_t raw_off, stat_off;                  // bytes from the front of the output scratch: raw rows, static rows
};

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// frame_offsets (n + 1) and, where given, pending_after / held_after (n) of a push of chunks offsets[u] .. offsets[u + 1]
// to sessions that return row t once row t + lag is known: frame_offsets counts the rows RETURNED.  held may be NULL
// with lag = 0; raw_offsets (n + 1, may be NULL) gets the running sum of the frames computed.  On INVALID_PARAM
// frame_offsets is filled up to the offending stream
inline int plan_streams(size_t flen, size_t hop, size_t lag, const size_t *pending, const size_t *held, const size_t *offsets,
                        size_t n, size_t *frame_offsets, size_t *pending_after, size_t *held_after, size_t *raw_offsets) {
    frame_offsets[0] = 0;
    if (raw_offsets) raw_offsets[0] = 0;
    for (size_t u = 0; u < n; ++u) {
        const size_t hu = held ? held[u] : 0;
        if (offsets[u + 1] < offsets[u] || pending[u] >= flen || hu > lag) return MFCC_HIP_ERROR_INVALID_PARAM;
        size_t nf, pa;
        plan(pending[u], offsets[u + 1] - offsets[u], flen, hop, nf, pa);
        const size_t emitted = hu + nf > lag ? hu + nf - lag : 0;
        frame_offsets[u + 1] = frame_offsets[u] + emitted;
        if (raw_offsets) raw_offsets[u + 1] = raw_offsets[u] + nf;
        if (pending_after) pending_after[u] = pa;
        if (held_after) held_after[u] = hu + nf - emitted;
    }
    return MFCC_HIP_SUCCESS;
}

// The tables one behind the other and the scratch behind the block, from the counts already in l.  A table has records
// exactly when its pass runs: only a push gathers (a plain bank, unless in lockstep) or carries (into ring or tail)
inline void lay_out(const Settings &s, Layout &l, size_t n_cmvn, size_t n_delta, bool push) {
    size_t off = 0;
    auto table = [&off](size_t n, int rec_ll) {
        const Table t{off, n};
        off += n * size_t(rec_ll);
        return t;
    };
    l.bank = table(l.n_rec, kRecLL);
    l.gather = table(push && !s.online() && !l.lockstep ? l.n_active : 0, kGatherLL);
    l.cmvn = table(n_cmvn, mfcc_online::kRecLL);
    l.delta = table(n_delta, mfcc_online::kRecLL);
    l.carry = table(push && s.post() ? l.n_active : 0, mfcc_online::kRecLL);
    l.pcen = table(s.pcen ? l.n_active : 0, mfcc_pcen::kOnlineRecLL);
    l.desc_ll = off;
    l.in_bytes = l.n_active ? l.n_active * l.stride * 2 + 256 : 0;
    // an online bank: raw rows, then static rows; a plain one: the rows a gather reads, where the launch is not direct
    const size_t rows = l.n_active * l.nfmax * s.W * s.elem;
    const size_t rows_bytes = s.online() ? up256(rows) : l.direct ? 0 : rows;
    l.raw_off = up256(l.desc_ll * sizeof(long long));
    l.stat_off = l.raw_off + (s.online() ? rows_bytes : 0);
    l.out_bytes = l.stat_off + rows_bytes + 64;
}

// ---- push.  Count: the plan per stream, the totals and the layout.  Refusals in this order, nothing touched:
// INVALID_PARAM of the plan (frame_offsets filled up to the offending stream), BUFFER_SMALL (cap counts elements of
// out_width() wide rows), success without work when no stream got samples (l.n_rec == 0), INVALID_PARAM without samples
inline int push_plan(const Settings &s, const State &st, const size_t *offsets, size_t n, bool have_samples, bool have_out,
                     size_t cap, size_t *frame_offsets, size_t *pending_after, size_t *held_after, size_t *raw_offsets,
                     Layout &l) {
    l = Layout{};
    const int rc = plan_streams(s.flen, s.hop, s.L, st.pending, st.held, offsets, n, frame_offsets, pending_after, held_after,
                                raw_offsets);
    if (rc) return rc;
    if (frame_offsets[n] && (!have_out || cap < frame_offsets[n] * s.out_width())) return MFCC_HIP_ERROR_BUFFER_SMALL;
    size_t nfmin = ~size_t(0), max_total = 0, n_cmvn = 0, n_delta = 0;
    for (size_t u = 0; u < n; ++u) {
        const size_t n_new = offsets[u + 1] - offsets[u], nf = raw_offsets[u + 1] - raw_offsets[u];
        if (!n_new) continue;                          // nothing of this stream changes (nf > 0 needs new samples)
        ++l.n_rec;
        if (!nf) continue;
        ++l.n_active;
        l.nfmax = nf > l.nfmax ? nf : l.nfmax;
        nfmin = nf < nfmin ? nf : nfmin;
        max_total = st.pending[u] + n_new > max_total ? st.pending[u] + n_new : max_total;
        if (s.norm) n_cmvn += mfcc_online::online_runs(st.seen[u], nf, s.S);
        if (s.order) n_delta += (frame_offsets[u + 1] - frame_offsets[u] + s.g - 1) / s.g;
    }
    if (!l.n_rec) return MFCC_HIP_SUCCESS;
    if (!have_samples) return MFCC_HIP_ERROR_INVALID_PARAM;
    l.stride = 1 + max_total;
    l.lockstep = l.n_active && nfmin == l.nfmax;
    l.direct = l.lockstep && !s.online();              // the frame kernels' [active][nf][row] IS the result
    lay_out(s, l, n_cmvn, n_delta, true);
    return MFCC_HIP_SUCCESS;
}

// where the fill step is in each table
struct Cursor {
    Rec *bank;
    long long *gather;
    mfcc_online::Rec *cmvn, *delta, *carry;
    mfcc_pcen::OnlineRec *pcen;
    Cursor(const Layout &l, long long *p)
        : bank(reinterpret_cast<Rec *>(p + l.bank.off)), gather(p + l.gather.off),
          cmvn(reinterpret_cast<mfcc_online::Rec *>(p + l.cmvn.off)), delta(reinterpret_cast<mfcc_online::Rec *>(p + l.delta.off)),
          carry(reinterpret_cast<mfcc_online::Rec *>(p + l.carry.off)),
          pcen(reinterpret_cast<mfcc_pcen::OnlineRec *>(p + l.pcen.off)) {}
};

// The records of the passes behind the frame launch for one stream: its nf fresh rows [seen, seen + nf) start at row
// row0 of the raw rows, `emitted` rows from row seen - held on leave for row out_row of the result.  PCEN (where its
// table has records) writes the result itself unless CMVN or deltas follow; CMVN does unless deltas follow; one run per
// CMVN record, g rows per delta record, indices clamped to `last`
inline void pass_recs(const Settings &s, const Layout &l, Cursor &c, size_t u, size_t row0, size_t seen, size_t held, size_t nf,
                      size_t emitted, size_t out_row, long long last) {
    using mfcc_online::Rec;
    if (l.pcen.n)
        *c.pcen++ = mfcc_pcen::OnlineRec{(long long)u, (long long)row0, (long long)seen, (long long)nf,
                                         (long long)(s.post() ? row0 : out_row)};
    if (s.norm) {
        const size_t k = mfcc_online::online_runs(seen, nf, s.S), end = seen + nf;
        for (size_t i = 0, t0 = seen / s.S * s.S; i < k; ++i, t0 += s.S)
            *c.cmvn++ = Rec{(long long)u, (long long)row0, (long long)seen, (long long)nf, (long long)t0,
                            (long long)(t0 + s.S < end ? t0 + s.S : end), (long long)(s.order ? row0 : out_row), 0};
    }
    if (s.order) {
        const size_t e = seen - held;
        for (size_t i = 0; i < emitted; i += s.g)
            *c.delta++ = Rec{(long long)u, (long long)row0, (long long)seen, (long long)nf, (long long)(e + i),
                             (long long)(s.g < emitted - i ? s.g : emitted - i), (long long)(out_row + i), last};
    }
}

// Fill: every record of a planned push (l.n_rec > 0) into p[0 .. l.desc_ll); active records first, in stream order, the
// accumulate-only records behind them.  Stream u's chunk is samples[offsets[u] - shift .. offsets[u + 1] - shift)
inline void push_fill(const Settings &s, const State &st, const size_t *offsets, size_t shift, size_t n,
                      const size_t *frame_offsets, const size_t *raw_offsets, const Layout &l, long long *p) {
    Cursor c(l, p);
    Rec *idle = c.bank + l.n_active;
    size_t a = 0;
    for (size_t u = 0; u < n; ++u) {
        const size_t n_new = offsets[u + 1] - offsets[u], nf = raw_offsets[u + 1] - raw_offsets[u];
        if (!n_new) continue;
        const Rec r{(long long)u, (long long)(offsets[u] - shift), (long long)n_new, (long long)st.pending[u], (long long)nf};
        if (!nf) {
            *idle++ = r;
            continue;
        }
        *c.bank++ = r;
        const size_t row0 = a++ * l.nfmax, emitted = frame_offsets[u + 1] - frame_offsets[u];
        if (l.gather.n) {
            *c.gather++ = (long long)row0;
            *c.gather++ = (long long)frame_offsets[u];
            *c.gather++ = (long long)nf;
        }
        if (!s.online()) continue;
        pass_recs(s, l, c, u, row0, st.seen[u], st.held[u], nf, emitted, frame_offsets[u], mfcc_online::kNoEdge);
        if (l.carry.n)
            *c.carry++ = mfcc_online::Rec{(long long)u, (long long)row0, (long long)st.seen[u], (long long)nf, 0, 0, 0, 0};
    }
}

// ---- the end of the k listed streams (distinct, below the bank's size): a push without new samples.  emit: the
// zero-padded tail frame joins each stream as its last row; give: the held rows and that one are returned with the end
// clamped -- frame_offsets (k + 1) counts them -- else none is (a reset).  Either way the streams are back in the
// reset state afterwards, and nothing is carried.  BUFFER_SMALL as for a push; k == 0 plans no work (l.n_rec == 0)
inline int end_plan(const Settings &s, const State &st, const size_t *list, size_t k, bool emit, bool give, bool have_out,
                    size_t cap, size_t *frame_offsets, Layout &l) {
    l = Layout{};
    const size_t nf = emit && give ? 1 : 0;
    size_t n_cmvn = 0, n_delta = 0;
    frame_offsets[0] = 0;
    for (size_t i = 0; i < k; ++i) {
        const size_t rows = give ? st.held[list[i]] + nf : 0;
        frame_offsets[i + 1] = frame_offsets[i] + rows;
        if (s.norm) n_cmvn += mfcc_online::online_runs(st.seen[list[i]], nf, s.S);
        if (s.order) n_delta += (rows + s.g - 1) / s.g;
    }
    if (frame_offsets[k] && (!have_out || cap < frame_offsets[k] * s.out_width())) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (!k) return MFCC_HIP_SUCCESS;
    l.n_rec = k;
    l.n_active = nf * k;                               // without the tail frame no samples go to the work buffer
    l.nfmax = nf;
    l.stride = s.flen + 1;
    l.lockstep = true;
    l.direct = !s.online();
    lay_out(s, l, n_cmvn, n_delta, false);
    return MFCC_HIP_SUCCESS;
}

inline void end_fill(const Settings &s, const State &st, const size_t *list, const size_t *frame_offsets, const Layout &l,
                     long long *p) {
    Cursor c(l, p);
    for (size_t i = 0; i < l.n_rec; ++i) {
        const size_t u = list[i], seen = st.seen[u], rows = frame_offsets[i + 1] - frame_offsets[i];
        *c.bank++ = Rec{(long long)u, 0, 0, (long long)st.pending[u], (long long)l.nfmax};
        if (s.online() && rows)
            pass_recs(s, l, c, u, i * l.nfmax, seen, st.held[u], l.nfmax, rows, frame_offsets[i], (long long)(seen + l.nfmax) - 1);
    }
}

}  // namespace mfcc_bank
