// The host side of a segment pass: which tiles it runs over, the table the kernels read them from, where its scratch
// areas lie, and what a direct entry checks before it runs ("The tile planner").  Normalization,
// PCEN, deltas, sliding normalization, the VAD decision, the voiced-row selection and both gate entries plan here.  No HIP
// in here: the host tests compile this header on its own (tests/test_seg_plan_host.py).  Segs, BlockRec and tile_of are
// the kernels' (kernel_normalize.hpp includes this header for them).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/mfcc_hip.h"

#ifdef __HIPCC__
#define MFCC_SEG_HD __host__ __device__ __forceinline__
#else
#define MFCC_SEG_HD inline
#endif

namespace mfcc_norm {

// one tile of a segment (table form of Segs)
struct BlockRec {
    long long row0;
    int rows;
    int seg;
};

// The tiles of a call.  Uniform form (blk == nullptr): n_segs segments of seg_rows rows each, back to back from row
// base_row, blocks_per_seg tiles each (a dense multi-channel call, equal-length utterances).  Table form: one record
// per tile and the first tile of every segment (seg_blk0, n_segs + 1 entries), built on the host.
struct Segs {
    long long base_row, seg_rows, blocks_per_seg;
    const BlockRec *blk;
    const long long *seg_blk0;
    long long n_blocks, n_segs;
    int width, tile_rows;
};

MFCC_SEG_HD void tile_of(const Segs &s, long long b, long long &row0, int &rows, long long &seg) {
    if (!s.blk) {
        seg = b / s.blocks_per_seg;
        const long long k = b - seg * s.blocks_per_seg;
        row0 = s.base_row + seg * s.seg_rows + k * s.tile_rows;
        const long long left = s.seg_rows - k * s.tile_rows;
        rows = int(left < s.tile_rows ? left : s.tile_rows);
    } else {
        const BlockRec r = s.blk[b];
        row0 = r.row0;
        rows = r.rows;
        seg = r.seg;
    }
}

}  // namespace mfcc_norm

namespace mfcc_seg {

using mfcc_norm::BlockRec;
using mfcc_norm::Segs;

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// ---- which rows are segments: n_segs runs of seg_rows rows back to back from row base_row (a dense call: one per
// channel), or segment k = rows off[k] .. off[k + 1] (off does not decrease; checked by the caller)
struct SegSpan {
    const size_t *off;      // nullptr: the uniform form
    size_t n_segs, base_row, seg_rows;
};

inline SegSpan span_uniform(size_t base_row, size_t n_segs, size_t seg_rows) { return SegSpan{nullptr, n_segs, base_row, seg_rows}; }
inline SegSpan span_offsets(const size_t *off, size_t n_segs) { return SegSpan{off, n_segs, 0, 0}; }

// no segment, or no row in any: every pass answers success before anything else
inline bool span_empty(const SegSpan &sp) {
    return sp.n_segs == 0 || (sp.off ? sp.off[sp.n_segs] == sp.off[0] : sp.seg_rows == 0);
}

inline bool offsets_ok(const size_t *off, size_t n_segs) {
    for (size_t k = 0; k < n_segs; ++k)
        if (off[k + 1] < off[k]) return false;
    return true;
}

// address ranges [lo, hi) that overlap
inline bool ranges_overlap(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) {
    return a_lo < b_hi && b_lo < a_hi;
}

// ---- the planner.  The tiles of tile_rows units of a span that is not empty: Segs and, for the table form, the length
// of its table in long longs.  The table is [first tile of every segment (n_segs + 1)][extra (n_segs), where the plan has
// the column][one record per tile].  The extra column of a plan over offsets comes from a second set of offsets:
// extra[k] = base[k] - off[k] * step (the gate: the rows of the segments against their window offsets, Wins::delta)
struct Column {
    const size_t *base;
    size_t step;
};

inline long long column_at(const Column &c, const size_t *off, size_t k) {
    return (long long)c.base[k] - (long long)(off[k] * c.step);
}

struct Plan {
    Segs s;                 // the uniform form as the kernels take it; the table form still lacks its pointers (plan_bind)
    size_t table_ll;        // 0: the uniform form
    bool extra;
};

static_assert(sizeof(BlockRec) == 2 * sizeof(long long), "record layout");

// Count.  A uniform span is filled in as it is -- a dense call may have tens of thousands of channels: no loop, no
// table.  Offsets give the uniform form when every segment has one length (and the extra column, where given, one step
// from each to the next, the end of the last segment included), else the table form.  Touches nothing but pl
inline int plan_count(const SegSpan &sp, int width, int tile_rows, const Column *extra, Plan &pl) {
    const size_t tr = size_t(tile_rows), n_segs = sp.n_segs;
    pl = Plan{};
    pl.s.width = width;
    pl.s.tile_rows = tile_rows;
    pl.s.n_segs = (long long)n_segs;
    const size_t *off = sp.off;
    const size_t len0 = off ? off[1] - off[0] : sp.seg_rows;
    auto step = [&](size_t k) { return extra ? column_at(*extra, off, k + 1) - column_at(*extra, off, k) : 0; };
    bool uniform = true;
    for (size_t k = 1; off && k < n_segs && uniform; ++k) uniform = off[k + 1] - off[k] == len0 && step(k) == step(0);
    if (uniform) {
        pl.s.base_row = (long long)(off ? off[0] : sp.base_row);
        pl.s.seg_rows = (long long)len0;
        pl.s.blocks_per_seg = (long long)((len0 + tr - 1) / tr);
        pl.s.n_blocks = pl.s.blocks_per_seg * pl.s.n_segs;
        return MFCC_HIP_SUCCESS;
    }
    if (n_segs >= (size_t(1) << 31)) return MFCC_HIP_ERROR_INVALID_PARAM;       // BlockRec::seg is an int
    size_t n_blocks = 0;
    for (size_t k = 0; k < n_segs; ++k) n_blocks += (off[k + 1] - off[k] + tr - 1) / tr;
    pl.s.n_blocks = (long long)n_blocks;
    pl.extra = extra != nullptr;
    pl.table_ll = n_segs + 1 + (extra ? n_segs : 0) + 2 * n_blocks;
    return MFCC_HIP_SUCCESS;
}

// Fill: the table of a table-form plan into table[0 .. pl.table_ll)
inline void plan_fill(const SegSpan &sp, const Column *extra, const Plan &pl, long long *table) {
    const size_t tr = size_t(pl.s.tile_rows), n_segs = sp.n_segs;
    long long *blk0 = table, *col = table + n_segs + 1;
    BlockRec *rec = reinterpret_cast<BlockRec *>(col + (extra ? n_segs : 0));
    size_t b = 0;
    for (size_t k = 0; k < n_segs; ++k) {
        blk0[k] = (long long)b;
        if (extra) col[k] = column_at(*extra, sp.off, k);
        for (size_t r = sp.off[k]; r < sp.off[k + 1]; r += tr) {
            const size_t left = sp.off[k + 1] - r;
            rec[b++] = BlockRec{(long long)r, int(left < tr ? left : tr), int(k)};
        }
    }
    blk0[n_segs] = (long long)b;
}

// Bind: points a table-form plan at the copy of its table at d_table; returns the extra column there (nullptr without)
inline const long long *plan_bind(Plan &pl, const long long *d_table) {
    if (!pl.table_ll) return nullptr;
    const size_t n_segs = size_t(pl.s.n_segs);
    pl.s.seg_blk0 = d_table;
    pl.s.blk = reinterpret_cast<const BlockRec *>(d_table + n_segs + 1 + (pl.extra ? n_segs : 0));
    return pl.extra ? d_table + n_segs + 1 : nullptr;
}

// ---- the scratch of a pass: its areas one behind the other, each rounded up to 256 bytes, the tile table last
struct Area {
    size_t per_tile, per_seg, fixed;        // bytes = n_blocks * per_tile + n_segs * per_seg + fixed
};
constexpr int kMaxAreas = 3;

struct Scratch {
    size_t off[kMaxAreas];
    size_t table_off, total;                // total: what the pass asks of its buffer
};

inline Scratch lay_out(const Area *areas, int n_areas, const Plan &pl) {
    Scratch l{};
    size_t at = 0;
    for (int i = 0; i < n_areas; ++i) {
        l.off[i] = at;
        at += up256(size_t(pl.s.n_blocks) * areas[i].per_tile + size_t(pl.s.n_segs) * areas[i].per_seg + areas[i].fixed);
    }
    l.table_off = at;
    l.total = at + pl.table_ll * sizeof(long long) + 64;
    return l;
}

// the selection (rows or gate windows): [tile counts (unsigned)][tile prefixes (n_blocks + 1)][segment offsets (n_segs + 1)]
constexpr Area kSelectAreas[3] = {{sizeof(unsigned), 0, 0}, {sizeof(long long), 0, sizeof(long long)},
                                  {0, sizeof(long long), sizeof(long long)}};

// ---- what a direct entry (mfcc_hip_*_dev on rows) checks before it runs.  Every pointer comes with the alignment it
// needs, the bytes of one of its units and its role: rows read or written are rows off[0] .. off[n_segs] behind the
// pointer; a packed output holds units 0 .. (number of units of the call); kUnsized: its range is not known yet
enum Role { kRead, kWrite, kWritePacked, kUnsized };

struct RowPtr {
    const void *p;
    size_t align, unit_bytes;
    Role role;
    bool optional;          // may be NULL: then it is not looked at
};

struct RowCall {
    int width, max_width;
    const size_t *off;      // rows of the segments
    size_t n_segs;
    const size_t *units;    // what the packed outputs count, where that is not rows (the gate: window offsets, which the
                            // caller made from off and so has checked off already); else nullptr
    const RowPtr *ptr;
    int n_ptr;
};

constexpr int kProceed = 1, kNothing = 2;       // next to the (negative) error codes: go on; nothing to do, success

// Width, offsets, then the empty span (kNothing: no pointer is looked at), then every pointer, then every written range
// against every other range
inline int check_rows(const RowCall &c) {
    if (c.width < 1 || c.width > c.max_width || (c.n_segs && !c.off)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!c.units && !offsets_ok(c.off, c.n_segs)) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t *u = c.units ? c.units : c.off;
    if (c.n_segs == 0 || u[c.n_segs] == u[0]) return kNothing;
    uintptr_t lo[8], hi[8];
    for (int i = 0; i < c.n_ptr; ++i) {
        const RowPtr &a = c.ptr[i];
        const uintptr_t p = reinterpret_cast<uintptr_t>(a.p);
        if ((!a.p && !a.optional) || (p & (a.align - 1))) return MFCC_HIP_ERROR_INVALID_PARAM;
        const bool packed = a.role == kWritePacked;
        lo[i] = p + (packed ? 0 : c.off[0]) * a.unit_bytes;
        hi[i] = p + (packed ? u[c.n_segs] - u[0] : c.off[c.n_segs]) * a.unit_bytes;
    }
    for (int i = 0; i < c.n_ptr; ++i)
        for (int j = 0; j < c.n_ptr; ++j) {
            const RowPtr &a = c.ptr[i], &b = c.ptr[j];
            const bool sized = a.p && b.p && a.role != kUnsized && b.role != kUnsized;
            if (i != j && sized && a.role != kRead && ranges_overlap(lo[i], hi[i], lo[j], hi[j])) return MFCC_HIP_ERROR_INVALID_PARAM;
        }
    return kProceed;
}

}  // namespace mfcc_seg
