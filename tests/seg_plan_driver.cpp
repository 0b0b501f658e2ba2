// Prints what mfcc_amd/csrc/seg_plan.hpp makes of every case on stdin (tests/test_seg_plan_host.py).  A case is one line
// of numbers behind its kind:
//   plan  width tile_rows n_segs n_given extra n_areas  off[n_given] (base[n_given] step)  (per_tile per_seg fixed)[n_areas]
//   dense width tile_rows n_segs base_row seg_rows n_areas                             (per_tile per_seg fixed)[n_areas]
//   check width max_width n_segs has_off has_units n_ptr  (off[n_segs + 1]) (units[n_segs + 1])
//                                                         (address align unit_bytes role optional)[n_ptr]
// n_given is n_segs + 1 except where the count is faked; n_areas -1 stands for the selection's areas.  The answer is one
// line.  check: the code.  plan / dense: rc, then after MFCC_HIP_SUCCESS the Segs (base_row seg_rows blocks_per_seg n_blocks
// n_segs width tile_rows), table_ll, the table (which starts out as -7777 everywhere), has_extra, the area offsets,
// table_off, total, and every tile as tile_of gives it from the bound plan: row0 rows seg.
// The table is allocated at exactly table_ll long longs: under -fsanitize=address a record past its end is an error.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "seg_plan.hpp"

using namespace mfcc_seg;

static bool read_n(std::vector<size_t> &v, size_t n) {
    v.assign(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (scanf("%zu", &v[i]) != 1) return false;
    return true;
}

static int plan_case(bool dense) {
    int width, tile_rows, has_extra = 0, n_areas;
    size_t n_segs, n_given = 0, base_row = 0, seg_rows = 0;
    if (scanf("%d %d %zu", &width, &tile_rows, &n_segs) != 3) return 2;
    if (dense ? scanf("%zu %zu", &base_row, &seg_rows) != 2 : scanf("%zu %d", &n_given, &has_extra) != 2) return 2;
    if (scanf("%d", &n_areas) != 1) return 2;
    std::vector<size_t> off, ex;
    Column column{nullptr, 0};
    if (!read_n(off, n_given) || !read_n(ex, has_extra ? n_given : 0) || (has_extra && scanf("%zu", &column.step) != 1)) return 2;
    column.base = ex.data();
    std::vector<Area> areas(kSelectAreas, kSelectAreas + 3);
    if (n_areas >= 0) {
        areas.resize(size_t(n_areas));
        for (Area &a : areas)
            if (scanf("%zu %zu %zu", &a.per_tile, &a.per_seg, &a.fixed) != 3) return 2;
    }
    const SegSpan sp = dense ? span_uniform(base_row, n_segs, seg_rows) : span_offsets(off.data(), n_segs);
    const Column *ep = has_extra ? &column : nullptr;
    Plan pl;
    const int rc = plan_count(sp, width, tile_rows, ep, pl);
    printf("%d", rc);
    if (rc == MFCC_HIP_SUCCESS) {
        long long *table = new long long[pl.table_ll];
        for (size_t i = 0; i < pl.table_ll; ++i) table[i] = -7777;
        if (pl.table_ll) plan_fill(sp, ep, pl, table);
        const Scratch lay = lay_out(areas.data(), int(areas.size()), pl);
        const long long *col = plan_bind(pl, table);
        const Segs &s = pl.s;
        printf(" %lld %lld %lld %lld %lld %d %d %zu", s.base_row, s.seg_rows, s.blocks_per_seg, s.n_blocks, s.n_segs, s.width,
               s.tile_rows, pl.table_ll);
        for (size_t i = 0; i < pl.table_ll; ++i) printf(" %lld", table[i]);
        printf(" %d", int(col != nullptr));
        if (col && col != table + n_segs + 1) return 3;
        for (size_t i = 0; i < areas.size(); ++i) printf(" %zu", lay.off[i]);
        printf(" %zu %zu", lay.table_off, lay.total);
        for (long long b = 0; b < s.n_blocks; ++b) {
            long long row0, seg;
            int rows;
            mfcc_norm::tile_of(s, b, row0, rows, seg);
            printf(" %lld %d %lld", row0, rows, seg);
        }
        delete[] table;
    }
    printf("\n");
    return 0;
}

static int check_case() {
    RowCall c{};
    int has_off, has_units;
    if (scanf("%d %d %zu %d %d %d", &c.width, &c.max_width, &c.n_segs, &has_off, &has_units, &c.n_ptr) != 6) return 2;
    std::vector<size_t> off, units;
    if (!read_n(off, has_off ? c.n_segs + 1 : 0) || !read_n(units, has_units ? c.n_segs + 1 : 0)) return 2;
    std::vector<RowPtr> ptr(size_t(c.n_ptr), RowPtr{});
    for (RowPtr &p : ptr) {
        size_t address;
        int role, optional;
        if (scanf("%zu %zu %zu %d %d", &address, &p.align, &p.unit_bytes, &role, &optional) != 5) return 2;
        p.p = reinterpret_cast<const void *>(address);
        p.role = Role(role);
        p.optional = optional != 0;
    }
    c.off = has_off ? off.data() : nullptr;
    c.units = has_units ? units.data() : nullptr;
    c.ptr = ptr.data();
    printf("%d\n", check_rows(c));
    return 0;
}

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        const int rc = !strcmp(kind, "check") ? check_case() : plan_case(!strcmp(kind, "dense"));
        if (rc) return rc;
    }
    return 0;
}
