// Prints what mfcc_amd/csrc/batch_plan.hpp makes of every case on stdin (tests/test_batch_plan_host.py).  A case is one
// line of numbers behind its kind:
//   ragged frame_len hop stream tile tile_hop s_used row_bytes kernel fixed lim_len lim_tiles chunk_bytes n_utt off[n_utt + 1]
//   dense  frame_len hop stream n nch row chunk_bytes
// kernel: mfcc_batch::Records; lim_len / lim_tiles 0: the defaults.  The answer is one line.
// ragged: rc, and after MFCC_HIP_SUCCESS total n_tiles max_len len0 frames0 uniform, frame_offsets[n_utt + 1], the route,
//   table_ll of the route, the pack plan (len F desc_ll gather_ll in_bytes desc_off out_bytes) and its table, the tile plan
//   (n_tiles chan_ll map_off bytes) and 6 fields per RaggedChan, the record plan (n_recs rec_ll bytes) and 6 fields per
//   RaggedRec, the number of utterance ranges and (u0 u1 rows0 rows1) of each.  After an error: frame_offsets as far as written.
// dense: frames, dense_cuts_channels, max_chunk_rows, the number of chunks and the 9 fields of each.
// Every table is allocated at exactly the length its plan names and starts out as -7777: under -fsanitize=address a
// record past its end is an error.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "batch_plan.hpp"

using namespace mfcc_batch;

static int ragged_case() {
    Framing f{};
    TileGeom g{};
    int stream, kernel, fixed;
    size_t row_bytes, lim_len, lim_tiles, chunk_bytes, n_utt;
    if (scanf("%zu %zu %d %d %d %d %zu %d %d %zu %zu %zu %zu", &f.frame_len, &f.hop, &stream, &g.tile, &g.tile_hop, &g.s_used,
              &row_bytes, &kernel, &fixed, &lim_len, &lim_tiles, &chunk_bytes, &n_utt) != 13)
        return 2;
    f.stream = stream != 0;
    std::vector<size_t> off(n_utt + 1), fo(n_utt + 1, 7777);
    for (size_t &o : off)
        if (scanf("%zu", &o) != 1) return 2;
    const Scan sc = scan(off.data(), n_utt, f, size_t(g.tile), fo.data());
    printf("%d", sc.rc);
    if (sc.rc) {
        for (size_t v : fo) printf(" %zu", v);
        printf("\n");
        return 0;
    }
    printf(" %zu %zu %zu %zu %zu %d", sc.total, sc.n_tiles, sc.max_len, sc.len0, sc.frames0, int(sc.uniform));
    for (size_t v : fo) printf(" %zu", v);
    // the scan by a function of the caller's gives the same
    std::vector<size_t> fo2(n_utt + 1, 7777);
    const Scan sc2 =
        scan_with(off.data(), n_utt, size_t(g.tile), [&](size_t u, size_t) { return fo[u + 1] - fo[u]; }, fo2.data());
    if (fo2 != fo || sc2.total != sc.total || sc2.n_tiles != sc.n_tiles || sc2.max_len != sc.max_len || sc2.uniform != sc.uniform)
        return 3;
    Limits lim;
    if (lim_len) lim.len = lim_len;
    if (lim_tiles) lim.tiles = lim_tiles;
    const Route r = route(Records(kernel), fixed != 0, sc, n_utt, lim);
    printf(" %d %zu", int(r), table_ll(r, n_utt));

    std::vector<long long> desc(7 * n_utt, -7777);
    const PackPlan pp = fill_pack(off.data(), fo.data(), n_utt, f, row_bytes, desc.data());
    printf(" %zu %zu %zu %zu %zu %zu %zu", pp.len, pp.F, pp.desc_ll, pp.gather_ll, pp.in_bytes, pp.desc_off, pp.out_bytes);
    if (pp.desc_ll != desc.size()) return 3;
    for (long long v : desc) printf(" %lld", v);

    std::vector<RaggedChan> chans(n_utt, RaggedChan{-7777, -7777, -7777, -7777, -7777, -7777});
    const TilePlan tp = fill_chans(off.data(), fo.data(), n_utt, g, chans.data());
    printf(" %zu %zu %zu %zu", tp.n_tiles, tp.chan_ll, tp.map_off, tp.bytes);
    if (tp.chan_ll * sizeof(long long) != chans.size() * sizeof(RaggedChan)) return 3;
    for (const RaggedChan &c : chans) printf(" %lld %lld %d %d %d %d", c.pcm_off, c.out_row, c.n_samples, c.frames, c.t_hi, c.tile0);

    size_t with_frames = 0;
    for (size_t u = 0; u < n_utt; ++u) with_frames += fo[u + 1] > fo[u];
    std::vector<RaggedRec> recs(with_frames, RaggedRec{-7777, -7777, -7777, -7777, -7777, -7777});
    const RecPlan rp = fill_recs(off.data(), fo.data(), n_utt, recs.data());
    printf(" %zu %zu %zu", rp.n_recs, rp.rec_ll, rp.bytes);
    if (rp.n_recs != recs.size()) return 3;
    for (const RaggedRec &c : recs) printf(" %lld %lld %d %d %d %d", c.pcm_off, c.out_row, c.n_samples, c.frames, c.pad0, c.pad1);

    const std::vector<UttRange> ranges = cut_ragged(off.data(), fo.data(), n_utt, chunk_bytes);
    printf(" %zu", ranges.size());
    for (const UttRange &u : ranges) printf(" %zu %zu %zu %zu", u.u0, u.u1, u.rows0, u.rows1);
    printf("\n");
    return 0;
}

static int dense_case() {
    Framing f{};
    int stream;
    size_t n, nch, row, chunk_bytes;
    if (scanf("%zu %zu %d %zu %zu %zu %zu", &f.frame_len, &f.hop, &stream, &n, &nch, &row, &chunk_bytes) != 7) return 2;
    f.stream = stream != 0;
    const size_t nf = frames_of(f, n);
    const std::vector<HostChunk> chunks = nf && nch ? cut_dense(n, nch, nf, row, f, chunk_bytes) : std::vector<HostChunk>();
    printf("%zu %d %zu %zu", nf, int(dense_cuts_channels(n, chunk_bytes)), max_chunk_rows(chunks), chunks.size());
    for (const HostChunk &c : chunks)
        printf(" %zu %zu %zu %zu %zu %d %zu %zu %zu", c.in_off, c.in_samples, c.n, c.stride, c.nch, c.halo, c.frames, c.out_elems,
               c.out_off);
    printf("\n");
    return 0;
}

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        const int rc = !strcmp(kind, "dense") ? dense_case() : ragged_case();
        if (rc) return rc;
    }
    return 0;
}
