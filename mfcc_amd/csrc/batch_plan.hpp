// The host side of a batch call: what a ragged call (mfcc_hip_process_ragged_*) and a host-buffer call (mfcc_hip_process_*
// on host pointers) decide before anything is launched ("The batch plan").  One scan of the
// utterance offsets, the route of the call, the tables each route hands to its kernels with the byte layout of the
// device buffers they go to, and the chunks a host buffer crosses the wire in.  Everything here is an address or a length
// that a kernel reads or writes.  No HIP in here: the host tests compile this header on its own
// (tests/test_batch_plan_host.py).  RaggedChan, RaggedTile and RaggedRec are the kernels' (kernel_fused512_w12.hpp and
// kernel_fixed512.hpp include this header for them): they read them with scalar loads at fixed offsets.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/mfcc_hip.h"

namespace mfcc_fused12 {

// ---- ragged corpora without a packing copy: the tiles of utterances of different lengths, straight out of the
// caller's buffer.  The host writes one record per utterance, a small kernel expands them into one 32-byte record per
// tile, and a wave fetches its next tile's record with one scalar load, a tile ahead of its use.  Every utterance is an
// independent stream that starts from reset (history 0) and is zero-padded at its end, exactly like a channel of the
// plain call -- so the frames are the same bits as one call per utterance.
struct RaggedChan {
    long long pcm_off;       // first sample of the utterance, relative to StreamDesc::pcm
    long long out_row;       // first output row (frame) of the utterance
    int n_samples, frames;   // of the utterance
    int t_hi;                // tiles 1 .. t_hi have their whole window inside the utterance
    int tile0;               // index of its first tile in the tile map
};
// what a wave needs to know about a tile, in one 32-byte record (one s_load_dwordx8): expanded from the utterance
// records by ragged_tile_map_kernel
struct RaggedTile {
    long long pcm_off;       // first sample of the tile's utterance, relative to StreamDesc::pcm
    long long out_row;       // first output row (frame) of that utterance
    int n_samples, frames;   // of the utterance
    int t_hi;                // tiles 1 .. t_hi of the utterance have their whole window inside it
    int t_in;                // the tile's index inside its utterance
};

// tile_hop samples from a tile to the next, s_used samples in a tile's window (the kernel's kTileHop, kSUsed)
inline int ragged_t_hi(long long n_samples, long long tiles, int tile_hop, int s_used) {
    if (n_samples < s_used) return -1;
    const long long hi = (n_samples - s_used) / tile_hop;
    return (int)(hi < tiles ? hi : tiles);
}

}  // namespace mfcc_fused12

namespace mfcc_fixed512 {

// One utterance of a ragged corpus (mfcc_hip_process_ragged_*): an independent stream that starts from reset and is
// zero-padded at its end, exactly like a channel of the plain call.  Only utterances with frames > 0 get a record.
struct RaggedRec {
    long long pcm_off;       // first sample, relative to StreamDesc::pcm
    long long out_row;       // first output row (frame) of the utterance == frames of all utterances before it
    int n_samples, frames;
    int pad0, pad1;
};

}  // namespace mfcc_fixed512

namespace mfcc_batch {

using mfcc_fixed512::RaggedRec;
using mfcc_fused12::RaggedChan;
using mfcc_fused12::RaggedTile;

static_assert(sizeof(RaggedChan) == 4 * sizeof(long long) && sizeof(RaggedTile) == 4 * sizeof(long long) &&
                  sizeof(RaggedRec) == 4 * sizeof(long long),
              "record layout");

// ---- frames of n samples: frames of frame_len samples every hop; stream: a zero-padded one behind the last whole one
struct Framing {
    size_t frame_len, hop;
    bool stream;
};

inline size_t frames_of(const Framing &f, size_t n) {
    if (n < f.frame_len) return f.stream ? 1 : 0;
    return (n - f.frame_len) / f.hop + (f.stream ? 2 : 1);
}

// the fused 512 kernel's tiles, as mfcc_hip.hip passes them in: frames per tile, samples from a tile to the next, samples
// in a tile's window
struct TileGeom {
    int tile, tile_hop, s_used;
};

// ---- the scan of a ragged call: ONE pass over offsets[0 .. n_utt].  Stops at the first offset below the one before
// it (rc = MFCC_HIP_ERROR_INVALID_PARAM; frame_offsets is then written up to there); else frame_offsets[0 .. n_utt] is
// the prefix sum of the frame counts
struct Scan {
    int rc;
    size_t total;           // frames
    size_t n_tiles;         // tiles of `tile` frames, every utterance tiled on its own
    size_t max_len;         // samples of the longest utterance: 0 -- the call reads no sample
    size_t len0, frames0;   // of utterance 0
    bool uniform;           // every utterance has len0 samples, and these have a frame
};

// frames(u, n): frames of utterance u, which has n samples; asked once per run of equal lengths
template <typename Frames>
inline Scan scan_with(const size_t *offsets, size_t n_utt, size_t tile, Frames &&frames, size_t *frame_offsets) {
    Scan s{};
    bool equal = true;
    frame_offsets[0] = 0;
    for (size_t u = 0; u < n_utt;) {
        if (offsets[u + 1] < offsets[u]) {
            s.rc = MFCC_HIP_ERROR_INVALID_PARAM;
            return s;
        }
        const size_t n = offsets[u + 1] - offsets[u], nf = frames(u, n), tiles = (nf + tile - 1) / tile;
        if (u == 0) {
            s.len0 = n;
            s.frames0 = nf;
        }
        equal = equal && n == s.len0;
        if (n > s.max_len) s.max_len = n;
        // the run of utterances of this length: one frame count, one division (a corpus of equal lengths is the per-step
        // host work of a sharded corpus, bench.py `enqueue_us_per_step`)
        size_t end = u + 1;
        while (end < n_utt && offsets[end + 1] >= offsets[end] && offsets[end + 1] - offsets[end] == n) ++end;
        s.n_tiles += tiles * (end - u);
        for (; u < end; ++u) frame_offsets[u + 1] = s.total += nf;
    }
    s.uniform = n_utt >= 1 && equal && s.frames0 > 0;
    return s;
}

// ... by the framing
inline Scan scan(const size_t *offsets, size_t n_utt, const Framing &f, size_t tile, size_t *frame_offsets) {
    return scan_with(offsets, n_utt, tile, [&](size_t, size_t n) { return frames_of(f, n); }, frame_offsets);
}

// ---- the route of a ragged call with at least one frame
enum class Route {
    kUniform,       // equal lengths back to back ARE a multi-channel stream: the plain launch, stride = length
    kTileRecords,   // float contract on the twelve-wave 512 kernel: RaggedChan per utterance, RaggedTile per tile
    kFrameRecords,  // fixed contract on the fused 512 kernel: RaggedRec per utterance with frames
    kPackGather     // everything else: pack into one stream, one launch, gather the rows
};

// what the kernel that runs the call can read utterances from
enum class Records { kNone, kTiles, kFrames };

// below these a record describes its corpus: utterances and samples per utterance (the records' int fields), tiles
// (the tile map's int index)
struct Limits {
    size_t len = size_t(1) << 31, tiles = size_t(1) << 30;
};

inline Route route(Records kernel, bool fixed, const Scan &s, size_t n_utt, const Limits &lim = Limits{}) {
    if (s.uniform) return Route::kUniform;
    const bool rec_fits = n_utt < lim.len && s.max_len < lim.len;
    if (!fixed && kernel == Records::kTiles && rec_fits && s.n_tiles < lim.tiles) return Route::kTileRecords;
    if (fixed && kernel == Records::kFrames && rec_fits) return Route::kFrameRecords;
    return Route::kPackGather;
}

// ---- the tables.  off: the n_utt + 1 sample offsets, fo: their frame offsets (the scan's)

// long longs of host memory the table of a route takes (at most)
inline size_t table_ll(Route r, size_t n_utt) {
    return r == Route::kUniform ? 0 : r == Route::kPackGather ? 7 * n_utt : 4 * n_utt;
}

// Pack and gather.  The utterances are packed into ONE stream at offsets that are multiples of the hop, separated by
// zeros: at least one zero in front (pre-emphasis history 0, like after the driver's soft reset, main.c:21-34) and zeros
// behind up to the end of the last frame (the zero-padded tail of main.c:134-144).  Frame k of utterance u is then frame
// start_u / hop + k of the packed stream -- the same samples, the same arithmetic, bit for bit -- and the frames that
// fall into the gaps are simply not copied out.
struct PackPlan {
    size_t len, F;          // samples and frames (every hop position is one) of the packed stream
    size_t desc_ll;         // the table: [pack descriptors, 4 per utterance][gather descriptors, 3 per utterance]
    size_t gather_ll;       // where the gather descriptors start in it
    size_t in_bytes;        // the stream's buffer
    size_t desc_off;        // the rows' buffer: F rows, the table at desc_off ...
    size_t out_bytes;       // ... out_bytes in all
};

// pack descriptor: (source offset, destination offset, samples, end of this utterance's part of the stream); gather
// descriptor: (first row in the stream, first row of the result, rows).  row_bytes: of a row of the result
inline PackPlan fill_pack(const size_t *off, const size_t *fo, size_t n_utt, const Framing &f, size_t row_bytes, long long *desc) {
    long long *gather = desc + 4 * n_utt;
    size_t pos = 0, last_with_frames = n_utt;
    for (size_t u = 0; u < n_utt; ++u) {
        const size_t n = off[u + 1] - off[u], nf = fo[u + 1] - fo[u];
        desc[4 * u] = (long long)off[u];
        desc[4 * u + 1] = (long long)pos;
        desc[4 * u + 2] = nf ? (long long)n : 0;
        gather[3 * u] = (long long)(pos / f.hop);
        gather[3 * u + 1] = (long long)fo[u];
        gather[3 * u + 2] = (long long)nf;
        if (nf) {
            const size_t last_end = f.hop * (nf - 1) + f.frame_len, extent = n > last_end ? n : last_end;
            pos = (pos + extent + 1 + f.hop - 1) / f.hop * f.hop;
            last_with_frames = u;
        }
        desc[4 * u + 3] = (long long)pos;          // this utterance's part of the stream ends where the next begins
    }
    PackPlan p{};
    p.F = pos / f.hop;
    p.len = pos + f.frame_len + f.hop;
    if (last_with_frames < n_utt) desc[4 * last_with_frames + 3] = (long long)p.len;     // the last one also zeroes the tail
    p.desc_ll = 7 * n_utt;
    p.gather_ll = 4 * n_utt;
    p.in_bytes = p.len * sizeof(int16_t) + 64;
    p.desc_off = (p.F * row_bytes + 7) & ~size_t(7);
    p.out_bytes = p.F * row_bytes + p.desc_ll * sizeof(long long) + 64;
    return p;
}

// Tile records: one RaggedChan per utterance, frameless ones included (no tile)
struct TilePlan {
    size_t n_tiles;
    size_t chan_ll;         // the table, in long longs
    size_t map_off;         // the device buffer: the table, the tile map (RaggedTile per tile) at map_off ...
    size_t bytes;           // ... bytes in all
};

inline TilePlan fill_chans(const size_t *off, const size_t *fo, size_t n_utt, const TileGeom &g, RaggedChan *chans) {
    size_t n_tiles = 0;
    for (size_t u = 0; u < n_utt; ++u) {
        const size_t n = off[u + 1] - off[u], nf = fo[u + 1] - fo[u], tiles = (nf + size_t(g.tile) - 1) / size_t(g.tile);
        RaggedChan c;
        c.pcm_off = (long long)off[u];
        c.out_row = (long long)fo[u];
        c.n_samples = (int)n;
        c.frames = (int)nf;
        c.t_hi = mfcc_fused12::ragged_t_hi((long long)n, (long long)tiles, g.tile_hop, g.s_used);
        c.tile0 = (int)n_tiles;
        chans[u] = c;
        n_tiles += tiles;
    }
    TilePlan p{};
    p.n_tiles = n_tiles;
    p.chan_ll = 4 * n_utt;
    p.map_off = (n_utt * sizeof(RaggedChan) + 255) & ~size_t(255);
    p.bytes = p.map_off + n_tiles * sizeof(RaggedTile) + 64;
    return p;
}

// Frame records: one RaggedRec per utterance with frames
struct RecPlan {
    size_t n_recs;
    size_t rec_ll;          // the table, in long longs
    size_t bytes;           // the device buffer: the table
};

inline RecPlan fill_recs(const size_t *off, const size_t *fo, size_t n_utt, RaggedRec *recs) {
    size_t n_recs = 0;
    for (size_t u = 0; u < n_utt; ++u) {
        const size_t nf = fo[u + 1] - fo[u];
        if (!nf) continue;
        RaggedRec c;
        c.pcm_off = (long long)off[u];
        c.out_row = (long long)fo[u];
        c.n_samples = (int)(off[u + 1] - off[u]);
        c.frames = (int)nf;
        c.pad0 = c.pad1 = 0;
        recs[n_recs++] = c;
    }
    RecPlan p{};
    p.n_recs = n_recs;
    p.rec_ll = 4 * n_recs;
    p.bytes = n_recs * sizeof(RaggedRec) + 64;
    return p;
}

// ---- the chunks of a host-buffer call (run_host_pipeline): about chunk_bytes of int16 samples each

// a dense call: nch channels of n samples, nf > 0 frames each, rows of `row` elements
struct HostChunk {
    size_t in_off;          // first sample handed to the kernel (the halo sample when halo = 1), from the call's first
    size_t in_samples;      // samples copied (all channels of the chunk; incl. the halo sample)
    size_t n, stride, nch;  // launch geometry: samples per channel after the halo, channel stride, channels
    int halo;
    size_t frames;          // frames per channel of this chunk (forced: a frame range of a longer stream)
    size_t out_elems;       // coefficients written
    size_t out_off;         // offset into `out`, in elements
};

// a channel that fits a chunk: chunks of whole channels; else frame ranges of one channel (dense_cuts_channels)
inline bool dense_cuts_channels(size_t n, size_t chunk_bytes) { return n * sizeof(int16_t) > chunk_bytes; }

inline std::vector<HostChunk> cut_dense(size_t n, size_t nch, size_t nf, size_t row, const Framing &f, size_t chunk_bytes) {
    std::vector<HostChunk> chunks;
    const size_t ch_bytes = n * sizeof(int16_t);
    if (!dense_cuts_channels(n, chunk_bytes)) {
        size_t per = chunk_bytes / (ch_bytes ? ch_bytes : 1);
        if (per < 1) per = 1;
        for (size_t c0 = 0; c0 < nch; c0 += per) {
            const size_t k = per < nch - c0 ? per : nch - c0;
            chunks.push_back({c0 * n, k * n, n, n, k, 0, nf, k * nf * row, c0 * nf * row});
        }
        return chunks;
    }
    // long channels: frame ranges [f0, f1) of one channel -- samples f0 * hop - 1 (history) .. (f1 - 1) * hop + frame_len
    size_t per = (chunk_bytes / sizeof(int16_t)) / f.hop;
    if (per < 1) per = 1;
    for (size_t c = 0; c < nch; ++c)
        for (size_t f0 = 0; f0 < nf; f0 += per) {
            const size_t f1 = nf < f0 + per ? nf : f0 + per, halo = f0 ? 1 : 0;
            const size_t s0 = f0 * f.hop - halo;
            size_t s1 = (f1 - 1) * f.hop + f.frame_len;
            if (s1 > n) s1 = n;                                  // the zero-padded tail of STREAM framing
            chunks.push_back({c * n + s0, s1 - s0, s1 - s0 - halo, s1 - s0, 1, int(halo), f1 - f0, (f1 - f0) * row,
                              (c * nf + f0) * row});
        }
    return chunks;
}

// rows of the largest chunk: what the staging of a chain that runs chunk by chunk holds
inline size_t max_chunk_rows(const std::vector<HostChunk> &chunks) {
    size_t rows = 0;
    for (const HostChunk &c : chunks)
        if (c.nch * c.frames > rows) rows = c.nch * c.frames;
    return rows;
}

// a ragged call: ranges of whole utterances [u0, u1) with rows [rows0, rows1) of the result; a range closes as soon as it
// reaches chunk_bytes
struct UttRange {
    size_t u0, u1, rows0, rows1;
};

inline std::vector<UttRange> cut_ragged(const size_t *off, const size_t *fo, size_t n_utt, size_t chunk_bytes) {
    std::vector<UttRange> ranges;
    size_t u0 = 0;
    for (size_t u = 0; u < n_utt; ++u)
        if (u + 1 == n_utt || (off[u + 1] - off[u0]) * sizeof(int16_t) >= chunk_bytes) {
            ranges.push_back({u0, u + 1, fo[u0], fo[u + 1]});
            u0 = u + 1;
        }
    return ranges;
}

}  // namespace mfcc_batch
