"""The table of tests/far_offsets.py, held on the CPU: every case crosses the lines it claims with a span that straddles
them, channels do not overlap, every 32-bit truncation of a used offset stays inside the case's own arena, no case holds
more than 48 GiB, and what the table does not reach is exactly the pinned list below.  This is the not-blind condition of
tests/test_gpu_far_inputs.py and tests/test_gpu_far_outputs.py: a case that silently stops crossing its line fails here."""
import far_offsets as fo
import kernel_families as kf
from far_offsets import B32, E31, E32


def _holds(layout, what):
    assert set(layout.lines) <= set(layout.crossed()), (what, layout.lines, layout.crossed())
    for line in layout.lines:                                # a span straddles it: starts before, ends behind it
        i = fo.line_index(line, layout.esize)
        assert any(s.start < i and s.end > i + 1 for s in layout.spans), (what, line)
    spans = sorted(layout.spans, key=lambda s: s.start)
    assert all(a.end <= b.start for a, b in zip(spans, spans[1:])), what
    assert all(0 <= s.start and s.end <= layout.used for s in spans), what
    assert layout.guard == 1 << 31 and layout.truncations_inside(), what
    assert layout.arena_bytes <= fo.CAP_BYTES, what


def test_truncations_cover_signed_and_unsigned_elements_and_bytes():
    assert fo.truncations((1 << 32) + 5, 2) == {5}
    assert fo.truncations((1 << 31) + 5, 2) == {(1 << 31) + 5, -(1 << 31) + 5, 5}
    assert fo.truncations((1 << 30) + 5, 4) == {(1 << 30) + 5, 5}
    assert fo.truncations((1 << 31) - 1, 4) == {(1 << 31) - 1, (1 << 30) - 1, -1}
    assert min(min(fo.truncations(o, es)) for es in (1, 2, 4) for o in (1 << 31, (1 << 32) - 1, 3 << 31)) == -(1 << 31)
    assert fo.line_index(B32, 4) == 1 << 30 and fo.line_index(B32, 2) == 1 << 31 and fo.line_index(B32, 1) == 1 << 32


def test_dense_input_cases():
    shapes = fo.dense_input_shapes()
    assert set(kf.IDS) <= set(shapes) and len(shapes) == len(kf.IDS) + len(fo.INPUT_EXTRA)
    for name, (n, esize) in shapes.items():
        stride, lay = fo.dense_input(n, esize)
        _holds(lay, name)
        assert stride % 2 == 1 and stride >= n, name         # odd, and the library demands stride >= n
        assert [b.start - a.start for a, b in zip(lay.spans, lay.spans[1:])] == [stride] * (len(lay.spans) - 1)
        assert lay.spans[0].end < 1 << 20                    # one channel near the base
        for line in lay.lines:                               # most of the straddler, so its later tiles, lies beyond
            i = fo.line_index(line, esize)
            assert any(s.straddles(i) and i - s.start < n // 2 for s in lay.spans), (name, line)
        if esize != 4:
            assert lay.spans[3].start > 1 << 32              # one wholly beyond 2^32
        assert (lay.guard + lay.used) * esize <= 4 * fo.INPUT_ARENA_WORDS, name
        assert set(lay.lines) == ({E31, B32} if esize == 4 else {E31, E32, B32})
    # all seven sample formats, each of the three sample sizes
    assert sorted(es for k, (_, _, es) in fo.INPUT_EXTRA.items() if k.startswith("fmt_")) == [1, 1, 1, 2, 4, 4, 4]


def test_ragged_input_cases():
    fams = {f.id: f for f in kf.ALL}
    for fid in fo.RAGGED_ROUTES:
        f = fams[fid]
        for lens in (fo.ragged_lens(f.nfft, f.hop), fo.uniform_lens(f.nfft, f.hop)):
            offs, lay = fo.ragged_input(lens)
            _holds(lay, fid)
            assert (1 << 32) - max(lens) < offs[0] < 1 << 32 and lay.crossed() == (E32,)
            assert [b - a for a, b in zip(offs, offs[1:])] == lens
            assert (lay.guard + lay.used) * 2 <= 4 * fo.INPUT_ARENA_WORDS


def test_segment_cases():
    assert fo.SEG_ROWS == (300, 129, 37) and set(fo.SEG_STRADDLER) == set(fo.LINES)
    assert max(fo.SEG_STRADDLER.values()) < len(fo.SEG_ROWS) - 1      # a segment, so a tile, starts beyond every line
    for line in fo.LINES:
        for width, esize, out_width in ((13, 4, None), (32, 4, None), (13, 4, 39), (13, 2, None)):
            offs, lay = fo.segments(line, width, esize, out_width)
            _holds(lay, (line, width, esize, out_width))
            w = out_width or width
            k = fo.SEG_STRADDLER[line]
            assert lay.spans[k].straddles(fo.line_index(line, esize)) and line in lay.crossed()
            assert len(lay.crossed()) == (2 if esize == 2 and line != E32 else 1)          # int16: e31 is b32
            assert tuple(b - a for a, b in zip(offs, offs[1:])) == fo.SEG_ROWS
            assert lay.used <= (fo.OUTPUT_ARENA_FLOATS if esize == 4 else 2 * fo.OUTPUT_ARENA_FLOATS), (line, w)
    # every pass at every line but the one the memory cap drops; what a call reads and writes lies apart, inside the arena
    assert len(fo.SEG_CASES) == 3 * len(fo.SEG_PASSES) - 1 and ("deltas", E32) not in fo.SEG_CASES
    assert {p for p, _ in fo.SEG_CASES} == set(fo.SEG_PASSES)
    for name, line in fo.SEG_CASES:
        offs, lays = fo.segment_case(name, line)
        assert line in lays[0].lines and line in lays[0].crossed(), (name, line)
        assert any(s.start > fo.line_index(line, lays[0].esize) for s in lays[0].spans), (name, line)
        for lay in lays:
            _holds(lay, (name, line))
            assert lay.used <= fo.OUTPUT_ARENA_FLOATS * (4 // lay.esize), (name, line)
        if len(lays) == 2:
            a, b = sorted(lays, key=lambda l: l.spans[0].start)
            assert a.spans[-1].end < b.spans[0].start, (name, line)
    # the arena: 2^31 guard floats and the used ones, under the cap with the compact copies beside it
    assert 4 * ((1 << 31) + fo.OUTPUT_ARENA_FLOATS) + (1 << 30) <= fo.CAP_BYTES


def test_dense_output_cases():
    assert len(set(fo.OUT_IDS)) == len(fo.OUT_CASES)
    for c in fo.OUT_CASES:
        lay = c.layout()
        _holds(lay, c.id)
        assert c.nch > 1 and c.q % 2 == 1 and c.rows_per_channel > 4 * c.q, c.id
        assert lay.used <= fo.OUTPUT_ARENA_FLOATS * (4 // c.esize), c.id
        assert c.live_bytes() <= fo.CAP_BYTES, (c.id, c.live_bytes() / 2.0 ** 30)
        # the samples: behind a guard of their own no truncated sample offset leaves the allocation either
        ilay = c.input_layout()
        assert not c.guard_input or (ilay.guard == 1 << 31 and ilay.truncations_inside()), c.id
        for k in (1 << 30, 1 << 31, 1 << 32):                # no wrap distance is a multiple of the period
            assert k % (c.q * c.width) and k % (c.q * c.hop), c.id
    # only the fixed-point case has no room for that guard under the cap: its samples alone are 22.8 GB
    assert [c.id for c in fo.OUT_CASES if not c.guard_input] == ["fixed512_cepstra32"]
    by_kernel = {}
    for c in fo.OUT_CASES:
        by_kernel.setdefault(c.kernel, set()).update(c.lines)
    for k in ("mfcc_spectrum512_kernel", "mfcc_spectrum_generic_kernel", "mfcc_fbank512_kernel", "mfcc_fbank_generic_kernel"):
        assert by_kernel[k] == {B32, E31, E32}, k
    for k in ("mfcc_fused512_w12_kernel", "mfcc_fused512_kernel", "mfcc_fixed512_kernel"):
        assert B32 in by_kernel[k], k
    assert {c.bank for c in fo.OUT_CASES if c.kernel == "mfcc_fbank512_kernel"} == {"htk128", "dense128"}
    assert next(c for c in fo.OUT_CASES if c.kernel == "mfcc_spectrum_generic_kernel").width == 513


def test_packed_result_and_host_route_cases():
    lens = fo.packed_lens()
    assert len(lens) == fo.PACKED_UTTS and len(set(lens)) == 5 and max(fo.PACKED_SAMPLED) == fo.PACKED_UTTS - 1
    lay = fo.packed_layout(lambda n: (n - 512) // 170 + 1)
    _holds(lay, "packed")
    assert all(s.count > 4 * fo.PACKED_Q * fo.PACKED_WIDTH for s in lay.spans)       # periods to compare inside each
    assert lay.used <= fo.OUTPUT_ARENA_FLOATS
    assert fo.OUTPUT_ARENA_BYTES + 2 * (fo.GUARD + sum(lens)) + (1 << 28) <= fo.CAP_BYTES       # samples behind a guard
    assert any(s.start > 1 << 30 for s in (lay.spans[u] for u in fo.PACKED_SAMPLED))  # a sampled one beyond the line
    assert any(s.start < 1 << 30 for s in (lay.spans[u] for u in fo.PACKED_SAMPLED))
    # the host route: whole chunks start beyond sample 2^31, and the channel ends inside one
    assert fo.HOST_SAMPLES - 2 * fo.HOST_CHUNK_SAMPLES > 1 << 31 and fo.HOST_SAMPLES % fo.HOST_CHUNK_SAMPLES
    assert (1 << 31) % (fo.HOST_Q * 170) and fo.HOST_Q % 2 == 1
    assert 2 * 2 * fo.HOST_SAMPLES <= fo.CAP_BYTES


PINNED_NOT_REACHED = [
    # out of scope by design
    ("launch_geom and ragged records: 32-bit tile arithmetic", "all"),
    ("fixed-point outputs", "e31+"),
    ("generic fixed kernels, 1024 families at 13 coefficients: outputs", B32),
    ("sessions, stream banks, live resampler, power gate object", "all"),
    # dropped for the memory cap
    ("deltas_rows: input rows", E32),
]


def test_what_is_not_reached_is_pinned():
    assert [(k, line) for k, line, _ in fo.NOT_REACHED] == PINNED_NOT_REACHED
    assert all(len(reason) > 10 for _, _, reason in fo.NOT_REACHED)
    # nothing is both listed and built
    built = {c.kernel for c in fo.OUT_CASES}
    assert not [k for k, _ in PINNED_NOT_REACHED if k.split(":")[0] in built]
