"""Layouts that put the offsets of a call past element 2^31, element 2^32 and byte 2^32 with little work -- TEST
INFRASTRUCTURE ONLY (a plain module: no HIP and no torch at import; tests/test_far_offsets_host.py holds every claim made
here on the CPU, tests/test_gpu_far_inputs.py and tests/test_gpu_far_outputs.py run the cases).

Every buffer under test lives inside one allocation, the arena: ``[guard | used]``.  The call gets the base of the used
region; the guard in front of it is 2^31 elements of the buffer's type, which is everything a 32-bit truncation of a used
offset can reach (:func:`truncations`: signed or unsigned, of the element index or of the byte offset).  A wrong offset
then shows as a wrong bit -- a sentinel that changed, or poison that was read -- not as a fault.

The lines:

* ``e31`` / ``e32``: element (sample or float) index 2^31 / 2^32;
* ``b32``: byte 2^32, that is element ``2^32 / element size``.
"""
from __future__ import annotations

from dataclasses import dataclass, field

E31, E32, B32 = "e31", "e32", "b32"
LINES = (E31, E32, B32)
GUARD = 1 << 31                       # elements of the buffer's type in front of the used region
CAP_BYTES = 48 << 30                  # device memory one case may hold at once
SLACK = 1 << 20                       # elements behind the last line of an arena

POISON_I16 = 0x5A5B                   # every byte, half word and word of an input guard: not zero, not a real sample run
SENTINEL = -7.0                       # every float a call must not touch (the suite's value)
SENTINEL_I16 = -7


def line_index(line, esize):
    """Element index of a line in a buffer of ``esize``-byte elements."""
    return {E31: 1 << 31, E32: 1 << 32, B32: (1 << 32) // esize}[line]


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def truncations(off, esize):
    """Where element offset ``off`` lands, in elements from the same base, when 32 bits of it survive: the element index
    unsigned and signed, the byte offset unsigned and signed."""
    b = off * esize
    return {off & 0xFFFFFFFF, _s32(off), (b & 0xFFFFFFFF) // esize, _s32(b) // esize}


@dataclass(frozen=True)
class Span:
    """One channel, utterance or segment: ``count`` elements from element ``start`` of the used region."""
    start: int
    count: int

    @property
    def end(self):
        return self.start + self.count

    def straddles(self, idx):
        return self.start < idx < self.end - 1


@dataclass(frozen=True)
class Layout:
    """A case's buffer: element size, elements of the used region, the spans the call touches, the lines it claims."""
    esize: int
    used: int
    spans: tuple
    lines: tuple
    guard: int = GUARD

    @property
    def arena_bytes(self):
        return (self.guard + self.used) * self.esize

    def crossed(self):
        """The lines some span straddles."""
        return tuple(l for l in LINES if any(s.straddles(line_index(l, self.esize)) for s in self.spans))

    def probe_offsets(self):
        """Used offsets whose truncations bound every other one's: both ends of every span and both sides of every line
        inside it (a truncation is monotone between those)."""
        out = set()
        for s in self.spans:
            out |= {s.start, s.end - 1}
            for l in LINES:
                i = line_index(l, self.esize)
                for k in (1 << 31, 1 << 32, i):
                    out |= {v for v in (k - 1, k) if s.start <= v < s.end}
        return sorted(out)

    def truncations_inside(self):
        return all(-self.guard <= t < self.used for o in self.probe_offsets() for t in truncations(o, self.esize))


# ------------------------------------------------------------------------------------------------ dense inputs
def dense_input(n, esize):
    """Channels of ``n`` elements on one odd stride: channel 0 at element 5, the next ones straddling the lines.  For
    1- and 2-byte samples the stride is just under 2^31: channel 1 straddles e31 (b32 too at 2 bytes), channel 2 e32 (b32
    at 1 byte), channel 3 lies wholly beyond 2^32.  For 4-byte samples it is just under 2^30: channel 1 straddles b32,
    channel 2 e31.  Returns ``(stride, Layout)``."""
    unit, nch = ((1 << 30), 3) if esize == 4 else ((1 << 31), 4)
    delta = (n // 5) | 1                 # a fifth, two fifths of the straddlers in front of their lines: tiles start beyond
    stride = unit - delta
    spans = tuple(Span(5 + c * stride, n) for c in range(nch))
    lines = {1: (E31, E32, B32), 2: (E31, E32, B32), 4: (E31, B32)}[esize]
    return stride, Layout(esize, spans[-1].end + 16, spans, lines)


def ragged_input(lens, straddler=0):
    """Utterances back to back in an int16 buffer, ``offsets[0]`` just under 2^32 so that utterance ``straddler`` straddles
    sample 2^32 and the ones behind it lie wholly beyond.  Returns ``(offsets, Layout)``."""
    before = sum(lens[:straddler])
    off0 = (1 << 32) - before - lens[straddler] // 2
    offs = [off0]
    for v in lens:
        offs.append(offs[-1] + v)
    spans = tuple(Span(a, b - a) for a, b in zip(offs[:-1], offs[1:]))
    return offs, Layout(2, offs[-1] + 16, spans, (E32,))


INPUT_ARENA_WORDS = (1 << 32) + SLACK          # 4-byte words: 2^31 guard + 2^31 used of them, 2^31 + 3 * 2^31 int16


DENSE_FRAMES = 37                              # three tiles of 16 frames, the last one partial

# what runs on the dense input layout besides the rows of kernel_families.ALL: id -> (frame length, hop, sample bytes)
INPUT_EXTRA = {
    "512_w12": (512, 170, 2), "512_w4": (512, 170, 2), "512_h160": (400, 160, 2), "512_h160_mb": (400, 160, 2),
    "1024_w12bf": (1024, 341, 2), "1024_w12": (1024, 341, 2), "1024_f32": (1024, 341, 2), "1024_bf16": (1024, 341, 2),
    "spectrum512_h170": (512, 170, 2), "spectrum512_h160": (400, 160, 2), "spectrum_generic": (200, 80, 2),
    "fbank512_f32_htk80": (512, 170, 2), "fbank512_mfma_dense128": (400, 160, 2), "fbank_generic": (200, 80, 2),
    "fmt_s16": (512, 170, 2), "fmt_ulaw": (512, 170, 1), "fmt_alaw": (512, 170, 1), "fmt_u8": (512, 170, 1),
    "fmt_i2s32": (512, 170, 4), "fmt_s32": (512, 170, 4), "fmt_f32": (512, 170, 4),
    "rate_8000": (256, 85, 2),                 # 8 kHz samples: half of a 512 / 170 frame at 16 kHz
}


def dense_input_shapes():
    """id -> (samples of a channel, sample bytes) of every dense input case."""
    import kernel_families as kf
    out = {f.id: (f.nfft + (DENSE_FRAMES - 1) * f.hop, 2) for f in kf.ALL}
    out.update({k: (L + (DENSE_FRAMES - 1) * hop, es) for k, (L, hop, es) in INPUT_EXTRA.items()})
    return out


RAGGED_ROUTES = ("f512", "x512", "g256", "x256_16", "f1024")


def ragged_lens(nfft, hop):
    """The ``offset0`` corpus of tests/test_gpu_ragged_routes.py."""
    return [nfft + hop + 3, nfft - 1, 16 * hop + nfft]


def uniform_lens(nfft, hop):
    return [nfft + 3 * hop] * 3


# ------------------------------------------------------------------------------------------------ segment passes
SEG_ROWS = (300, 129, 37)             # the corpus lengths of tests/test_gpu_post_chain.py
# Which segment straddles the line.  Never the last one: a pass adds a tile's first row times the width to its base
# pointer and walks the tile from there, so a truncated product shows only in a tile that STARTS beyond the line -- with
# the last segment across the line every tile of the call starts in front of it (a mutant of kernel_normalize.hpp's
# ``row0 * W`` passed that layout).
SEG_STRADDLER = {B32: 1, E31: 0, E32: 1}


def segments(line, width, esize=4, out_width=None):
    """Three consecutive segments of SEG_ROWS rows of ``width`` elements, placed so that segment ``SEG_STRADDLER[line]``
    straddles the line (``out_width``: the line is met in a second buffer of that row width instead, as ``deltas_rows``'
    ``out=``).  Returns ``(row offsets, Layout of the buffer that meets the line)``."""
    w = out_width or width
    k = SEG_STRADDLER[line]
    row_of_line = line_index(line, esize) // w
    r0 = row_of_line - sum(SEG_ROWS[:k]) - SEG_ROWS[k] // 2
    fo = [r0]
    for v in SEG_ROWS:
        fo.append(fo[-1] + v)
    spans = tuple(Span(a * w, (b - a) * w) for a, b in zip(fo[:-1], fo[1:]))
    return fo, Layout(esize, (fo[-1] + 8) * w, spans, (line,))


SEG_PASSES = ("normalize", "normalize_sliding", "pcen", "deltas", "deltas_out", "vad", "select", "gate")
SEG_WIDTH = 13
SEG_SHIFT_ROWS = 1000                 # normalize_sliding: ``out`` is the same arena, this many rows further on
# deltas_rows writes rows (1 + order) times as wide at the same row index.  "deltas": order 1, the INPUT meets the line and
# the output lies at twice the offset; "deltas_out": order 2, the OUTPUT meets the line.  An input across float 2^32 would
# put its output past float 2^33: 43 GB of arena with the guard, which no case can hold beside its input under the cap.
SEG_CASES = [(p, l) for p in SEG_PASSES for l in (B32, E31, E32) if (p, l) != ("deltas", E32)]


def _row_layout(fo, width, esize, lines, shift_rows=0):
    spans = tuple(Span((a + shift_rows) * width, (b - a) * width) for a, b in zip(fo[:-1], fo[1:]))
    return Layout(esize, (fo[-1] + shift_rows + 8) * width, spans, lines)


def segment_case(name, line):
    """``(row offsets, [Layout of every range of the arena the call touches])`` of a pass at a line; the first layout is
    the one that meets the line."""
    w = SEG_WIDTH
    if name == "deltas_out":
        fo, lay = segments(line, w, out_width=3 * w)
        return fo, [lay, _row_layout(fo, w, 4, ())]
    fo, lay = segments(line, w, 2 if name == "gate" else 4)
    if name == "deltas":
        return fo, [lay, _row_layout(fo, 2 * w, 4, ())]
    if name == "normalize_sliding":
        return fo, [lay, _row_layout(fo, w, 4, (), SEG_SHIFT_ROWS)]
    return fo, [lay]
OUTPUT_ARENA_FLOATS = (1 << 32) + 2 * SLACK    # the used floats of the output arena; 2^31 guard floats in front
OUTPUT_ARENA_BYTES = 4 * (GUARD + OUTPUT_ARENA_FLOATS)


# ------------------------------------------------------------------------------------------------ dense outputs
@dataclass(frozen=True)
class OutCase:
    """A frame kernel whose dense output crosses ``lines``: ``nch`` channels of ``q``-hop periods, ``width`` elements a
    row.  ``entry``: "process", "fixed", "spectrum" or "fbank"; ``kw``: the MFCC arguments; ``bank``: the filterbank
    matrix by name; ``ref``: which reference holds one period."""
    id: str
    kernel: str
    entry: str
    kw: dict
    width: int
    hop: int
    flen: int
    lines: tuple
    nch: int = 4
    q: int = 33
    env: dict = field(default_factory=dict)
    bank: str = ""
    esize: int = 4

    @property
    def rows_per_channel(self):
        top = max(line_index(l, self.esize) for l in self.lines)
        return -(-(top + SLACK // 2) // (self.width * self.nch))

    @property
    def samples(self):
        return self.flen + (self.rows_per_channel - 1) * self.hop

    def layout(self):
        per = self.rows_per_channel * self.width
        spans = tuple(Span(c * per, per) for c in range(self.nch))
        return Layout(self.esize, self.nch * per + SLACK // 2, spans, self.lines)

    def input_layout(self):
        """The samples: channels back to back, so sample offsets pass the lines as well."""
        spans = tuple(Span(c * self.samples, self.samples) for c in range(self.nch))
        return Layout(2, self.nch * self.samples, spans, (), GUARD if self.guard_input else 0)

    @property
    def guard_input(self):
        """Whether the samples get a poison guard of their own in front (2^31 int16): wherever the cap leaves room for
        it.  Without one a truncated sample offset could read in front of the allocation."""
        return self._bytes(2 * GUARD) <= CAP_BYTES

    def _bytes(self, input_guard):
        return OUTPUT_ARENA_BYTES + input_guard + 2 * self.nch * self.samples + (1 << 28)

    def live_bytes(self):
        """The module's output arena, the input with its guard and the compact comparison call."""
        return self._bytes(2 * GUARD if self.guard_input else 0)


_S512 = dict(nfft=512, hop=170, nfilters=8, nceptrums=8, power_scale=512.0)
_S1024 = dict(nfft=1024, hop=341, nfilters=8, nceptrums=8, power_scale=1024.0)
_S256 = dict(nfft=256, hop=80, win_length=200, nfilters=8, nceptrums=8, power_scale=256.0)
_K512 = dict(nfft=512, nfilters=32, nceptrums=32)
_K1024 = dict(nfft=1024, nfilters=40, nceptrums=40, power_scale=0)
_FRAMED = dict(nfft=512, hop=160, win_length=400, nfilters=32, nceptrums=32)
_HTK64 = dict(nfft=512, hop=160, win_length=400, nfilters=64, nceptrums=13, mel="htk", fmin=0, fmax=8000, output="logmel")
_G1024 = dict(nfft=1024, nfilters=64, nceptrums=32, power_scale=0, output="logmel")
_ALL3 = (B32, E31, E32)
_W4, _F1024 = "MFCC_HIP_FUSED512", "MFCC_HIP_FUSED1024"

# the widest row each family takes: 32 cepstra or 32 log-mel bands at 512, 64 bands on the matrix-driven hop-160 form and
# on the generic kernel, 40 cepstra at 1024 (only its default form has a log-mel tail, the four-wave 512 form has none)
OUT_CASES = [
    OutCase("spectrum512", "mfcc_spectrum512_kernel", "spectrum", _S512, 257, 170, 512, _ALL3),
    OutCase("spectrum_generic_1024", "mfcc_spectrum_generic_kernel", "spectrum", _S1024, 513, 341, 1024, _ALL3),
    OutCase("fbank512_f32_htk128", "mfcc_fbank512_kernel", "fbank", _S512, 128, 170, 512, _ALL3, bank="htk128"),
    OutCase("fbank512_mfma_dense128", "mfcc_fbank512_kernel", "fbank", _S512, 128, 170, 512, _ALL3, bank="dense128"),
    OutCase("fbank_generic_dense128", "mfcc_fbank_generic_kernel", "fbank", _S256, 128, 80, 200, _ALL3, bank="dense128"),
    OutCase("512_w12_cepstra32", "mfcc_fused512_w12_kernel", "process", _K512, 32, 170, 512, (B32,)),
    OutCase("512_w12_logmel32", "mfcc_fused512_w12_kernel", "process", dict(_K512, output="logmel"), 32, 170, 512, (B32,)),
    OutCase("512_w4_cepstra32", "mfcc_fused512_kernel", "process", _K512, 32, 170, 512, (B32,), env={_W4: "w4"}),
    OutCase("512_h160_cepstra32", "mfcc_fused512_h160_kernel", "process", _FRAMED, 32, 160, 400, (B32,)),
    OutCase("512_h160_logmel32", "mfcc_fused512_h160_kernel", "process", dict(_FRAMED, output="logmel"), 32, 160, 400,
            (B32,)),
    OutCase("512_h160_mb_logmel64", "mfcc_fused512_h160_mb_kernel", "process", _HTK64, 64, 160, 400, (B32,)),
    OutCase("1024_w12bf_cepstra40", "mfcc_fused1024_w12bf_kernel", "process", _K1024, 40, 341, 1024, (B32,)),
    OutCase("1024_w12bf_logmel40", "mfcc_fused1024_w12bf_kernel", "process", dict(_K1024, output="logmel"), 40, 341, 1024,
            (B32,)),
    OutCase("1024_w12_cepstra40", "mfcc_fused1024_w12_kernel", "process", _K1024, 40, 341, 1024, (B32,),
            env={_F1024: "w12"}),
    OutCase("1024_f32_cepstra40", "mfcc_fused1024_kernel", "process", _K1024, 40, 341, 1024, (B32,), env={_F1024: "f32"}),
    OutCase("1024_bf16_cepstra40", "mfcc_fused1024_kernel", "process", _K1024, 40, 341, 1024, (B32,),
            env={_F1024: "bf16"}),
    OutCase("generic_1024_logmel64", "mfcc_float_generic_kernel", "process", _G1024, 64, 341, 1024, (B32,)),
    OutCase("fixed512_cepstra32", "mfcc_fixed512_kernel", "fixed", _K512, 32, 170, 512, (B32,), esize=2),
]
OUT_IDS = [c.id for c in OUT_CASES]


# ------------------------------------------------------------------------------------------------ one ragged result
# process_packed on the tile-record route (512 / 170 / 32, log-mel rows of 32 floats): PACKED_UTTS utterances of
# PACKED_Q-hop periods, utterance u 997 (u mod 5) samples short of PACKED_SAMPLES, so that the rows pass byte 2^32
PACKED_KW = dict(nfft=512, nfilters=32, nceptrums=13, output="logmel")
PACKED_KERNEL, PACKED_WIDTH, PACKED_Q = "mfcc_fused512_w12_kernel", 32, 33
PACKED_UTTS, PACKED_SAMPLES = 20_000, 290_000
PACKED_SAMPLED = (0, 1, 2, 9_999, 10_000, 15_553, 19_998, 19_999)


def packed_lens():
    return [PACKED_SAMPLES - 997 * (u % 5) for u in range(PACKED_UTTS)]


def packed_layout(frames_of):
    """The result of the ragged call: one span per utterance, ``frames_of(samples)`` rows of PACKED_WIDTH floats each."""
    per = {v: frames_of(v) for v in set(packed_lens())}
    spans, at = [], 0
    for v in packed_lens():
        spans.append(Span(at, per[v] * PACKED_WIDTH))
        at += per[v] * PACKED_WIDTH
    return Layout(4, at + SLACK // 2, tuple(spans), (B32,))


# ------------------------------------------------------------------------------------------------ the host route
# one int16 channel of just over 2^31 periodic samples through the host entry of process (512 / 170 / 32 / 13): frame-range
# chunks at the default chunk size, so a chunk's sample offset and its first output row pass the line
HOST_KW = dict(nfft=512, nfilters=32, nceptrums=13)
HOST_CHUNK_SAMPLES = (64 << 20) // 2             # mfcc_hip.hip: host_chunk_bytes
HOST_SAMPLES = (1 << 31) + 3 * HOST_CHUNK_SAMPLES + 1235
HOST_Q = 33


# ------------------------------------------------------------------------------------------------ what is not reached
# (kernel or route, line or "all", reason).  The first three are out of scope by the design of the library; the rest is
# what this table does not build yet, each with its reason.
NOT_REACHED = [
    ("launch_geom and ragged records: 32-bit tile arithmetic", "all",
     "2^31 tiles or channels, 2^26 tiles per channel, 2^31 samples per utterance: no corpus reaches them on one card; "
     "tests/test_launch_geom_host.py and tests/test_batch_plan_host.py hold them at lowered limits"),
    ("fixed-point outputs", E31 + "+", "past 2^31 int16 elements the input alone passes the memory cap"),
    ("generic fixed kernels, 1024 families at 13 coefficients: outputs", B32,
     "the input alone would pass the 48 GiB cap"),
    ("sessions, stream banks, live resampler, power gate object", "all", "bounded state per line"),
    ("deltas_rows: input rows", E32,
     "memory cap: the expanded rows lie at (1 + order) times the offset, past float 2^33 -- 43 GB of arena with its guard, "
     "beside the inputs of the module's other cases; the input crosses b32 and e31, the output all three lines"),
]


# ------------------------------------------------------------------------------------------------ device helpers
def fill_periodic(dst, period):
    """``dst`` (a 1-D device tensor: a channel) = ``period`` repeated and cut at its length; ``period``: a 1-D device
    tensor of ``q`` hops, ``q`` odd, so that no power-of-two wrap distance is a multiple of it (config 4 of
    tests/test_gpu_full_size.py builds its channels this way)."""
    p = period.numel()
    full = dst.numel() // p
    dst[:full * p].view(full, p)[:] = period
    dst[full * p:] = period[:dst.numel() - full * p]


def chunks(t, step=1 << 28):
    """Flat views of a contiguous tensor, ``step`` elements each: every device reduction here stays below 2^31 elements."""
    flat = t.reshape(-1)
    for a in range(0, flat.numel(), step):
        yield flat[a:a + step]


def fill(t, value):
    for c in chunks(t):
        c.fill_(value)


def all_equal_to(t, value):
    """Every element of ``t`` equals ``value``, compared on the device."""
    return all(bool((c == value).all()) for c in chunks(t))


def dev_equal(a, b):
    """Bit for bit on the device, NaN patterns included (the tensors are compared as integers)."""
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    a, b = a.contiguous().view(it), b.contiguous().view(it)
    return all(torch.equal(x, y) for x, y in zip(chunks(a), chunks(b)))
