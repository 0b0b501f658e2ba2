"""The fixed-point kernels at the loud end of their integer range (tests/fixed_stimuli.py: what the stimuli reach is
asserted on the oracle alone by tests/test_fixed_reach_host.py), bit for bit against the RTL oracle.

G1  every fixed family, both framings, all stimuli as channels of one strided device call, 1 .. 9 frames, n_cep 1 and all;
G2  the fused 512 kernel's filterbank reduction at the other sample rates;
G3  the same rows from every fixed entry point: host array, ragged batch, stream session, stream bank;
G4  the receiver's gate on real rows loud enough for its 32-bit sum to wrap.

Everything is integer arithmetic: every comparison is ``array_equal``."""
import numpy as np
import pytest

import fixed_stimuli as fs
import gate_ref as gr
import kernel_families as kf
from kernel_families import as_np
from oracle import mfcc_fixed as mx

pytestmark = pytest.mark.gpu
PADS = ["notebook", "stream"]
FRAMES = (1, 2, 3, 4, 5, 9)
FIXED_IDS = [f.id for f in kf.FIXED]


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()             # a copy: the shared stimuli are read-only


_STACK = {}


def stimuli(n, nfft):
    """All stimuli as channels (len(fs.NAMES), n), made once per length and left unchanged."""
    if (n, nfft) not in _STACK:
        a = fs.stack(n, nfft)
        a.setflags(write=False)
        _STACK[n, nfft] = a
    return _STACK[n, nfft]


def differ(tag, got, ref):
    """Raises with the first differing (channel, frame, coefficient)."""
    got = as_np(got)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.int16, (tag, got.shape, ref.shape, got.dtype)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        where = tuple(int(v) for v in bad[0])
        name = fs.NAMES[where[0]] if got.ndim == 3 and got.shape[0] == len(fs.NAMES) else ""
        raise AssertionError("%s: %d value(s) differ from the RTL oracle, first at %s %s: got %d, oracle %d"
                             % (tag, len(bad), where, name, got[where], ref[where]))


# ------------------------------------------------------------------------------------------------ G1

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", kf.FIXED, ids=FIXED_IDS)
def test_g1_every_family_on_all_stimuli(mfcc_amd, fam, pad):
    """The fused kernel runs log2 + DCT once per two (32 filters) or four (16 filters) frames: 1, 2, 3, 4, 5 and 9 frames
    leave every residue partly filled.  An odd channel stride from an odd base offset, as E1 does."""
    import torch
    nch = len(fs.NAMES)
    full = kf.Family(fam.id, True, fam.kernel, fam.nfft, fam.nfilters, fam.nfilters, fam.samplerate)
    refs = {}
    for ncep in (1, fam.nfilters):
        with kf.open_handle(mfcc_amd, fam, pad, nceptrums=ncep) as m:
            assert m.kernel_name(fixed=True) == fam.kernel
            for i, nfr in enumerate(FRAMES):
                n = fs.n_samples(fam.nfft, nfr, pad)
                pcm = stimuli(n, fam.nfft)
                if nfr not in refs:
                    refs[nfr] = np.stack([kf.fixed_ref(full, c, pad) for c in pcm])
                ref = np.ascontiguousarray(refs[nfr][:, :, :ncep])
                off = 2 * i + 1
                stride = n + 2 * i + 3
                stride += 1 - stride % 2
                flat = np.zeros(off + stride * nch + 8, np.int16)
                for c in range(nch):
                    flat[off + c * stride: off + c * stride + n] = pcm[c]
                view = torch.as_strided(_dev(flat), (nch, n), (stride, 1), storage_offset=off)
                got = m.process_fixed(view)
                assert tuple(got.shape) == (nch, nfr, ncep) and m.num_frames(n) == nfr
                differ("%s %s %d frames n_cep %d" % (fam.id, pad, nfr, ncep), got, ref)


# ------------------------------------------------------------------------------------------------ G2

RATES = [(r, 32) for r in (8000, 11025, 22050, 32000, 44100, 48000)] + [(r, 16) for r in (8000, 22050, 48000)]


def test_g2_fused_kernel_other_sample_rates(mfcc_amd):
    """The piece size and the lane count of mfcc_fixed512_kernel's segmented reduction follow the filter widths, i.e.
    the rate: the carries of the loud power values through every such layout, or -105 where the oracle's filterbank
    asserts -- the rates and filter counts of test_fixed_fused_kernel_other_sample_rates."""
    pcm = stimuli(fs.n_samples(512, 9, "stream"), 512)
    ran = 0
    for sr, nfil in RATES:
        with mfcc_amd.MFCC(nfft=512, nfilters=nfil, nceptrums=nfil, samplerate=sr, pad_mode="stream") as m:
            try:
                ref = mx.mfcc_fixed_ref(pcm, nfilters=nfil, nceptrums=nfil, sample_rate=float(sr))
            except AssertionError:
                with pytest.raises(mfcc_amd.MfccHipError) as e:
                    m.process_fixed(_dev(pcm))
                assert e.value.code == -105, sr
                continue
            assert m.kernel_name(fixed=True) == "mfcc_fixed512_kernel", (sr, nfil)
            differ("%d Hz %d filters" % (sr, nfil), m.process_fixed(_dev(pcm)), ref)
            ran += 1
    assert ran >= 6


# ------------------------------------------------------------------------------------------------ G3

G3_FAMS = [f for f in kf.FIXED if f.id in ("x512", "x512_16f", "x1024_64")]
G3_STIMULI = ("square_b123h", "loud_silent")         # loud where the filterbank shows it, and loud beside silent frames
CHUNKS = (1, 169, 170, 171, 1000)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("fam", G3_FAMS, ids=[f.id for f in G3_FAMS])
def test_g3_every_entry_point_gives_the_same_rows(mfcc_amd, fam, pad):
    import torch
    nfft, hop = fam.nfft, fam.hop
    lens = [fs.n_samples(nfft, k, pad) for k in (1, 2, 5, 9)] + [nfft // 2]
    with kf.open_handle(mfcc_amd, fam, pad) as m:
        frames = [m.num_frames(v) for v in lens]
        assert frames[:4] == [1, 2, 5, 9]                              # the too-short one: no row, or STREAM's padded one
        for name in G3_STIMULI:
            utts = [fs.STIMULI[name](v, nfft) for v in lens]
            refs = [kf.fixed_ref(fam, u, pad) for u in utts]
            one = [as_np(m.process_fixed(_dev(u))) for u in utts]      # the per-utterance call
            for i, (o, r) in enumerate(zip(one, refs)):
                differ("%s %s %s utterance %d" % (fam.id, pad, name, i), o, r)
            # host array
            for i, u in enumerate(utts):
                differ("%s %s %s host %d" % (fam.id, pad, name, i), m.process_fixed(u), refs[i])
            # ragged batch in one flat device buffer
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            packed, fo = m.process_packed(_dev(np.concatenate(utts)), offs, fixed=True)
            torch.cuda.synchronize()
            assert [int(v) for v in np.diff(fo.astype(np.int64))] == frames
            for i, r in enumerate(refs):
                differ("%s %s %s packed %d" % (fam.id, pad, name, i), packed[int(fo[i]):int(fo[i + 1])], r)
            # a stream session, one pass per chunk size
            x, R = utts[3], refs[3]
            with m.stream(fixed=True) as s:
                for c in CHUNKS:
                    rows = [s.push(x[a:a + c]) for a in range(0, len(x), c)] + [s.flush()]
                    differ("%s %s %s session in chunks of %d" % (fam.id, pad, name, c), np.concatenate(rows), R)
                    assert s.pending == 0
            # a stream bank: one line per utterance, every line on another chunk size in every round
            with m.stream_bank(len(utts), fixed=True) as bank:
                pos = [0] * len(utts)
                got = [[] for _ in utts]
                k = 0
                while any(p < len(u) for p, u in zip(pos, utts)):
                    sizes = [CHUNKS[(k + i) % len(CHUNKS)] for i in range(len(utts))]
                    chunks = [u[p:p + c] for u, p, c in zip(utts, pos, sizes)]
                    for i, rows in enumerate(bank.push(chunks)):
                        got[i].append(rows.copy())
                    pos = [p + len(c) for p, c in zip(pos, chunks)]
                    k += 1
                for i, rows in enumerate(bank.flush()):
                    got[i].append(rows.copy())
            for i, r in enumerate(refs):
                differ("%s %s %s bank line %d" % (fam.id, pad, name, i), np.concatenate(got[i]), r)


# ------------------------------------------------------------------------------------------------ G4

def test_g4_gate_on_real_loud_rows(mfcc_amd, wav_pcm):
    """512 / 16 / 16: full-scale noise on the pre-emphasised side gives c0 of 13 661 .. 15 622, and the sum of c0^2 over
    the middle 31 of 93 rows is 2^32.68 (the oracle's figures): above the threshold, and negative as the 32-bit sum
    that software/cepstrum.c:161-183 keeps.  So ``gate`` and ``gate_ref`` differ on rows a kernel produced.  A speech
    line and a silent line go through the same pushes: stream_bank(fixed=True) -> power_gate(n_frames=93), 95 rows a
    line in pushes that do not line up with the frames, no synchronize in between."""
    import torch
    n = fs.n_samples(512, 95)
    lines = [fs.STIMULI["noise"](n, 512), np.asarray(wav_pcm[3000:3000 + n], np.int16), np.zeros(n, np.int16)]
    ref_rows = [mx.mfcc_fixed_ref(x, nfilters=16, nceptrums=16, pad_mode="notebook") for x in lines]
    assert all(r.shape == (95, 16) for r in ref_rows)
    want = [gr.gate(r, [0, 95], 93, 1) for r in ref_rows]              # (power, gate, gate_ref, win_offsets) per line
    assert all(len(w[0]) == 3 for w in want)
    assert want[0][1].all() and not want[0][2].any() and want[0][0].min() > 1 << 32
    outs = [[] for _ in lines]
    rows_got = [[] for _ in lines]
    with mfcc_amd.MFCC(nfft=512, nfilters=16, nceptrums=16) as m:
        assert m.kernel_name(fixed=True) == "mfcc_fixed512_kernel"
        with m.stream_bank(3, fixed=True) as bank, m.power_gate(3, n_frames=93) as gate:
            cuts = [0, 7000, 7001, 15900, 16100, n]
            for a, b in zip(cuts[:-1], cuts[1:]):
                chunks = [x[a:b] for x in lines]
                offsets = np.arange(4, dtype=np.uint64) * np.uint64(b - a)
                rows, fo = bank.push_packed(_dev(np.concatenate(chunks)), offsets)
                p, g, r, wo = gate.push(rows, fo)
                for u in range(3):
                    rows_got[u].append(rows[int(fo[u]):int(fo[u + 1])])
                    outs[u].append([t[int(wo[u]):int(wo[u + 1])] for t in (p, g, r)])
            torch.cuda.synchronize()
            assert [int(v) for v in gate.seen] == [95, 95, 95]
    for u in range(3):
        differ("line %d rows" % u, torch.cat(rows_got[u]), ref_rows[u])
        for i, what in enumerate(("power", "gate", "gate_ref")):
            got = as_np(torch.cat([o[i] for o in outs[u]]))
            assert np.array_equal(got, want[u][i]), (u, what, got, want[u][i])
    loud_gate = as_np(torch.cat([o[1] for o in outs[0]]))
    loud_ref = as_np(torch.cat([o[2] for o in outs[0]]))
    assert (loud_gate != loud_ref).any()                              # the two gates differ on the loud line
    assert not as_np(torch.cat([o[1] for o in outs[2]])).any()        # silence passes neither
