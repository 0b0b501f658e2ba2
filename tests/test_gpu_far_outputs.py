"""Every kernel and pass writes rows that lie past byte 2^32, float 2^31 and float 2^32 of the buffer it is given.

One module-scoped float32 arena of tests/far_offsets.py's layout -- 2^31 guard floats in front of 2^32 used ones and
some, 25.8 GB -- is filled with a sentinel once.  A wrong offset shows as a sentinel that changed or as a row that kept
its sentinel, never as a fault: tests/test_far_offsets_host.py proves on the CPU that no 32-bit truncation of an offset
used here leaves the arena.

* Segment passes: three segments of 300, 129 and 37 rows far into the arena, one of them across the line; the rows
  must equal, bit for bit, the same entry on a compact copy, and every other float of the arena stays the sentinel.
* Frame kernels: a few channels of periodic samples (a period of ``q`` hops, ``q`` odd), ``out=`` a view of the arena.
  Per channel rows ``[q, nf - q)`` equal rows ``[2q, nf)`` on the device, the first ``2q`` rows equal a compact call bit
  for bit, one period per channel is held to the kernel's reference, the guard and the tail stay sentinels.
* One ``process_packed`` call whose result passes byte 2^32, against dense calls for a sample of utterances.
* One host-entry call on a channel of just over 2^31 samples, against the device call.

The samples of a frame-kernel case lie behind a poison guard of their own wherever the memory cap leaves room (all but
the fixed-point case, whose samples alone are 22.8 GB): their offsets pass 2^31 and 2^32 as well.

Measured on an MI355X (pytest --durations=0), 43 tests in 12 s: 2.2 s to make and fill the arena once; frame kernels
1024_bf16 2.2 s, 1024_w12bf 1.1 s, fbank_generic 1.0 s, 512_w4 0.9 s, spectrum_generic_1024 0.4 s, fbank512 htk128 0.3 s,
spectrum512, fixed512 and generic_1024 0.1 s, the others 0.05 s or less; the host entry 1.4 s; process_packed 0.1 s;
every segment pass 0.05 s or less.  Inside the whole suite the slowest were 1024_w12 2.8 s, 512_w4 2.7 s and the host
entry 1.4 s; no other test of this file was among the suite's 25 slowest (0.7 s).
"""
import numpy as np
import pytest

import far_offsets as fo
import fbank_ref as fr
import framed_ref as frm
import kernel_families as kf
import logmel_bound as lb
import melbank_ref as mr
import spectrum_ref as sr
from kernel_families import as_np, same
from oracle import error_bound as eb
from oracle import mfcc_fixed as mx

pytestmark = pytest.mark.gpu

W = fo.SEG_WIDTH
ROWS = sum(fo.SEG_ROWS)


@pytest.fixture(scope="module")
def mfcc_amd():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mfcc_amd
    return mfcc_amd


class Arena:
    def __init__(self):
        import torch
        self.f32 = torch.empty(fo.GUARD + fo.OUTPUT_ARENA_FLOATS, dtype=torch.float32, device="cuda")
        fo.fill(self.f32, fo.SENTINEL)
        self.used = self.f32[fo.GUARD:]
        # the same bytes as int16 rows: the guard is 2^31 int16 then, the floats in front of it are never reached
        self.i16 = self.f32.view(torch.int16)
        self.used16 = self.i16[2 * fo.GUARD:]

    def rows(self, n_rows, width, shift_rows=0, i16=False):
        """``(n_rows, width)`` of the used region, ``shift_rows`` rows in."""
        used = self.used16 if i16 else self.used
        return used[shift_rows * width:(shift_rows + n_rows) * width].view(n_rows, width)

    def untouched(self):
        """Every float is the sentinel; if not, they are made so again, for the tests that follow."""
        ok = fo.all_equal_to(self.f32, fo.SENTINEL)
        if not ok:
            fo.fill(self.f32, fo.SENTINEL)
        return ok

    def guards_untouched(self, used_floats):
        """The guard in front and everything behind the first ``used_floats`` floats of the used region."""
        ok = fo.all_equal_to(self.f32[:fo.GUARD], fo.SENTINEL) and fo.all_equal_to(self.used[used_floats:], fo.SENTINEL)
        if not ok:
            fo.fill(self.f32, fo.SENTINEL)
        return ok


@pytest.fixture(scope="module")
def arena():
    import torch
    a = Arena()
    yield a
    del a.used16, a.i16, a.used, a.f32
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def handle(mfcc_amd):
    with mfcc_amd.MFCC(nfft=512, nfilters=32, nceptrums=13) as m:
        yield m


# ---------------------------------------------------------------------------------------------------- segment passes
def _source(i16=False):
    """(ROWS, W) rows of the three segments: log2-like energies with rows of -inf (int16: coefficients)."""
    rng = np.random.default_rng(77)
    if i16:
        return rng.integers(-3000, 3000, (ROWS, W)).astype(np.int16)
    x = (rng.standard_normal((ROWS, W)) * 3.0 + 6.0).astype(np.float32)
    x[40:47] = -np.inf
    x[310] = -np.inf
    return x


VAD = dict(column=0, energy_threshold=0.0, energy_mean_scale=1.0, frames_context=2)


@pytest.mark.parametrize("name,line", fo.SEG_CASES, ids=["%s-%s" % c for c in fo.SEG_CASES])
def test_segment_pass_far_into_the_arena(handle, arena, name, line):
    import torch
    m = handle
    offs, lays = fo.segment_case(name, line)
    r0, r3 = offs[0], offs[-1]
    far_fo = np.asarray(offs, np.uint64)
    near_fo = far_fo - np.uint64(r0)
    i16 = name == "gate"
    src = torch.from_numpy(_source(i16)).cuda()
    n_rows = r3 + 8
    rows = arena.rows(n_rows, W, i16=i16)
    rows[r0:r3] = src
    wrote = [rows[r0:r3]]
    try:
        if name == "normalize":
            far = m.normalize_rows(rows, far_fo, mode="meanvar")[r0:r3]
            near = m.normalize_rows(src.clone(), near_fo, mode="meanvar")
        elif name == "normalize_sliding":
            out = arena.rows(n_rows, W, fo.SEG_SHIFT_ROWS)
            wrote.append(out[r0:r3])
            kw = dict(mode="mean", window=50, min_window=1, center=False)
            far = m.normalize_rows(rows, far_fo, out=out, **kw)[r0:r3]
            near = m.normalize_rows(src, near_fo, out=torch.full_like(src, fo.SENTINEL), **kw)
        elif name == "pcen":
            far = m.pcen_rows(rows, far_fo)[r0:r3]
            near = m.pcen_rows(src.clone(), near_fo)
        elif name in ("deltas", "deltas_out"):
            order = 1 if name == "deltas" else 2
            out = arena.rows(n_rows, W * (1 + order))
            wrote.append(out[r0:r3])
            far = m.deltas_rows(rows, far_fo, order=order, out=out)[r0:r3]
            near = m.deltas_rows(src, near_fo, order=order)
        elif name == "vad":
            voiced = m.vad_rows(rows, far_fo, **VAD)
            assert int(voiced.sum()) == int(voiced[r0:r3].sum())             # nothing outside the segments
            far, near = voiced[r0:r3], m.vad_rows(src, near_fo, **VAD)
            assert 0 < int(near.sum()) < ROWS
        elif name == "select":
            near_mask = m.vad_rows(src, near_fo, **VAD)
            mask = torch.zeros(n_rows, dtype=torch.uint8, device="cuda")
            mask[r0:r3] = near_mask
            cap = torch.full((ROWS + 3, W), fo.SENTINEL, dtype=torch.float32, device="cuda")
            far, far_oo = m.select_rows(rows, mask, far_fo, out=cap)
            near, near_oo = m.select_rows(src, near_mask, near_fo)
            assert np.array_equal(far_oo, near_oo) and 0 < len(near) < ROWS
            assert bool((cap[len(near):] == fo.SENTINEL).all())
        else:
            far = m.gate_rows(rows, far_fo)
            near = m.gate_rows(src, near_fo)
            assert np.array_equal(far[3], near[3]) and int(near[3][-1]) > 0
            far, near = torch.cat([t.to(torch.int64) for t in far[:3]]), torch.cat([t.to(torch.int64) for t in near[:3]])
        torch.cuda.synchronize()
        assert same(far, near), "%s at %s: rows %d.. differ from the compact call" % (name, line, r0)
        if name in ("vad", "select", "gate", "deltas", "deltas_out", "normalize_sliding"):
            assert same(rows[r0:r3], src), "%s at %s changed its input" % (name, line)
    finally:
        torch.cuda.synchronize()
        for t in wrote:
            t.fill_(fo.SENTINEL_I16 if i16 else fo.SENTINEL)
        if i16:                                     # the int16 rows were half words of sentinel floats before
            arena.used[(r0 * W) // 2 - 1:(r3 * W) // 2 + 2].fill_(fo.SENTINEL)
        clean = arena.untouched()                   # also after a failure above: the next test starts from sentinels
    assert clean, "%s at %s wrote outside its rows" % (name, line)


# ---------------------------------------------------------------------------------------------------- frame kernels
OUT_KINDS = ["speech", "noise", "uniform", "noise"]               # the second noise is 24 dB down


def _periods(case, wav_pcm, q, hop, n_kinds=4):
    out = [kf.signal(OUT_KINDS[c], q * hop, 800 + c, wav_pcm) for c in range(n_kinds)]
    out[3] = (out[3] // 16).astype(np.int16)
    return out


_fill_periodic = fo.fill_periodic


def _guarded_samples(count, guard=True):
    """``count`` int16 samples behind a guard of 2^31 samples of poison in the same allocation: a sample offset that lost
    its upper bits reads poison, not the memory in front of the allocation."""
    import torch
    front = fo.GUARD if guard else 0
    buf = torch.empty(front + count, dtype=torch.int16, device="cuda")
    fo.fill(buf[:front], fo.POISON_I16)
    return buf[front:]


def _bank(name):
    return {"htk128": lambda: fr.htk_weights(128), "dense128": lambda: fr.dense_random(128),
            "dense128_256": lambda: fr.dense_random(128, 256)}[name]()


def _reference(case, x):
    """(ref, bound) of the rows of ``x`` (channels, n); bound ``None``: bit for bit."""
    kw, kernel = case.kw, case.kernel
    nfft = kw["nfft"]
    if case.entry == "spectrum":
        ref = sr.reference(x, nfft, case.hop, case.flen)
        return ref, sr.bound(ref)
    if case.entry == "fbank":
        Wm = _bank(case.bank if nfft == 512 else case.bank + "_256")
        return fr.reference_and_bound(x, Wm, nfft, case.hop, case.flen, form=fr.form_of(Wm, kernel))
    if case.entry == "fixed":
        return np.stack([mx.mfcc_fixed_ref(c, nfft=nfft, nfilters=kw["nfilters"], nceptrums=kw["nceptrums"],
                                           sample_rate=16000.0, pad_mode="notebook") for c in x]), None
    output = kw.get("output", "cepstra")
    if kernel in ("mfcc_fused512_h160_kernel", "mfcc_fused512_h160_mb_kernel"):
        args = dict(L=case.flen, hop=case.hop, nfft=nfft, n_mel=kw["nfilters"], sample_rate=16000, power_scale=512.0,
                    n_cep=kw["nceptrums"], output=output)
        if kernel.endswith("mb_kernel"):
            return mr.reference_and_bound(x, "bf16x2/fp32", low=float(kw["fmin"]), high=kw["fmax"], **args)
        return frm.reference_and_bound(x, "bf16x2/fp32", **args)
    nb = dict(nfft=nfft, hop=case.hop, n_mel=kw["nfilters"], sample_rate=16000, power_scale=float(nfft))
    if output == "logmel":
        return lb.reference_and_bound(x, lb.MODEL[kernel], **nb)
    model = eb.model_of(kernel, case.env.get("MFCC_HIP_FUSED1024"))
    return eb.reference_and_bound(x, model, n_cep=kw["nceptrums"], **nb)


def _check_period(case, got, ref, bound, what):
    if bound is None:
        assert np.array_equal(got, ref), "%s: differs from the RTL oracle" % what
    elif case.entry == "spectrum":
        sr.check(got, ref, bound, what)
    elif case.entry == "fbank":
        assert fr.check(got, ref, bound, "energy", 0.0, what)[1] == 0
    else:
        eb.check(got, ref, bound, what)


@pytest.mark.parametrize("case", fo.OUT_CASES, ids=fo.OUT_IDS)
def test_frame_kernel_writes_far_rows(mfcc_amd, arena, wav_pcm, monkeypatch, case):
    import torch
    for var in ("MFCC_HIP_FUSED512", "MFCC_HIP_FUSED1024"):
        monkeypatch.delenv(var, raising=False)
    for var, value in case.env.items():
        monkeypatch.setenv(var, value)
    q, hop, nch, width = case.q, case.hop, case.nch, case.width
    nf, n = case.rows_per_channel, case.samples
    fixed = case.entry == "fixed"
    periods = _periods(case, wav_pcm, q, hop)
    with mfcc_amd.MFCC(**case.kw) as m:
        if case.entry == "spectrum":
            assert m.spectrum_kernel_name() == case.kernel
            call = m.power_spectrum
        elif case.entry == "fbank":
            m.set_filterbank(_bank(case.bank if case.kw["nfft"] == 512 else case.bank + "_256"), "energy")
            assert m.filterbank_kernel_name() == case.kernel
            call = m.filterbank
        else:
            assert m.kernel_name(fixed=fixed) == case.kernel
            call = m.process_fixed if fixed else m.process
        assert m.num_frames(n) == nf and m._row(fixed, {"spectrum": "spectrum", "fbank": "fbank"}.get(case.entry)) == width
        pcm = _guarded_samples(nch * n, case.guard_input).view(nch, n)
        for c in range(nch):
            _fill_periodic(pcm[c], torch.from_numpy(periods[c]).cuda())
        out = arena.rows(nch * nf, width, i16=fixed).view(nch, nf, width)
        try:
            back = call(pcm, out=out)
            assert back.data_ptr() == out.data_ptr()
            n2 = case.flen + (2 * q - 1) * hop
            compact = call(pcm[:, :n2].contiguous())
            torch.cuda.synchronize()
            assert tuple(compact.shape) == (nch, 2 * q, width)
            for c in range(nch):
                assert fo.dev_equal(out[c, q:nf - q], out[c, 2 * q:nf]), "%s: channel %d is not periodic" % (case.id, c)
            head = out[:, :2 * q].clone()
            assert same(head, compact), "%s: the first rows differ from a compact call" % case.id
        finally:
            torch.cuda.synchronize()
            del pcm
            torch.cuda.empty_cache()
            used = out.numel() // 2 if fixed else out.numel()
            fo.fill(arena.used[:used + 2], fo.SENTINEL)
            clean = arena.guards_untouched(used + 2)
        assert clean, "%s wrote outside its view" % case.id
    x = np.stack([np.resize(p, n2) for p in periods[:nch]])
    ref, bound = _reference(case, x)
    _check_period(case, as_np(head)[:, q:], ref[:, q:], None if bound is None else bound[:, q:], "%s, one period" % case.id)


# ---------------------------------------------------------------------------------------------------- one ragged result
def test_process_packed_result_passes_byte_2_32(mfcc_amd, arena, wav_pcm):
    import torch
    lens = fo.packed_lens()
    q, width = fo.PACKED_Q, fo.PACKED_WIDTH
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    periods = [torch.from_numpy(p).cuda() for p in _periods(None, wav_pcm, q, 170)]
    flat = _guarded_samples(int(offs[-1]))
    for v in sorted(set(lens)):                      # utterance u repeats period u mod 4 from its own first sample
        for k in range(4):
            one = torch.empty(v, dtype=torch.int16, device="cuda")
            _fill_periodic(one, periods[k])
            us = [u for u in range(k, len(lens), 4) if lens[u] == v]
            for u in us:
                flat[int(offs[u]):int(offs[u + 1])] = one
    with mfcc_amd.MFCC(**fo.PACKED_KW) as m:
        assert m.kernel_name() == fo.PACKED_KERNEL
        lay = fo.packed_layout(m.num_frames)
        total = sum(s.count for s in lay.spans) // width
        assert (total * width * 4) > 1 << 32
        out = arena.rows(total, width)
        try:
            rows, fro = m.process_packed(flat, offs, out=out)
            assert rows.data_ptr() == out.data_ptr() and int(fro[-1]) == total
            assert [int(v) * width for v in fro[:-1]] == [s.start for s in lay.spans]
            torch.cuda.synchronize()
            for u in sorted(set(fo.PACKED_SAMPLED) | set(range(0, len(lens), 997))):
                a, b = int(fro[u]), int(fro[u + 1])
                assert fo.dev_equal(rows[a + q:b - q], rows[a + 2 * q:b]), "utterance %d is not periodic" % u
                if u in fo.PACKED_SAMPLED:
                    dense = m.process(flat[int(offs[u]):int(offs[u + 1])])
                    assert same(rows[a:b], dense), "utterance %d differs from a dense call" % u
        finally:
            torch.cuda.synchronize()
            del flat
            fo.fill(arena.used[:total * width], fo.SENTINEL)
            clean = arena.guards_untouched(total * width)
        assert clean, "process_packed wrote outside its rows"


# ---------------------------------------------------------------------------------------------------- the host route
def test_host_entry_on_a_channel_past_2_31_samples(mfcc_amd, wav_pcm):
    import torch
    period = _periods(None, wav_pcm, fo.HOST_Q, 170)[0]
    x = np.resize(period, fo.HOST_SAMPLES)
    with mfcc_amd.MFCC(**fo.HOST_KW) as m:
        assert m.kernel_name() == "mfcc_fused512_w12_kernel"
        host = m.process(x)
        d = torch.from_numpy(x).cuda()
        dev = m.process(d)
        torch.cuda.synchronize()
        q, nf = fo.HOST_Q, len(host)
        assert nf == m.num_frames(fo.HOST_SAMPLES) and fo.dev_equal(dev[q:nf - q], dev[2 * q:nf])
        assert same(host, dev), "frame-range chunks past sample 2^31 differ from the device call"
    del d, dev
    torch.cuda.empty_cache()
