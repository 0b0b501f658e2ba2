"""Host side of the frame length below nfft (mfcc_hip_create_framed and the _framed helpers): the ABI, frame counts,
refusals, the window table, the bank plans against a model of N independent sessions, the Python argument checks and
the float64 reference of tests/framed_ref.py itself.  No GPU."""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import get_window

import framed_ref as fr
import mfcc_amd
from mfcc_amd import _lib as L
from oracle import mfcc_float as mf

NEW = ["mfcc_hip_create_framed", "mfcc_hip_frame_length", "mfcc_hip_num_frames_framed", "mfcc_hip_get_table_framed",
       "mfcc_hip_bank_plan_framed", "mfcc_hip_bank_plan_online_framed"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _count(p, flen, n):
    out = C.c_size_t(99999)
    rc = L.load().mfcc_hip_num_frames_framed(C.byref(p), flen, n, C.byref(out))
    return rc, int(out.value)


# ------------------------------------------------------------------------------------------------ ABI

def test_new_exports_exist_and_the_abi_is_unchanged():
    lib = L.load()
    for name in NEW:
        assert name in L.SYMBOLS and getattr(lib, name) is not None, name
    assert lib.mfcc_hip_abi_version() == 2 == L.ABI_VERSION
    assert C.sizeof(L.Params) == 64
    assert lib.mfcc_hip_frame_length(None) == 0


# ------------------------------------------------------------------------------------------------ frame counts

@pytest.mark.parametrize("n,notebook,stream", [(16000, 98, 99), (399, 0, 1), (400, 1, 2), (559, 1, 2), (560, 2, 3)])
def test_frame_counts_at_400_160(n, notebook, stream):
    for pad, want in (("notebook", notebook), ("stream", stream)):
        assert mfcc_amd.num_frames(n, win_length=400, nfft=512, hop=160, pad_mode=pad) == want
        assert fr.num_frames(n, 400, 160, pad) == want
        rc, got = _count(mfcc_amd.make_params(nfft=512, hop=160, pad_mode=pad), 400, n)
        assert rc == L.SUCCESS and got == want


@pytest.mark.parametrize("pad", ["notebook", "stream"])
@pytest.mark.parametrize("nfft,hop", [(512, 170), (512, 160), (256, 80), (1024, 1024)])
def test_zero_and_nfft_are_the_unframed_count(nfft, hop, pad):
    p = mfcc_amd.make_params(nfft=nfft, hop=hop, nfilters=8, nceptrums=8, pad_mode=pad)
    for n in list(range(0, 3 * nfft + 7, 13)) + [nfft - 1, nfft, nfft + hop - 1, nfft + hop]:
        plain = mfcc_amd.num_frames(n, nfft=nfft, hop=hop, nfilters=8, nceptrums=8, pad_mode=pad)
        assert _count(p, 0, n) == (L.SUCCESS, plain)
        assert _count(p, nfft, n) == (L.SUCCESS, plain)
        assert mfcc_amd.num_frames(n, win_length=nfft, nfft=nfft, hop=hop, nfilters=8, nceptrums=8, pad_mode=pad) == plain


# ------------------------------------------------------------------------------------------------ refusals

def test_frame_lengths_outside_the_contract_are_refused():
    lib = L.load()
    p = mfcc_amd.make_params(nfft=512, hop=160)
    one = mfcc_amd.make_params(nfft=64, hop=1, nfilters=8, nceptrums=8)
    default_hop = mfcc_amd.make_params(nfft=512)                          # hop 0 -> 170
    h = C.c_void_p()
    n = C.c_size_t(0)
    zeros, fo = np.zeros(1, np.uint64), np.zeros(2, np.uint64)
    offs = np.array([0, 10], np.uint64)
    for params, flen in ((p, 513), (p, 159), (one, 1), (default_hop, 169), (p, -1)):
        assert _count(params, flen, 1000)[0] == L.ERROR_INVALID_PARAM, flen
        assert lib.mfcc_hip_get_table_framed(C.byref(params), flen, L.TABLE_WINDOW_F32, None, 0, C.byref(n)) \
            == L.ERROR_INVALID_PARAM, flen
        assert lib.mfcc_hip_create_framed(C.byref(params), flen, C.byref(h)) == L.ERROR_INVALID_PARAM and not h.value
        assert lib.mfcc_hip_bank_plan_framed(C.byref(params), flen, _ptr(zeros), _ptr(offs), 1, _ptr(fo), None) \
            == L.ERROR_INVALID_PARAM, flen
        assert lib.mfcc_hip_bank_plan_online_framed(C.byref(params), flen, 0, _ptr(zeros), _ptr(zeros), _ptr(offs), 1,
                                                    _ptr(fo), None, None) == L.ERROR_INVALID_PARAM, flen
    assert _count(default_hop, 170, 1000) == (L.SUCCESS, 5)               # the default hop itself is a frame length
    assert _count(one, 2, 10) == (L.SUCCESS, 9)


# ------------------------------------------------------------------------------------------------ window table

@pytest.mark.parametrize("nfft,hop,flen", [(512, 160, 400), (256, 80, 200), (1024, 320, 800), (512, 160, 511),
                                           (512, 160, 160), (64, 1, 2)])
def test_window_table_is_the_short_window_then_zeros(nfft, hop, flen):
    kw = dict(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    w = mfcc_amd.get_table(L.TABLE_WINDOW_F32, win_length=flen, **kw)
    assert w.dtype == np.float32 and w.shape == (nfft,)
    np.testing.assert_allclose(w[:flen], get_window("hamm", flen, fftbins=True), rtol=0, atol=6e-8)
    assert not w[flen:].any() and not np.signbit(w[flen:]).any()
    # every other table is the plain one
    for which in (L.TABLE_MEL_POINTS_I32, L.TABLE_MEL_DENSE_F32, L.TABLE_DCT_F32):
        assert np.array_equal(mfcc_amd.get_table(which, win_length=flen, **kw), mfcc_amd.get_table(which, **kw))


@pytest.mark.parametrize("nfft", [512, 1024, 64])
def test_window_table_with_zero_is_the_existing_table_bit_for_bit(nfft):
    lib = L.load()
    p = mfcc_amd.make_params(nfft=nfft, nfilters=8, nceptrums=8)
    plain = mfcc_amd.get_table(L.TABLE_WINDOW_F32, nfft=nfft, nfilters=8, nceptrums=8)
    for flen in (0, nfft):
        buf = np.empty(nfft, np.float32)
        n = C.c_size_t(0)
        assert lib.mfcc_hip_get_table_framed(C.byref(p), flen, L.TABLE_WINDOW_F32, _ptr(buf), buf.nbytes, C.byref(n)) \
            == L.SUCCESS
        assert n.value == 4 * nfft and np.array_equal(buf.view(np.uint32), plain.view(np.uint32))


# ------------------------------------------------------------------------------------------------ bank plans

class Session:
    """One online session: samples queue up; whenever a frame's worth of them is there a frame leaves and the queue
    moves on by one hop.  With a lag, a row is returned once ``lag`` later ones exist."""

    def __init__(self, flen, hop, lag=0):
        self.flen, self.hop, self.lag, self.queued, self.held = flen, hop, lag, 0, 0

    def push(self, n):
        frames = 0
        self.queued += n
        while self.queued >= self.flen:
            frames += 1
            self.queued -= self.hop
        emitted = max(0, self.held + frames - self.lag)
        self.held += frames - emitted
        return emitted


@pytest.mark.parametrize("lag", [None, 0, 4])
@pytest.mark.parametrize("nfft,hop,flen", [(512, 160, 400), (256, 80, 200), (1024, 320, 800), (512, 160, 160),
                                           (512, 170, 512), (128, 1, 2)])
def test_framed_plans_equal_n_independent_sessions(nfft, hop, flen, lag):
    lib = L.load()
    p = mfcc_amd.make_params(nfft=nfft, hop=hop, nfilters=8, nceptrums=8)
    rng = np.random.default_rng(nfft * 1000 + hop + flen)
    n = 7
    sessions = [Session(flen, hop, lag or 0) for _ in range(n)]
    pending = np.zeros(n, dtype=np.uint64)
    held = np.zeros(n, dtype=np.uint64)
    sizes = [0, 1, 2, 7, hop - 1, hop, hop + 1, flen - 1, flen, flen + 1, 3 * flen + 5, nfft]
    for rnd in range(150):
        lens = rng.choice(sizes, n)
        if rnd % 11 == 0:
            lens[rng.integers(n)] = int(rng.integers(3 * flen + 1, 6 * flen))
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[0] = int(rng.integers(0, 100))
        offsets[1:] = offsets[0] + np.cumsum(lens).astype(np.uint64)
        fo = np.full(n + 1, 12345, dtype=np.uint64)
        after = np.full(n, 12345, dtype=np.uint64)
        held_after = np.full(n, 12345, dtype=np.uint64)
        if lag is None:
            rc = lib.mfcc_hip_bank_plan_framed(C.byref(p), flen, _ptr(pending), _ptr(offsets), n, _ptr(fo), _ptr(after))
        else:
            rc = lib.mfcc_hip_bank_plan_online_framed(C.byref(p), flen, lag, _ptr(pending), _ptr(held), _ptr(offsets), n,
                                                      _ptr(fo), _ptr(after), _ptr(held_after))
        assert rc == L.SUCCESS
        rows = [s.push(int(k)) for s, k in zip(sessions, lens)]
        assert fo[0] == 0 and np.array_equal(np.diff(fo.astype(np.int64)), rows), (rnd, lens)
        assert np.array_equal(after, [s.queued for s in sessions]), (rnd, lens)
        assert int(after.max()) < flen
        if lag is not None:
            assert np.array_equal(held_after, [s.held for s in sessions])
            held = held_after
        pending = after
    # pending[u] must stay below the frame length, not below nfft
    bad = np.zeros(n, dtype=np.uint64)
    bad[3] = flen
    zero_offs = np.zeros(n + 1, dtype=np.uint64)
    fo = np.zeros(n + 1, dtype=np.uint64)
    assert lib.mfcc_hip_bank_plan_framed(C.byref(p), flen, _ptr(bad), _ptr(zero_offs), n, _ptr(fo), None) \
        == L.ERROR_INVALID_PARAM
    assert lib.mfcc_hip_bank_plan_online_framed(C.byref(p), flen, 0, _ptr(bad), _ptr(np.zeros(n, np.uint64)),
                                                _ptr(zero_offs), n, _ptr(fo), None, None) == L.ERROR_INVALID_PARAM


def test_plain_plans_are_the_frame_length_zero_case():
    lib = L.load()
    p = mfcc_amd.make_params()
    pending = np.array([0, 100, 511], np.uint64)
    offsets = np.array([0, 700, 700, 2000], np.uint64)
    a, b = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    pa, pb = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    assert lib.mfcc_hip_bank_plan(C.byref(p), _ptr(pending), _ptr(offsets), 3, _ptr(a), _ptr(pa)) == L.SUCCESS
    assert lib.mfcc_hip_bank_plan_framed(C.byref(p), 0, _ptr(pending), _ptr(offsets), 3, _ptr(b), _ptr(pb)) == L.SUCCESS
    assert np.array_equal(a, b) and np.array_equal(pa, pb)


# ------------------------------------------------------------------------------------------------ Python

def test_python_argument_checks_come_before_the_library():
    for bad in (513, 159, 1, 0, -400, 400.0, "400", True):
        with pytest.raises(ValueError):
            mfcc_amd.MFCC(nfft=512, hop=160, win_length=bad, nfilters=32, nceptrums=13)
        with pytest.raises(ValueError):
            mfcc_amd.num_frames(16000, win_length=bad, nfft=512, hop=160)
        with pytest.raises(ValueError):
            mfcc_amd.get_table(L.TABLE_WINDOW_F32, win_length=bad, nfft=512, hop=160)
    with pytest.raises(ValueError):
        mfcc_amd.num_frames(16000, win_length=169, nfft=512)            # the default hop, 170, above the frame
    assert mfcc_amd.num_frames(16000, win_length=170, nfft=512) == (16000 - 170) // 170 + 1
    assert mfcc_amd.num_frames(16000, win_length=np.int64(400), nfft=512, hop=160) == 98


def test_dist_plans_take_a_frame_length():
    from mfcc_amd import dist as md
    plain = md.plan_frames(16000, 3)
    assert plain == md.plan_frames(16000, 3, 512, 170, None, 512)
    shards = md.plan_frames(16000, 3, 512, 160, frame_length=400)
    assert sum(s.n_frames for s in shards) == 98
    assert shards[-1].sample_hi == 97 * 160 + 400 and shards[1].sample_lo == shards[1].frame_lo * 160 - 1
    assert shards[0].sample_hi == (shards[0].frame_hi - 1) * 160 + 400


# ------------------------------------------------------------------------------------------------ the reference

@pytest.mark.parametrize("nfft,hop,n_mel,ps", [(512, 170, 32, 512.0), (256, 80, 20, 256.0)])
def test_framed_ref_with_the_full_frame_is_the_notebook(wav_pcm, nfft, hop, n_mel, ps):
    x = wav_pcm[3000:3000 + 40 * hop + nfft + 9]
    ref, st = mf.mfcc_notebook(x, nfft=nfft, hop=hop, n_mel=n_mel, power_scale=ps, return_stages=True)
    got, gs = fr.framed_notebook(x, nfft, hop, nfft=nfft, n_mel=n_mel, power_scale=ps)
    assert np.array_equal(got, ref)
    for k in ("power", "filters", "mel", "logmel", "dct_basis"):
        assert np.array_equal(np.asarray(gs[k]), np.asarray(st[k])), k


def test_framed_ref_known_answers_on_the_golden_wav(wav_pcm):
    cep, st = fr.framed_notebook(wav_pcm, 400, 160, nfft=512, n_mel=32, sample_rate=16000, power_scale=512.0)
    assert cep.shape == (1112, 32) == (fr.num_frames(len(wav_pcm), 400, 160), 32)
    np.testing.assert_allclose(cep[0, :3], [31.91789058, 2.56199734, -1.83419968], rtol=0, atol=1e-6)
    np.testing.assert_allclose(cep[500, :3], [40.52235812, -11.34543673, 0.36045787], rtol=0, atol=1e-6)
    assert st["power"].shape == (1112, 257) and st["mel"].shape == st["logmel"].shape == (1112, 32)


@pytest.mark.parametrize("output", ["cepstra", "logmel"])
def test_the_lifter_argument_of_both_references(wav_pcm, output):
    """``lifter=0`` is the call without it, which is the stages' own rows and bound; ``lifter=22`` is those rows and that
    bound times ``1 + 11 sin(pi k / 22)``, and leaves log-mel rows alone (the library's lifter is folded into the DCT)."""
    import melbank_ref as mr
    from oracle import error_bound as eb
    x = wav_pcm[3000:3000 + 20 * 160 + 400].copy()
    x[1500:2500] = 0                                                    # two all-zero frames: NaN rows of the bound
    kw = dict(L=400, hop=160, nfft=512, n_mel=32, n_cep=16, output=output)
    weights = 1.0 + 11.0 * np.sin(np.pi * np.arange(16) / 22.0)
    for ref_mod, more in ((fr, {}), (mr, dict(low=20.0, high=8000))):
        plain, bound = ref_mod.reference_and_bound(x, "bf16x2/fp32", **kw, **more)
        zero, zbound = ref_mod.reference_and_bound(x, "bf16x2/fp32", lifter=0.0, **kw, **more)
        lift, lbound = ref_mod.reference_and_bound(x, "bf16x2/fp32", lifter=22.0, **kw, **more)
        assert np.array_equal(zero, plain, equal_nan=True) and np.array_equal(zbound, bound, equal_nan=True)
        assert np.isnan(bound).all(axis=1).sum() >= 2 and np.isfinite(bound).all(axis=1).sum() >= 10
        if output == "logmel":
            assert plain.shape == (21, 32)
            assert np.array_equal(lift, plain, equal_nan=True) and np.array_equal(lbound, bound, equal_nan=True)
            continue
        if ref_mod is fr:
            cep, st = fr.framed_notebook(x, 400, 160)
        else:
            cep, st = mr.banked_notebook(x, mr.matrix(512, 32, 16000, 20.0, 8000), 400, 160)
        assert np.array_equal(plain, cep[:, :16], equal_nan=True)
        assert np.array_equal(bound, eb.bound_from_stages(st, "bf16x2/fp32", 16), equal_nan=True)
        assert np.array_equal(lift, plain * weights, equal_nan=True)
        assert np.array_equal(lbound, bound * np.abs(weights), equal_nan=True)
        assert np.array_equal(lift, mf.lifter(plain, 22), equal_nan=True)
