"""The kernel families of the library, one row each: how to make a handle that runs the family, the kernel the handle
must report, and the contract its results are held to -- TEST INFRASTRUCTURE ONLY (a plain module, not a conftest).

* float families: ``oracle.error_bound.check`` against ``eb.model_of(kernel_name)``, every coefficient of every frame;
* fixed families: ``oracle.mfcc_fixed.mfcc_fixed_ref`` bit for bit.

A test asserts ``kernel_name()`` before anything else, so that a handle rerouted to another kernel fails loudly
instead of testing the wrong code.  All geometry comes from ``nfft`` / ``hop`` of the row.

The input kinds below stay quiet behind pre-emphasis, full scale included; ``fixed_stimuli.STIMULI`` is the loud set
of the fixed families (tests/test_gpu_fixed_reach.py).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import error_bound as eb
from oracle import mfcc_fixed as mx


@dataclass(frozen=True)
class Family:
    id: str
    fixed: bool
    kernel: str
    nfft: int
    nfilters: int
    nceptrums: int
    samplerate: int = 16000
    extra: dict = field(default_factory=dict)      # further MFCC() arguments (power_scale)
    why: str = ""
    hop: int = 0                                   # 0: nfft // 3, the library's default

    def __post_init__(self):
        if not self.hop:
            object.__setattr__(self, "hop", self.nfft // 3)

    def kwargs(self, pad_mode="notebook", **over):
        kw = dict(nfft=self.nfft, hop=self.hop, nfilters=self.nfilters, nceptrums=self.nceptrums,
                  samplerate=self.samplerate, pad_mode=pad_mode, **self.extra)
        kw.update(over)
        return kw

    def notebook_kw(self):
        """Arguments of ``oracle.mfcc_float.mfcc_notebook`` for this family's float handle."""
        ps = self.extra.get("power_scale", 512.0)
        return dict(nfft=self.nfft, hop=self.hop, n_mel=self.nfilters, sample_rate=self.samplerate,
                    power_scale=float(self.nfft) if not ps else float(ps))


FLOAT = [
    Family("f512", False, "mfcc_fused512_w12_kernel", 512, 32, 13, why="the control"),
    Family("f512_48k", False, "mfcc_fused512_w12_kernel", 512, 32, 13, 48000, why="the int8 DC-band path"),
    Family("f512_16f", False, "mfcc_fused512_w12_kernel", 512, 16, 16, why="16 filters: block 1 masked"),
    Family("f1024", False, "mfcc_fused1024_w12bf_kernel", 1024, 40, 13, extra=dict(power_scale=0), why="config 4"),
    Family("f1024_44k", False, "mfcc_fused1024_w12bf_kernel", 1024, 40, 32, 44100, extra=dict(power_scale=0),
           why="a per-rate schedule"),
    Family("g64", False, "mfcc_float_generic_kernel", 64, 8, 8, extra=dict(power_scale=0)),
    Family("g256", False, "mfcc_float_generic_kernel", 256, 20, 13, extra=dict(power_scale=0),
           why="n_mel not a power of two"),
    Family("g1024_64", False, "mfcc_float_generic_kernel", 1024, 64, 32, extra=dict(power_scale=0)),
    # other hops: every one runs on the generic kernel, whatever its shape (the fused kernels hard-code theirs)
    Family("f512_h160", False, "mfcc_float_generic_kernel", 512, 32, 13, hop=160,
           why="10 ms at 16 kHz; the fused 512 kernel's shape"),
    Family("f512_h171", False, "mfcc_float_generic_kernel", 512, 32, 13, hop=171, why="one off the fused hop"),
    Family("f1024_h256", False, "mfcc_float_generic_kernel", 1024, 40, 13, extra=dict(power_scale=0), hop=256,
           why="75 % overlap; the fused 1024 kernel's shape"),
    Family("g512_h257", False, "mfcc_float_generic_kernel", 512, 32, 32, 48000, hop=257,
           why="hop above nfft / 2; the exact-DC branch"),
    Family("g256_h256", False, "mfcc_float_generic_kernel", 256, 20, 13, extra=dict(power_scale=0), hop=256,
           why="hop = nfft: frames share only the pre-emphasis history"),
    Family("g128_h1", False, "mfcc_float_generic_kernel", 128, 16, 13, extra=dict(power_scale=0), hop=1,
           why="every sample starts a frame"),
]
FIXED = [
    Family("x512", True, "mfcc_fixed512_kernel", 512, 32, 13, why="the control"),
    Family("x512_16f", True, "mfcc_fixed512_kernel", 512, 16, 16, why="log2 + DCT once per four frames"),
    Family("x64_4", True, "mfcc_fixed_kernel", 64, 4, 4, why="the 16-point DCT FFT of fx_fft_inplace"),
    Family("x256_16", True, "mfcc_fixed_kernel", 256, 16, 16),
    Family("x512_8", True, "mfcc_fixed_kernel", 512, 8, 8, why="the generic <512> instantiation"),
    Family("x1024_64", True, "mfcc_fixed_kernel", 1024, 64, 32),
]
ALL = FLOAT + FIXED
IDS = [f.id for f in ALL]

# HTK banks at 512 / 160 by the set mask mfcc_fused160mb::build_tables derives from their matrix (bit 2 block + group: the
# (filter block, K group) pair carries weight; the bank kernel branches on it and indexes its operands by a running
# count).  id -> (n_mel, fmin, fmax, sample rate, mask).  tests/test_fused512_tables_host.py proves the masks on the CPU,
# tests/test_gpu_melbank.py runs every one; the banks of the other tests give 3, 13, 45 and 213 only.
MASK_BANKS = {
    "m0_1f_bin16": (1, 480, 530, 16000, 0),             # no set at all: all weight on bin 16, through column 16
    "m1_1f": (1, 3000, 3400, 16000, 1),                 # block 0, group 0 only
    "m2_2f_high": (2, 6000, 8000, 16000, 2),            # group 1 without group 0
    "m10_24f_high": (24, 4000, 8000, 16000, 10),        # two blocks, group 1 only
    "m11_17f_8k": (17, 300, 3400, 8000, 11),            # second block with one filter
    "m21_40f_telephone": (40, 300, 3400, 16000, 21),    # three blocks, group 0 only
    "m42_40f_high": (40, 4000, 8000, 16000, 42),        # three blocks, group 1 only
    "m53_48f": (48, 20, 8000, 16000, 53),               # three full blocks
    "m170_64f_high": (64, 5000, 8000, 16000, 170),      # four blocks, group 1 only
    "m181_49f": (49, 20, 8000, 16000, 181),             # fourth block with one filter
    "m11_17f": (17, 20, 8000, 16000, 11),
    "m45_33f": (33, 20, 8000, 16000, 45),
}


def open_handle(mfcc_amd, fam: Family, pad_mode="notebook", **over):
    """An ``MFCC`` handle of the family; fails unless the library reports the family's kernel."""
    m = mfcc_amd.MFCC(**fam.kwargs(pad_mode, **over))
    name = m.kernel_name(fixed=fam.fixed)
    if name != fam.kernel:
        m.close()
        raise AssertionError("%s: handle runs %s, not %s" % (fam.id, name, fam.kernel))
    return m


def run(m, fam: Family, x, **kw):
    """``process`` / ``process_fixed`` by the family's contract."""
    return m.process_fixed(x, **kw) if fam.fixed else m.process(x, **kw)


def as_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(a, b) -> bool:
    """Bit for bit, -inf / NaN patterns included."""
    a, b = as_np(a), as_np(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


# ------------------------------------------------------------------------------------------------ inputs

KINDS = ["speech", "noise", "uniform", "square", "const_min", "silences"]


def signal(kind, n, seed, wav_pcm):
    """One channel of int16 input: a slice of the golden speech file, Gaussian noise, full-scale uniform noise, an
    alternating +-full-scale square, constant -32768, or noise with silent stretches."""
    rng = np.random.default_rng(seed)
    if kind == "speech":
        return np.resize(wav_pcm[(seed * 977) % 20000:], n).astype(np.int16)
    if kind == "noise":
        return np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16)
    if kind == "uniform":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    if kind == "square":
        period = int(rng.integers(2, 40))
        return np.where((np.arange(n) // max(1, period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)
    if kind == "const_min":
        return np.full(n, -32768, np.int16)
    if kind == "silences":
        x = np.clip(np.rint(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16)
        for a in rng.integers(0, max(n - 3000, 1), 3):
            x[a:a + int(rng.integers(300, 3000))] = 0
        return x
    raise ValueError(kind)


def channels(n, seed, wav_pcm, kinds=KINDS):
    return np.stack([signal(k, n, seed + i, wav_pcm) for i, k in enumerate(kinds)])


def silent_stream(fam: Family, n_frames, seed):
    """Noise of ``n_frames`` notebook frames with stretches of digital silence longer than a frame (frames that see
    zeros only: -inf log-mel on the float path) and shorter ones (frames that see them partly)."""
    hop, nfft = fam.hop, fam.nfft
    n = hop * (n_frames - 1) + nfft
    x = np.clip(np.rint(np.random.default_rng(seed).standard_normal(n) * 3000), -32768, 32767).astype(np.int16)
    for a, length in ((n // 5, 3 * nfft + hop), (n // 2, nfft // 2), ((3 * n) // 4, 2 * nfft + 7)):
        x[a:a + length] = 0
    return x


# ------------------------------------------------------------------------------------------------ oracle

def check_oracle(fam: Family, got, pcm, pad_mode="notebook", halo=0, what=""):
    """``got`` (channels?, frames, n_cep) against the family's contract on ``pcm`` (channels?, n); with ``halo=1``,
    sample 0 of every channel is pre-emphasis history only.  Returns the worst error / bound ratio (0 for fixed)."""
    got = as_np(got)
    pcm = np.asarray(pcm)
    if pcm.ndim == 1:
        got, pcm = got[None], pcm[None]
    worst = 0.0
    for c in range(len(pcm)):
        tag = "%s %s channel %d" % (fam.id, what, c)
        if fam.fixed:
            ref = fixed_ref(fam, pcm[c], pad_mode, halo)
            assert got[c].shape == ref.shape, (tag, got[c].shape, ref.shape)
            if not np.array_equal(got[c], ref):
                bad = np.argwhere(got[c] != ref)
                raise AssertionError("%s: %d value(s) differ from the RTL oracle, first at (frame, coef) %s: got %d, "
                                     "oracle %d" % (tag, len(bad), tuple(bad[0]), got[c][tuple(bad[0])],
                                                    ref[tuple(bad[0])]))
        else:
            ref, bound = eb.reference_and_bound(pcm[c], eb.model_of(fam.kernel), n_cep=fam.nceptrums,
                                                pad_mode=pad_mode, halo=halo, **fam.notebook_kw())
            worst = max(worst, eb.check(got[c], ref, bound, tag))
    return worst


def fixed_ref(fam: Family, x, pad_mode="notebook", halo=0):
    """The RTL oracle of one channel; ``halo=1``: ``x[0]`` is history only -- the channel goes ``hop - 1`` zeros into a
    longer stream, whose frame 1 is then the shard's frame 0 with ``x[0]`` in front of it, and frame 0 is dropped."""
    x = np.asarray(x)
    if halo:
        x = np.concatenate([np.zeros(fam.hop - 1, x.dtype), x])
    ref = mx.mfcc_fixed_ref(x, nfft=fam.nfft, nfilters=fam.nfilters, nceptrums=fam.nceptrums,
                            sample_rate=float(fam.samplerate), pad_mode=pad_mode)
    return ref[1:] if halo else ref
