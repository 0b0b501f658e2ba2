"""float64 reference and per-element error bound of the power-spectrum output (``MFCC.power_spectrum``) -- TEST
INFRASTRUCTURE ONLY (a plain module, not a conftest).

Reference.  The notebook's own ``audio_power`` (MFCC.ipynb cell 22): ``oracle.mfcc_float.mfcc_notebook(...,
return_stages=True)["power"]`` on the sample stream whose notebook framing gives the kernel's frames
(``oracle.error_bound._frames_source``: STREAM padding and the ``halo`` sample).  A framed handle (frame length ``L`` below
``nfft``) takes the float64 staging of tests/framed_ref.py, restated here up to the power; with ``L = nfft`` that is the
notebook's chain call for call.

Bound, per element, with ``P`` the reference power of the element::

    B = C_SPEC (2 sqrt(P) e + e^2) + 4 u P        e = u rms(X) log2(nfft),  u = 2^-24

``e`` is the FFT term of ``oracle/error_bound.py`` (rms over the frame's full spectrum, in the units of ``X /
power_scale``); ``4 u P`` covers the two squares, their sum and the scale.

C_SPEC is measured, not tuned per input.  With C_SPEC = 1 a plain fp32 FFT already exceeds the per-bin bound on structured
inputs (mel bands average that out, single bins do not), so the constant is taken from an fp32 restatement on the CPU
(:func:`restatement_f32`: exact integer pre-emphasis, the window rounded to fp32, ``scipy.fft.rfft`` on float32, the power
in fp32): C_SPEC is twice its worst ``|delta| / B(C_SPEC = 1)`` over the inputs of the GPU tests (:func:`input_list`, all
three framings of :data:`FRAMINGS`; at the fused kernel's two shapes also the steady-state batch as an MI355X gets it,
385 channels of 37 frames, and at 512 / 170 the whole golden wav), rounded up to a power of two -- twice, because the
kernels' 32 x 16 decomposition orders its roundings differently from pocketfft at the same depth -- and never above 8, the
coherent worst case of window rounding ``(2 sqrt(nfft) + log2 nfft) / log2 nfft`` at nfft 1024.  :func:`measure` gives
the table; measured on the CPU (worst ratio of the restatement at C_SPEC = 1, the kind that gives it):

    ===================  =====  ==========
    nfft / hop / frame   worst  input
    ===================  =====  ==========
    512 / 170 / 512      2.73   sine8 (the steady-state batch; 1.39, square, on the seven channels of 33 frames)
    512 / 160 / 400      2.16   sine8 (the steady-state batch; 1.28, sine8, on the seven channels)
    1024 / 341 / 1024    2.01   sine8
    256 / 80 / 200       1.04   square
    64 / 21 / 64         0.69   uniform
    ===================  =====  ==========

so C_SPEC = 8: 2 x 2.73 = 5.46, rounded up to a power of two (and at the cap).  tests/test_spectrum_host.py measures the
table again, requires that constant of it, and holds the restatement to B / 2: the reference arithmetic alone stays well
inside what a kernel is allowed.

Not-blind conditions (conditions, not tolerances): every element of a frame with a non-zero pre-emphasised sample has a
finite, positive bound; the elements with bound 0 are exactly the frames whose pre-emphasised samples are all zero, and
a kernel must return +0.0 there bit for bit; :func:`check` raises on any NaN, any negative value and any shape mismatch.
"""
from __future__ import annotations

import numpy as np
import scipy.fft

from oracle import error_bound as eb
from oracle import mfcc_float as mf

U = 2.0 ** -24
C_SPEC = 8.0
C_SPEC_CAP = 8.0

# (nfft, hop, frame length) the tests cover; the first two run the fused kernel, the others the generic one
CONFIGS = [(512, 170, 512), (512, 160, 400), (1024, 341, 1024), (256, 80, 200), (64, 21, 64)]
FRAMINGS = [("notebook", 0), ("stream", 0), ("notebook", 1)]          # (pad_mode, halo)
KINDS = ["speech", "noise", "uniform", "square", "const_min", "silences", "sine8"]
MAX_FRAMES = 33


def power_scale_of(nfft):
    return 512.0 if nfft == 512 else float(nfft)


def num_frames(n, L, hop, pad_mode="notebook"):
    if pad_mode == "notebook":
        return 0 if n < L else (n - L) // hop + 1
    return 1 if n < L else (n - L) // hop + 2


def samples_for(frames, L, hop):
    """Samples of a channel with ``frames`` notebook frames."""
    return L + (frames - 1) * hop


def signal(kind, n, seed, wav_pcm, nfft):
    """One channel: the six kinds of tests/kernel_families.py and a full-scale sine on bin 8 of the transform, its
    start phase from the seed."""
    import kernel_families as kf
    if kind == "sine8":
        return np.rint(32767.0 * np.sin(2.0 * np.pi * 8.0 * np.arange(n) / nfft + 0.37 * seed)).astype(np.int16)
    return kf.signal(kind, n, seed, wav_pcm)


def batch_inputs(nfft, hop, L, wav_pcm, n_channels, frames, seed=11):
    """(n_channels, n) int16, ``frames`` notebook frames long: channel i is kind ``KINDS[i % 7]`` with seed ``seed + i``."""
    n = samples_for(frames, L, hop)
    return np.stack([signal(KINDS[i % len(KINDS)], n, seed + i, wav_pcm, nfft) for i in range(n_channels)])


def input_list(nfft, hop, L, wav_pcm, frames=MAX_FRAMES, seed=11):
    """(7, n) int16: one channel per kind, ``frames`` notebook frames long."""
    return batch_inputs(nfft, hop, L, wav_pcm, len(KINDS), frames, seed)


# the batch of the steady-state test (tests/test_gpu_spectrum.py, shaped like tests/test_gpu_steady_state.py): channels of
# ``tpc`` tiles (3 unless the CU count is a multiple of 3), the last one partial, about 4.5 x CUs tiles
MI355X_CUS = 256


def steady_shape(n_cu):
    """(tiles per channel, frames per channel, channels) of the steady-state batch on ``n_cu`` compute units."""
    tpc = next(t for t in (3, 5, 7) if n_cu % t)
    return tpc, 16 * (tpc - 1) + 5, 9 * n_cu // (2 * tpc) + 1


def _source(x, L, hop, pad_mode, halo):
    """``eb._frames_source`` with the frame length in place of nfft (the same function when they are equal)."""
    x = np.asarray(x)
    if halo:
        x = np.concatenate([np.zeros(hop - 1, dtype=x.dtype), x])
    if pad_mode == "stream":
        nf = num_frames(len(x), L, hop, "stream")
        x = np.concatenate([x, np.zeros((nf - 1) * hop + L - len(x), dtype=x.dtype)])
    elif pad_mode != "notebook":
        raise ValueError(pad_mode)
    return x, int(bool(halo))


def reference(pcm, nfft=512, hop=170, L=None, power_scale=None, pad_mode="notebook", halo=0):
    """float64 ``(channels?, frames, nfft // 2 + 1)`` power of int16 ``pcm`` ``(n,)`` or ``(channels, n)``."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        return np.stack([reference(c, nfft, hop, L, power_scale, pad_mode, halo) for c in pcm])
    L = nfft if L is None else L
    scale = power_scale_of(nfft) if power_scale is None else float(power_scale)
    bins = nfft // 2 + 1
    if L == nfft:
        x, drop = eb._frames_source(pcm, nfft, hop, pad_mode, halo)
        if len(x) < nfft:
            return np.zeros((0, bins))
        # the filterbank does not reach the power; 8 filters exist at every nfft
        _, st = mf.mfcc_notebook(x, nfft=nfft, hop=hop, n_mel=8, sample_rate=16000, power_scale=scale, return_stages=True)
        return np.asarray(st["power"], dtype=np.float64)[drop:]
    x, drop = _source(pcm, L, hop, pad_mode, halo)
    if len(x) < L:
        return np.zeros((0, bins))
    framed = mf.frame_audio(mf.pre_emphasis(x), nfft=L, hop=hop)          # tests/framed_ref.py: framed_notebook
    win = framed * mf.hamming_window(L)
    padded = np.zeros((len(win), nfft))
    padded[:, :L] = win
    return np.asarray(mf.power_spectrum(mf.fft_frames(padded, nfft), scale), dtype=np.float64)[drop:]


def emphasised_frames(pcm, nfft, hop, L, pad_mode, halo):
    """int64 ``(frames, L)``: ``32 x[i] - 31 x[i - 1]`` of every frame's own samples -- 32 times the pre-emphasised
    stream, exact."""
    x, drop = _source(np.asarray(pcm), L, hop, pad_mode, halo)
    if len(x) < L:
        return np.zeros((0, L), np.int64)
    x = x.astype(np.int64)
    e = 32 * x - 31 * np.concatenate([[0], x[:-1]])
    nf = (len(x) - L) // hop + 1
    idx = np.arange(L)[None, :] + hop * np.arange(nf)[:, None]
    return e[idx][drop:]


def bound(power, c_spec=C_SPEC):
    """Per-element bound of a float64 reference ``(..., frames, bins)``."""
    power = np.asarray(power, dtype=np.float64)
    nfft = 2 * (power.shape[-1] - 1)
    full = power[..., 0] + power[..., -1] + 2.0 * power[..., 1:-1].sum(axis=-1)
    e = (U * np.sqrt(full / nfft) * np.log2(nfft))[..., None]
    return c_spec * (2.0 * np.sqrt(power) * e + e * e) + 4.0 * U * power


def restatement_f32(pcm, nfft=512, hop=170, L=None, power_scale=None, pad_mode="notebook", halo=0):
    """The chain in fp32 on the CPU: exact integer pre-emphasis, the window rounded to fp32, ``scipy.fft.rfft`` on
    float32 (which must return complex64), the power in fp32.  float32 ``(channels?, frames, bins)``."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        return np.stack([restatement_f32(c, nfft, hop, L, power_scale, pad_mode, halo) for c in pcm])
    L = nfft if L is None else L
    scale = power_scale_of(nfft) if power_scale is None else float(power_scale)
    e = emphasised_frames(pcm, nfft, hop, L, pad_mode, halo)
    y = (e.astype(np.float32) / np.float32(32.0)).astype(np.float32)       # exact: |e| < 2^21
    w = mf.hamming_window(L).astype(np.float32)
    padded = np.zeros((len(y), nfft), np.float32)
    padded[:, :L] = y * w[None, :]
    X = scipy.fft.rfft(padded, axis=1)
    if X.dtype != np.complex64:
        raise AssertionError("scipy.fft.rfft of float32 returned %s, not complex64" % X.dtype)
    inv = np.float32(1.0 / (scale * scale))
    p = (X.real * X.real + X.imag * X.imag) * inv
    assert p.dtype == np.float32
    return p


def zero_frames(pcm, nfft, hop, L, pad_mode, halo):
    """Boolean ``(channels?, frames)``: frames whose pre-emphasised samples are all zero."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        return np.stack([zero_frames(c, nfft, hop, L, pad_mode, halo) for c in pcm])
    return ~(emphasised_frames(pcm, nfft, hop, nfft if L is None else L, pad_mode, halo) != 0).any(axis=1)


def assert_not_blind(b, zero, what=""):
    """The not-blind condition: ``b`` (..., frames, bins) is finite everywhere, positive in every element of a frame that
    has a non-zero sample, and 0 exactly in the frames of ``zero`` (..., frames)."""
    b = np.asarray(b)
    zero = np.asarray(zero, dtype=bool)
    if b.shape[:-1] != zero.shape:
        raise AssertionError("%s: bound %s, frames %s" % (what, b.shape, zero.shape))
    if not np.isfinite(b).all():
        raise AssertionError("%s: %d element(s) without a finite bound" % (what, int((~np.isfinite(b)).sum())))
    is0 = b == 0.0
    want = np.broadcast_to(zero[..., None], b.shape)
    if not np.array_equal(is0, want) or (b < 0).any():
        raise AssertionError("%s: %d element(s) of live frames with bound 0, %d of all-zero frames with a positive one"
                             % (what, int((is0 & ~want).sum()), int((~is0 & want).sum())))


def ratios(got, ref, b):
    """``|got - ref| / bound`` per element (0 where the bound is 0 and the value is +0.0) after the refusals: a shape
    mismatch, a NaN or an infinity, a negative value (-0.0 included), anything but +0.0 where the bound is 0."""
    got = np.asarray(got)
    ref = np.asarray(ref, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if got.shape != ref.shape or ref.shape != b.shape:
        raise AssertionError("shape %s, reference %s, bound %s" % (got.shape, ref.shape, b.shape))
    if not np.isfinite(got).all():
        raise AssertionError("%d value(s) are NaN or infinite" % int((~np.isfinite(got)).sum()))
    if (np.signbit(got)).any():
        raise AssertionError("%d value(s) are negative (or -0.0)" % int(np.signbit(got).sum()))
    pinned = b == 0.0
    if (got[pinned] != 0).any():
        raise AssertionError("%d value(s) of all-zero frames are not +0.0" % int((got[pinned] != 0).sum()))
    g = got.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(pinned, 0.0, np.abs(g - ref) / np.where(pinned, 1.0, b))


def check(got, ref, b, what="", limit=1.0):
    """Assert the refusals of :func:`ratios` and ``|got - ref| <= limit * bound`` everywhere; returns the worst ratio."""
    r = ratios(got, ref, b)
    worst = float(r.max()) if r.size else 0.0
    if worst > limit:
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
        over = r > limit
        frames = np.argwhere(over.any(axis=-1))[:, -1] if r.ndim >= 2 else np.zeros(0, int)
        raise AssertionError("%s: %d element(s) over %.3g x their bound; worst ratio %.3g at %s: got %.9g, reference %.9g, "
                             "bound %.3g; failing frames by frame %% 16: %s; failing bins mod 32: %s"
                             % (what or "power spectrum", int(over.sum()), limit, worst, idx, float(np.asarray(got)[idx]),
                                float(np.asarray(ref)[idx]), float(np.asarray(b)[idx]),
                                np.bincount(frames % 16, minlength=16).tolist(),
                                np.bincount(np.argwhere(over)[:, -1] % 32, minlength=32).tolist()))
    return worst


def measure(wav_pcm):
    """{config: (worst ratio of the fp32 restatement at C_SPEC = 1, kind)} over :func:`input_list` and FRAMINGS."""
    table = {}

    def worst_of(x, nfft, hop, L, pad_mode, halo, names):
        ref = reference(x, nfft, hop, L, pad_mode=pad_mode, halo=halo)
        r = ratios(restatement_f32(x, nfft, hop, L, pad_mode=pad_mode, halo=halo), ref, bound(ref, 1.0))
        per_ch = r.reshape(len(x), -1).max(axis=1)
        k = int(np.argmax(per_ch))
        return float(per_ch[k]), names[k % len(names)]

    for nfft, hop, L in CONFIGS:
        x = input_list(nfft, hop, L, wav_pcm)
        found = [worst_of(x, nfft, hop, L, pad_mode, halo, KINDS) for pad_mode, halo in FRAMINGS]
        if nfft == 512:                      # the fused kernel's shapes: the steady-state batch as an MI355X gets it
            _, frames, nch = steady_shape(MI355X_CUS)
            found.append(worst_of(batch_inputs(nfft, hop, L, wav_pcm, nch, frames), nfft, hop, L, "notebook", 0, KINDS))
        if (nfft, hop, L) == (512, 170, 512):
            found.append(worst_of(np.asarray(wav_pcm)[None, :], nfft, hop, L, "notebook", 0, ["golden wav"]))
        table[(nfft, hop, L)] = max(found)
    return table


def c_spec_from(table):
    worst = max(v for v, _ in table.values())
    c = 1.0
    while c < 2.0 * worst:
        c *= 2.0
    return min(c, C_SPEC_CAP)
