"""float64 reference and per-element error bound of the log-mel output (``output="logmel"``) -- test infrastructure.

The reference is the notebook's own log-mel stage (:func:`oracle.mfcc_float.mfcc_notebook`, ``stages["logmel"]``,
``audio_log.T``) on the sample stream whose notebook framing gives the kernel's frames (STREAM padding and the
``halo`` sample built as :mod:`oracle.error_bound` builds them).  The bound is that module's per-coefficient bound with
the identity as the "DCT" basis: with an fp32 DCT model it is ``dL_b + 9 u |L_b|`` per band, where ``dL_b`` carries
the FFT and mel-contraction error of the declared model through the log (see BF16X2_MEL_EXTRA for the bf16 kernels).

One fixed absolute term is added for the log itself.  The relative term ``9 u |L_b|`` vanishes where the band energy is
near 1 (L_b near 0), but ``v_log_f32`` -- what both ``__builtin_amdgcn_logf`` and the device ``log2f`` become -- is an
approximation documented by the ISA to about one ULP of its result's binade near 1.0, i.e. an absolute error of order
2^-23 there, and the rounding of the fp32 argument adds 2^-24 / ln 2.  ``LOG2_ABS = 2^-21`` covers both with margin.  It
is the same for every kernel and every test, and is not tuned per input.

The bound is per band.  A structurally empty band -- a filter row without any weight, which uncommon sample rates give
(88.2 kHz and up at 512 / 32; VGGish's bank on 48 kHz audio) -- is -inf in every frame; ``eb.bound_from_stages`` would
read each frame as all-zero and give up the whole row.  :func:`bound_from_stages` here pins only that band's column to
the oracle's -inf and bounds the other bands as if the empty one were not there; :func:`assert_not_blind` is the cap on
what a bound may give up.  tests/framed_ref.py and tests/melbank_ref.py bound their log-mel rows through it too.
"""
import numpy as np

from oracle import error_bound as eb
from oracle import mfcc_float as mf

LOG2_ABS = 2.0 ** -21

# The two twelve-wave kernels contract the mel filters on bf16 x 2-split operands.  oracle.error_bound charges that
# contraction 2^-17 of the band energy; its own analysis puts the dropped terms at up to 1.5 x 2^-17 of each product, and
# the matrix instruction's accumulation of the split products adds its own rounding, which the model does not carry.
# Behind the DCT these errors average out over 32 bands; a log-mel value sees its band's error undiluted (the golden
# wav: up to 2.05 x 2^-17 on 4 of 33 472 values).  So the log-mel bound of those kernels charges a further 2^-16 of
# the band energy -- 2^-16 / ln 2 in log2 -- for every input alike.
BF16X2_MEL_EXTRA = 2.0 ** -16 / np.log(2.0)

# declared arithmetic of the log-mel forms: the mel contraction of the kernel, an "fp32 DCT" (the identity)
MODEL = {
    "mfcc_fused512_w12_kernel": "bf16x2/fp32",
    "mfcc_fused1024_w12bf_kernel": "bf16x2/fp32",
    "mfcc_float_generic_kernel": "fp32/fp32",
}


def empty_bands(filters):
    """Boolean (n_mel,): the structurally empty bands of a bank -- filter rows whose weights are all zero (the notebook's
    integer filter points coincide, or an HTK triangle falls between two bins).  Such a band's energy is 0 in every frame
    and every arithmetic: its log-mel column is the oracle's -inf."""
    return ~(np.asarray(filters) != 0).any(axis=1)


def bound_from_stages(st, model):
    """(frames, n_mel) log-mel bound from the float64 stages of one channel: ``eb.bound_from_stages`` with the identity
    as the DCT basis, plus LOG2_ABS and the bf16 x 2 charge.  A structurally empty band pins its own column to the
    oracle's -inf (bound NaN in that column only); every other band keeps the bound it would have without it: the empty
    rows leave ``filters``, ``mel``, ``logmel`` and the basis before ``eb.bound_from_stages`` -- which would read the
    band as an all-zero frame and give up the whole row -- and their columns come back afterwards.  All-zero frames
    still pin the whole row.  With no empty band this is the plain call, value for value."""
    extra = BF16X2_MEL_EXTRA if eb.MODELS[model][0] == "bf16x2" else 0.0
    empty = empty_bands(st["filters"])
    live = ~empty
    n_live = int(live.sum())
    if empty.any():
        st = dict(st, filters=np.asarray(st["filters"])[live], mel=np.asarray(st["mel"])[:, live],
                  logmel=np.asarray(st["logmel"])[:, live])
    with np.errstate(invalid="ignore"):          # inf x 0 of the identity basis: only in rows the bound leaves open
        b = eb.bound_from_stages(dict(st, dct_basis=np.eye(n_live)), model, n_live) + LOG2_ABS + extra
    if not empty.any():
        return b
    full = np.full((len(b), len(empty)), np.nan)
    full[:, live] = b
    return full


def assert_not_blind(bound, filters, what=""):
    """The not-blind condition of a log-mel bound (..., frames, n_mel) on inputs without digital silence -- a cap, not a
    tolerance: every element of every non-empty band has a finite bound, and the elements without one are exactly
    frames x empty bands.  A bound that fails this would let a kernel return anything in the elements it gave up."""
    b = np.asarray(bound).reshape(-1, np.shape(bound)[-1])
    open_ = ~np.isfinite(b)
    want = np.broadcast_to(empty_bands(filters)[None, :], b.shape)
    if not np.array_equal(open_, want):
        raise AssertionError("%s: %d element(s) of non-empty bands without a finite bound, %d of empty bands with one"
                             % (what or "log-mel bound", int((open_ & ~want).sum()), int((~open_ & want).sum())))


def roundoff_zero_weights(n_mel, n_cep, tol=1e-12):
    """The (k, b) pairs of the DCT basis with ``|D[k, b]| < tol``: float64 roundoff of an exact zero of
    ``cos(pi k (2 b + 1) / (2 n_mel))``, i.e. ``k (2 b + 1)`` an odd multiple of ``n_mel``.  Listed from the basis itself.
    With an empty band ``b`` the oracle's coefficient ``k`` is ``-inf x roundoff``: its sign, or NaN, is not the
    operation's.  None at 16 or 32 filters; at 40 the pairs with ``k (2 b + 1)`` in {40, 120, 200, ...}."""
    D = mf.dct_basis(n_mel, n_mel)[:n_cep]
    return [(int(k), int(b)) for k, b in np.argwhere(np.abs(D) < tol)]


def free_roundoff_coefficients(bound, filters, n_cep):
    """``bound`` (frames, n_cep) of a cepstral reference on a bank with empty bands, with +inf (unconstrained, see
    ``eb.ratios``) in the columns ``k`` that have a roundoff-zero weight on an empty band.  Nothing else changes."""
    empty = empty_bands(filters)
    ks = sorted({k for k, b in roundoff_zero_weights(len(empty), n_cep) if empty[b]})
    if ks:
        bound = np.array(bound, dtype=np.float64)
        bound[..., ks] = np.inf
    return bound


def reference_and_bound(pcm, model, pad_mode="notebook", halo=0, **notebook_kw):
    """(ref, bound), float64 (channels?, frames, n_mel), for int16 ``pcm`` of shape (n,) or (channels, n)."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 2:
        rb = [reference_and_bound(c, model, pad_mode, halo, **notebook_kw) for c in pcm]
        return np.stack([r for r, _ in rb]), np.stack([b for _, b in rb])
    nfft = notebook_kw.get("nfft", 512)
    hop = notebook_kw.get("hop", 170)
    n_mel = notebook_kw.get("n_mel", 32)
    x, drop = eb._frames_source(pcm, nfft, hop, pad_mode, halo)
    _, st = mf.mfcc_notebook(x, return_stages=True, **notebook_kw)
    st = dict(st, power=st["power"][drop:], mel=st["mel"][drop:], logmel=st["logmel"][drop:])
    ref = np.asarray(st["logmel"], dtype=np.float64)
    if len(ref) == 0:
        return ref.reshape(0, n_mel), np.zeros((0, n_mel))
    return ref, bound_from_stages(st, model)


def check(got, pcm, kernel, what="", **kw):
    """eb.check of ``got`` against the log-mel reference of ``pcm`` under ``kernel``'s model; returns the worst ratio."""
    ref, bound = reference_and_bound(pcm, MODEL[kernel], **kw)
    return eb.check(got, ref, bound, what or kernel)
