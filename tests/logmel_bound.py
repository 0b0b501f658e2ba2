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
    st = dict(st, power=st["power"][drop:], mel=st["mel"][drop:], logmel=st["logmel"][drop:], dct_basis=np.eye(n_mel))
    ref = np.asarray(st["logmel"], dtype=np.float64)
    if len(ref) == 0:
        return ref.reshape(0, n_mel), np.zeros((0, n_mel))
    with np.errstate(invalid="ignore"):          # inf x 0 of the identity basis: only in rows the bound leaves open
        extra = BF16X2_MEL_EXTRA if eb.MODELS[model][0] == "bf16x2" else 0.0
        return ref, eb.bound_from_stages(st, model, n_mel) + LOG2_ABS + extra


def check(got, pcm, kernel, what="", **kw):
    """eb.check of ``got`` against the log-mel reference of ``pcm`` under ``kernel``'s model; returns the worst ratio."""
    ref, bound = reference_and_bound(pcm, MODEL[kernel], **kw)
    return eb.check(got, ref, bound, what or kernel)
