"""Host-side mirror of the reference's interface for the MFCC hot path.

The reference exposes this path two ways and both are mirrored here, names and argument
meaning kept:

* ``MFCC(width=16, nfft=512, samplerate=16e3, nfilters=16, nceptrums=16)`` -- the nMigen core's
  constructor, ``mfcc/core/mfcc.py:20-21`` (stream in: ``sink``, stream out: ``source``, ``reset``).
  Here the streams become whole arrays: :meth:`MFCC.process` (float contract, fp32 on the GPU)
  and :meth:`MFCC.process_fixed` (RTL-exact int16).
* ``mfcc_open / mfcc_convert(sess, path_in, path_out) / mfcc_close`` -- the host driver,
  ``software/main.c:36,100,53``, plus the directory walker ``show_dir_content`` (:206-247).

Everything numerical happens in libmfcc_hip.so (HIP kernels); this module only marshals
buffers.  Without a GPU :class:`MFCC` construction raises ``MfccHipError(NOT_FOUND)``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import MfccHipError, Params, ptr

PAD_NOTEBOOK = _lib.PAD_NOTEBOOK
PAD_STREAM = _lib.PAD_STREAM
_PAD = {"notebook": PAD_NOTEBOOK, "stream": PAD_STREAM, PAD_NOTEBOOK: PAD_NOTEBOOK, PAD_STREAM: PAD_STREAM}
_IMPL = {"auto": _lib.IMPL_AUTO, "generic": _lib.IMPL_GENERIC, "fused512": _lib.IMPL_FUSED512}
_OUTPUT = {"cepstra": _lib.OUTPUT_CEPSTRA, "logmel": _lib.OUTPUT_LOGMEL}
_NORMALIZE = {None: _lib.NORMALIZE_NONE, "none": _lib.NORMALIZE_NONE, "mean": _lib.NORMALIZE_MEAN,
              "meanvar": _lib.NORMALIZE_MEAN_VAR}


# sample_format -> (enum mfcc_hip_sample_format, the dtype a sample array must have)
_SAMPLE = {"s16": (_lib.SAMPLE_S16, np.int16), "ulaw": (_lib.SAMPLE_ULAW, np.uint8), "alaw": (_lib.SAMPLE_ALAW, np.uint8),
           "u8": (_lib.SAMPLE_U8, np.uint8), "i2s32": (_lib.SAMPLE_I2S32, np.int32), "s32": (_lib.SAMPLE_S32, np.int32),
           "f32": (_lib.SAMPLE_F32, np.float32)}


def _sample_args(sample_format):
    """(name, enum value, NumPy dtype) of a sample format, or ValueError."""
    if not isinstance(sample_format, str) or sample_format not in _SAMPLE:
        raise ValueError("sample_format must be one of %s, not %r" % (", ".join(repr(k) for k in _SAMPLE), sample_format))
    code, dtype = _SAMPLE[sample_format]
    return sample_format, code, np.dtype(dtype)


def normalize_mode(mode) -> int:
    """``None`` / ``"none"``, ``"mean"`` or ``"meanvar"`` -> ``enum mfcc_hip_normalize``."""
    try:
        return _NORMALIZE[mode]
    except (KeyError, TypeError):
        raise ValueError("normalize must be None, 'mean' or 'meanvar', not %r" % (mode,)) from None


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_f32(v):
    """A real number that is still finite as the float the ABI takes."""
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and \
        abs(float(v)) <= float(np.finfo(np.float32).max)


def _delta_args(order, window, orders=(0, 1, 2)):
    """(order, window) as ints, or ValueError: order in ``orders``, window 1..8 (MFCC_HIP_MAX_DELTA_WINDOW)."""
    if not _is_int(order) or int(order) not in orders:
        raise ValueError("deltas must be one of %s, not %r" % (orders, order))
    if not _is_int(window) or not 1 <= int(window) <= _lib.MAX_DELTA_WINDOW:
        raise ValueError("delta_window must be 1..%d, not %r" % (_lib.MAX_DELTA_WINDOW, window))
    return int(order), int(window)


_VAD = {None: _lib.VAD_OFF, "off": _lib.VAD_OFF, "select": _lib.VAD_SELECT}


def _vad_args(mode=None, column=0, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0,
              proportion_threshold=0.6, width=None):
    """(mode, column, energy_threshold, energy_mean_scale, frames_context, proportion_threshold) for
    mfcc_hip_set_vad / mfcc_hip_vad_dev, or ValueError: mode ``None`` or ``"select"``, column an int >= 0 (below
    ``width`` when given), a finite threshold, a finite scale >= 0, context 0..64 (MFCC_HIP_MAX_VAD_CONTEXT),
    0 < proportion < 1.  The defaults are Kaldi's compute-vad-energy."""
    try:
        m = _VAD[mode]
    except (KeyError, TypeError):
        raise ValueError("vad must be None or 'select', not %r" % (mode,)) from None
    if not _is_int(column) or int(column) < 0 or (width is not None and int(column) >= int(width)):
        raise ValueError("vad_column must be an int in 0..%s, not %r" % ("width - 1" if width is None else width - 1,
                                                                         column))
    if not _is_f32(energy_threshold):
        raise ValueError("vad_energy_threshold must be a finite number, not %r" % (energy_threshold,))
    if not _is_f32(energy_mean_scale) or energy_mean_scale < 0:
        raise ValueError("vad_energy_mean_scale must be a finite number >= 0, not %r" % (energy_mean_scale,))
    if not _is_int(frames_context) or not 0 <= int(frames_context) <= _lib.MAX_VAD_CONTEXT:
        raise ValueError("vad_frames_context must be 0..%d, not %r" % (_lib.MAX_VAD_CONTEXT, frames_context))
    if not _is_f32(proportion_threshold) or not 0.0 < float(np.float32(proportion_threshold)) < 1.0:
        raise ValueError("vad_proportion_threshold must lie strictly between 0 and 1, not %r" % (proportion_threshold,))
    return (m, int(column), float(energy_threshold), float(energy_mean_scale), int(frames_context),
            float(proportion_threshold))


PCEN_DEFAULTS = dict(s=0.025, alpha=0.98, delta=2.0, r=0.5, eps=1e-6)      # Wang et al. 2017; mfcc_hip_pcen_defaults


def pcen_smoothing(time_constant, samplerate, hop) -> float:
    """librosa.pcen's smoother coefficient of a time constant in seconds: ``(sqrt(1 + 4 t^2) - 1) / (2 t^2)`` with
    ``t = time_constant * samplerate / hop``."""
    t = float(time_constant) * float(samplerate) / float(hop)
    return (math.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def _pcen_args(pcen=None, samplerate=16000, hop=170, **kw):
    """``struct mfcc_hip_pcen`` of ``pcen`` (``True``: the defaults; a dict of ``s`` or ``time_constant``, ``alpha``,
    ``delta``, ``r``, ``eps``; keywords on top of it), ``None`` for ``None`` / ``False``, or ValueError: real numbers
    that stay finite as fp32, ``0 < s <= 1``, ``0 <= alpha <= 1``, ``delta >= 0``, ``0 < r <= 1``, ``eps > 0``."""
    if pcen is None or pcen is False:
        if kw:
            raise ValueError("PCEN parameters %s without pcen" % sorted(kw))
        return None
    if pcen is True:
        pcen = {}
    if not isinstance(pcen, dict):
        raise ValueError("pcen must be None, True or a dict of parameters, not %r" % (pcen,))
    a = dict(pcen, **kw)
    unknown = sorted(set(a) - set(PCEN_DEFAULTS) - {"time_constant"})
    if unknown:
        raise ValueError("unknown PCEN parameters %s (known: s, time_constant, alpha, delta, r, eps)" % unknown)
    if "time_constant" in a:
        tc = a.pop("time_constant")
        if "s" in a:
            raise ValueError("pcen takes s or time_constant, not both")
        if not _is_f32(tc) or not float(tc) > 0.0:
            raise ValueError("pcen time_constant must be a finite number of seconds > 0, not %r" % (tc,))
        a["s"] = pcen_smoothing(tc, samplerate, hop)
    v = dict(PCEN_DEFAULTS, **a)
    for k in PCEN_DEFAULTS:
        if not _is_f32(v[k]):
            raise ValueError("pcen %s must be a finite number, not %r" % (k, v[k]))
    f = {k: float(np.float32(v[k])) for k in PCEN_DEFAULTS}              # the values the library sees
    if not 0.0 < f["s"] <= 1.0:
        raise ValueError("pcen s must lie in (0, 1], not %r" % (v["s"],))
    if not 0.0 <= f["alpha"] <= 1.0:
        raise ValueError("pcen alpha must lie in [0, 1], not %r" % (v["alpha"],))
    if not f["delta"] >= 0.0:
        raise ValueError("pcen delta must be >= 0, not %r" % (v["delta"],))
    if not 0.0 < f["r"] <= 1.0:
        raise ValueError("pcen r must lie in (0, 1], not %r" % (v["r"],))
    if not f["eps"] > 0.0:
        raise ValueError("pcen eps must be > 0 (as fp32), not %r" % (v["eps"],))
    p = _lib.Pcen()
    p.struct_size = C.sizeof(_lib.Pcen)
    p.s, p.alpha, p.delta, p.r, p.eps = f["s"], f["alpha"], f["delta"], f["r"], f["eps"]
    return p


def pcen_constants(pcen=True, samplerate=16000, hop=170, **kw):
    """``(decay[128], a, delta_r)`` of mfcc_hip_pcen_constants: the fp32 constants of the tile form.  No GPU needed."""
    p = _pcen_args(pcen, samplerate, hop, **kw)
    if p is None:
        raise ValueError("pcen_constants needs parameters")
    decay = np.empty(_lib.PCEN_TILE, dtype=np.float32)
    a, dr = C.c_float(), C.c_float()
    _lib.check(_lib.load().mfcc_hip_pcen_constants(C.byref(p), ptr(decay), C.byref(a), C.byref(dr)),
               "pcen_constants")
    return decay, np.float32(a.value), np.float32(dr.value)


_MIN_WINDOW = 100                  # default minimum window of the causal form (Kaldi's --min-cmn-window)


def _window_args(window, min_window=_MIN_WINDOW, center=True):
    """(window, min_window, center) as ints for mfcc_hip_set_normalize_window, or ValueError.  ``window`` None: off,
    (0, 1, 1).  Otherwise 1 <= min_window <= window <= 16 384 (MFCC_HIP_MAX_NORMALIZE_WINDOW); a ``min_window`` left
    at its default is clamped to ``window``."""
    if isinstance(center, bool) or (_is_int(center) and int(center) in (0, 1)):
        center = int(center)
    else:
        raise ValueError("normalize_center must be True or False, not %r" % (center,))
    if window is None:
        return 0, 1, center
    if not _is_int(window) or not 1 <= int(window) <= _lib.MAX_NORMALIZE_WINDOW:
        raise ValueError("normalize_window must be None or 1..%d, not %r" % (_lib.MAX_NORMALIZE_WINDOW, window))
    if not _is_int(min_window):
        raise ValueError("normalize_min_window must be an int, not %r" % (min_window,))
    window, min_window = int(window), int(min_window)
    if min_window == _MIN_WINDOW:
        min_window = min(min_window, window)
    if not 1 <= min_window <= window:
        raise ValueError("normalize_min_window must be 1..normalize_window (%d), not %r" % (window, min_window))
    return window, min_window, center


_WINDOWS = {"hamming": _lib.WINDOW_HAMMING, "hann": _lib.WINDOW_HANN, "povey": _lib.WINDOW_POVEY,
            "blackman": _lib.WINDOW_BLACKMAN, "rectangular": _lib.WINDOW_RECTANGULAR}
_WINDOW_NAMES = {v: k for k, v in _WINDOWS.items()}


def _preemph_pair(preemph):
    """``(num, den)`` of a pre-emphasis coefficient: a ``(num, den)`` tuple of integers as it is, a float ``x`` as
    ``Fraction(x).limit_denominator(128)`` -- ``ValueError`` when that fraction is further than 1e-9 from ``x`` or when
    ``num + den > 255``, asking for a tuple.  The range itself (``0 <= num <= den``, ``den >= 1``) is checked here too,
    with words; the library reduces the pair by its gcd."""
    if isinstance(preemph, (tuple, list)):
        if len(preemph) != 2 or not all(_is_int(v) for v in preemph):
            raise ValueError("preemph must be a number or a (num, den) pair of integers, not %r" % (preemph,))
        num, den = int(preemph[0]), int(preemph[1])
    else:
        if isinstance(preemph, bool) or not isinstance(preemph, (int, float, np.integer, np.floating)) \
                or not np.isfinite(preemph):
            raise ValueError("preemph must be a number or a (num, den) pair of integers, not %r" % (preemph,))
        from fractions import Fraction
        x = float(preemph)
        fr = Fraction(x).limit_denominator(128)
        if abs(float(fr) - x) > 1e-9 or fr.numerator + fr.denominator > _lib.MAX_PREEMPH_SUM:
            raise ValueError("preemph=%r is no fraction num / den with den <= 128 and num + den <= %d: give the "
                             "(num, den) pair to use, e.g. (32, 33) or (97, 100)" % (preemph, _lib.MAX_PREEMPH_SUM))
        num, den = fr.numerator, fr.denominator
    if den < 1 or num < 0 or num > den or num + den > _lib.MAX_PREEMPH_SUM:
        raise ValueError("preemph (%d, %d): need 0 <= num <= den, den >= 1 and num + den <= %d"
                         % (num, den, _lib.MAX_PREEMPH_SUM))
    return num, den


def make_front(window="hamming", window_periodic=True, preemph=31 / 32) -> _lib.Front:
    """``struct mfcc_hip_front`` of the front arguments of :class:`MFCC`: the window function (``"hamming"``, ``"hann"``,
    ``"povey"``, ``"blackman"``, ``"rectangular"``, or the integer of ``enum mfcc_hip_window``), its periodic
    (``True``) or symmetric form, and the pre-emphasis coefficient as a float or a ``(num, den)`` pair.  The defaults
    are the reference's front."""
    if isinstance(window, str):
        if window not in _WINDOWS:
            raise ValueError("window must be one of %s, not %r" % (sorted(_WINDOWS), window))
        kind = _WINDOWS[window]
    elif _is_int(window) and int(window) in _WINDOW_NAMES:
        kind = int(window)
    else:
        raise ValueError("window must be one of %s, not %r" % (sorted(_WINDOWS), window))
    if not isinstance(window_periodic, (bool, np.bool_)):
        raise ValueError("window_periodic must be True or False, not %r" % (window_periodic,))
    num, den = _preemph_pair(preemph)
    f = _lib.Front()
    f.struct_size = C.sizeof(_lib.Front)
    f.window, f.symmetric, f.preemph_num, f.preemph_den = kind, 0 if window_periodic else 1, num, den
    return f


def make_params(nfft=512, hop=None, nfilters=32, nceptrums=13, samplerate=16000, pad_mode="notebook",
                power_scale=512.0, lifter=0.0, device=-1, impl="auto", output="cepstra", window="hamming",
                window_periodic=True, preemph=31 / 32) -> Params:
    """``output``: ``"cepstra"`` (rows of ``nceptrums`` DCT-II coefficients) or ``"logmel"`` (rows of ``nfilters``
    log2 mel band energies, the stage before the DCT; float path only, no lifter).  ``window``, ``window_periodic``,
    ``preemph``: the front (:func:`make_front`), which the C parameter block does not hold: it travels as the
    ``front`` attribute of the result, for the ``_fronted`` calls."""
    lib = _lib.load()
    front = make_front(window, window_periodic, preemph)
    p = Params()
    p.front = front
    _lib.check(lib.mfcc_hip_default_params(C.byref(p)))
    p.nfft = int(nfft)
    p.hop = 0 if hop is None else int(hop)          # 0 -> nfft // 3 (mfcc/core/mfcc.py:43)
    p.n_mel = int(nfilters)
    p.n_cep = int(nceptrums)
    p.sample_rate = int(samplerate)
    p.pad_mode = _PAD[pad_mode]
    p.power_scale = float(power_scale) if power_scale else 0.0
    p.lifter = float(lifter)
    p.device = int(device)
    p.float_impl = _IMPL[impl] if isinstance(impl, str) else int(impl)
    p.output = _OUTPUT[output] if isinstance(output, str) else int(output)
    return p


def _win_length(win_length, nfft, hop) -> int:
    """The effective frame length of ``win_length`` (``None``: ``nfft``), checked like ``mfcc_hip_create_framed`` does:
    ``hop <= win_length <= nfft`` and ``win_length >= 2``, with ``hop=None`` meaning ``nfft // 3``."""
    nfft = int(nfft)
    if win_length is None:
        return nfft
    if not _is_int(win_length):
        raise ValueError("win_length must be an integer or None, not %r" % (win_length,))
    win_length = int(win_length)
    hop = nfft // 3 if hop is None or int(hop) == 0 else int(hop)
    if win_length < 2 or win_length > nfft:
        raise ValueError("win_length must be 2..nfft (%d), not %d" % (nfft, win_length))
    if win_length < hop:
        raise ValueError("win_length (%d) must not be below hop (%d): samples between frames would be skipped"
                         % (win_length, hop))
    return win_length


_MEL = {"notebook": _lib.MEL_NOTEBOOK, "htk": _lib.MEL_HTK}


def _mel_bank(mel, fmin, fmax, samplerate, nfilters):
    """``(mel, fmin, effective fmax, MelBank)`` of the bank arguments (the edges rounded to fp32, as the library holds
    them and ``mfcc_hip_mel_bank_of`` returns them), checked like ``mfcc_hip_create_banked`` does:
    ``"notebook"`` takes no band edges (``fmax`` is reported as ``samplerate / 2``, where its points end); ``"htk"``
    needs ``0 <= fmin < fmax <= samplerate / 2`` (``fmax=None``: ``samplerate / 2``) and 1..64 filters."""
    def number(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("%s must be a finite number, not %r" % (what, v))
        return float(v)
    if mel not in _MEL:
        raise ValueError("mel must be 'notebook' or 'htk', not %r" % (mel,))
    nyquist = float(int(samplerate)) / 2.0
    # the bank holds its edges as fp32 (struct mfcc_hip_mel_bank): the checks and the attributes use what it will hold
    fmin = float(np.float32(number(fmin, "fmin")))
    top = nyquist if fmax is None else float(np.float32(number(fmax, "fmax")))
    bank = _lib.MelBank()
    bank.struct_size = C.sizeof(_lib.MelBank)
    bank.kind = _MEL[mel]
    if mel == "notebook":
        if fmin != 0.0 or fmax is not None:
            raise ValueError("the notebook bank has no band edges (fmin=%r, fmax=%r): use mel='htk'" % (fmin, fmax))
        return mel, 0.0, nyquist, bank
    if not 0.0 <= fmin < top <= nyquist:
        raise ValueError("need 0 <= fmin < fmax <= samplerate / 2 (%g), not fmin=%g, fmax=%g" % (nyquist, fmin, top))
    if fmax is not None and top == 0.0:
        raise ValueError("fmax must be positive, not %r" % (fmax,))
    if not 1 <= int(nfilters) <= 64:
        raise ValueError("an htk bank has 1..64 filters, not %r" % (nfilters,))
    bank.low_hz = fmin
    bank.high_hz = 0.0 if fmax is None else top
    return mel, fmin, top, bank


_CENTER = {None: _lib.CENTER_OFF, False: _lib.CENTER_OFF, "off": _lib.CENTER_OFF, True: _lib.CENTER_REFLECT,
           "reflect": _lib.CENTER_REFLECT, "zeros": _lib.CENTER_ZEROS}
_CENTER_NAMES = {_lib.CENTER_OFF: None, _lib.CENTER_REFLECT: "reflect", _lib.CENTER_ZEROS: "zeros"}


def center_mode(center) -> int:
    """``None`` / ``False`` / ``True`` / ``"reflect"`` / ``"zeros"`` -> ``enum mfcc_hip_center``, or ValueError."""
    if isinstance(center, (bool, str, type(None))) and center in _CENTER:
        return _CENTER[center]
    raise ValueError("center must be None, False, True, 'reflect' or 'zeros', not %r" % (center,))


def center_geometry(n_samples, mode, params, win_length) -> tuple:
    """``(frames, left pad, padded samples)`` of ``n_samples`` under centring (include/mfcc_hip.h; host only)."""
    f, left, padded = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.load().mfcc_hip_center_geometry(C.byref(params), int(win_length), center_mode(mode), int(n_samples),
                                                    C.byref(f), C.byref(left), C.byref(padded)), "center_geometry")
    return int(f.value), int(left.value), int(padded.value)


def num_frames(n_samples, win_length=None, center=None, **kw) -> int:
    """Frames a stream of ``n_samples`` yields (host-only; `nframes`, software/main.c:95); ``win_length``: the frame
    length of a framed handle (``MFCC(win_length=...)``), ``None`` = ``nfft``; ``center``: as for :class:`MFCC`
    (``1 + n_samples // hop`` frames, none for a signal too short to reflect)."""
    lib = _lib.load()
    L = _win_length(win_length, kw.get("nfft", 512), kw.get("hop"))
    p = make_params(**kw)
    if center_mode(center) != _lib.CENTER_OFF:
        return center_geometry(n_samples, center, p, L)[0]
    out = C.c_size_t(0)
    _lib.check(lib.mfcc_hip_num_frames_framed(C.byref(p), L, int(n_samples), C.byref(out)), "num_frames")
    return int(out.value)


def spectrum_bins(**kw) -> int:
    """Width of a ``MFCC.power_spectrum`` row for ``make_params(**kw)``: ``nfft // 2 + 1`` (host-only)."""
    p = make_params(**kw)
    out = C.c_size_t(0)
    _lib.check(_lib.load().mfcc_hip_spectrum_bins(C.byref(p), C.byref(out)), "spectrum_bins")
    return int(out.value)


_FBANK_SCALES = {"energy": _lib.FBANK_ENERGY, "log2": _lib.FBANK_LOG2, "ln": _lib.FBANK_LN, "log10": _lib.FBANK_LOG10}


def htk_filterbank(n_bands, nfft=512, samplerate=16000, fmin=0.0, fmax=None) -> np.ndarray:
    """The HTK-style mel matrix of ``MFCC(mel="htk")`` for 1..128 bands: float32 ``(n_bands, nfft // 2 + 1)``, triangles
    on the mel axis ``1127 ln(1 + f / 700)`` between ``fmin`` and ``fmax`` (default: ``samplerate / 2``), no area
    normalisation (host-only).  What ``MFCC.set_filterbank`` takes; up to 64 bands it is ``get_table`` of an HTK handle
    bit for bit."""
    if float(samplerate) != int(samplerate):
        raise ValueError("samplerate must be an integer, not %r" % (samplerate,))
    lib = _lib.load()
    n = C.c_size_t(0)
    args = (int(nfft), int(samplerate), int(n_bands), float(fmin), 0.0 if fmax is None else float(fmax))
    _lib.check(lib.mfcc_hip_htk_weights(*args, None, 0, C.byref(n)), "htk_filterbank")
    out = np.empty(n.value, dtype=np.float32)
    _lib.check(lib.mfcc_hip_htk_weights(*args, ptr(out), out.size, C.byref(n)), "htk_filterbank")
    return out.reshape(int(n_bands), int(nfft) // 2 + 1)


def _fbank_args(weights, scale, floor, bins):
    """``(struct mfcc_hip_fbank, contiguous float32 (n_bands, bins) host array)`` of ``MFCC.set_filterbank``'s arguments,
    or ValueError / TypeError: the checks the library makes too, with words."""
    if _is_torch(weights):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights)
    if w.dtype.kind not in "fiu":
        raise TypeError("weights must be a real array, not %s" % w.dtype)
    w = np.ascontiguousarray(w, dtype=np.float32)
    if w.ndim != 2 or w.shape[1] != bins:
        raise ValueError("weights must have shape (n_bands, %d), not %s" % (bins, w.shape))
    if not 1 <= w.shape[0] <= _lib.MAX_FBANK_BANDS:
        raise ValueError("n_bands must be 1..%d, not %d" % (_lib.MAX_FBANK_BANDS, w.shape[0]))
    if not np.isfinite(w).all() or bool((w < 0).any()):
        raise ValueError("every weight must be finite and not negative")
    if scale not in _FBANK_SCALES:
        raise ValueError("scale must be one of %s, not %r" % (sorted(_FBANK_SCALES), scale))
    floor = float(floor)
    if not 0.0 <= floor <= float(np.finfo(np.float32).max):
        raise ValueError("floor must be finite and >= 0, not %r" % (floor,))
    p = _lib.Fbank()
    p.struct_size = C.sizeof(_lib.Fbank)
    p.n_bands, p.scale, p.floor = w.shape[0], _FBANK_SCALES[scale], floor
    return p, w


_TABLE_DTYPES = {
    _lib.TABLE_WINDOW_F32: np.float32, _lib.TABLE_MEL_POINTS_I32: np.int32,
    _lib.TABLE_MEL_DENSE_F32: np.float32, _lib.TABLE_DCT_F32: np.float32,
    _lib.TABLE_FX_CURVE_I32: np.int32, _lib.TABLE_FX_TWIDDLE_I32: np.int32,
    _lib.TABLE_FX_MEL_DENSE_U32: np.uint32,
}


def get_table(which, win_length=None, mel="notebook", fmin=0.0, fmax=None, **kw) -> np.ndarray:
    """The constant tables as the library's host code builds them (works without a GPU).  ``win_length``: the frame
    length of a framed handle; only the window table depends on it (``nfft`` floats, zeros from ``win_length`` on) and
    on the front (``window``, ``window_periodic``; ``preemph`` is validated and does not enter the table).
    ``mel``, ``fmin``, ``fmax``: the bank of the handle (``MFCC(mel=...)``); the dense mel table depends on it, and an
    ``"htk"`` bank has neither filter points nor a fixed-point table (``UNSUPPORTED``)."""
    L = _win_length(win_length, kw.get("nfft", 512), kw.get("hop"))
    bank = _mel_bank(mel, fmin, fmax, kw.get("samplerate", 16000), kw.get("nfilters", 32))[3]
    lib = _lib.load()
    p = make_params(**kw)
    n = C.c_size_t(0)
    front = C.byref(p.front)
    _lib.check(lib.mfcc_hip_get_table_fronted(C.byref(p), L, C.byref(bank), front, which, None, 0, C.byref(n)), "get_table")
    buf = np.empty(n.value, dtype=np.uint8)
    _lib.check(lib.mfcc_hip_get_table_fronted(C.byref(p), L, C.byref(bank), front, which, ptr(buf), buf.nbytes, C.byref(n)))
    return buf.view(_TABLE_DTYPES[which])


def window(kind, length, periodic=True) -> np.ndarray:
    """The window function ``kind`` (``"hamming"``, ``"hann"``, ``"povey"``, ``"blackman"``, ``"rectangular"``) over
    ``length`` samples (2..1024) as the library builds it: float32 ``(length,)``, periodic or symmetric (host-only).  What
    ``MFCC(window=kind, window_periodic=periodic, win_length=length)`` multiplies a frame by."""
    if not _is_int(length) or not 2 <= int(length) <= 1024:
        raise ValueError("length must be an integer 2..1024, not %r" % (length,))
    length = int(length)
    nfft = 64
    while nfft < length:
        nfft *= 2
    # hop 1: any frame length up to nfft is a valid framing
    return get_table(_lib.TABLE_WINDOW_F32, win_length=length, nfft=nfft, hop=1, window=kind,
                     window_periodic=periodic)[:length].copy()


def _is_torch(x):
    return type(x).__module__.startswith("torch")


# ---- what every entry point does to its arrays in front of the library call: one helper per job
def _offsets(offsets, what, of, n=None, limit=None, unit=1, ordered=True, limit_from=1):
    """``offsets`` (segment, utterance or line ``u`` = entries ``u``, ``u + 1``) as a contiguous 1-D uint64 array, or
    ValueError: not 1-D, no entry (``n`` given: not ``n + 1`` entries), decreasing, or the last one times ``unit`` beyond
    ``limit`` (the size of ``of``).  ``ordered=False`` leaves the order unchecked: the segment passes hand a decreasing
    list to the library (``INVALID_PARAM``), ``process_packed`` checks it on the lengths it needs anyway.
    ``limit_from=2`` (the segment passes) holds only a list with a segment to the limit: one entry reads nothing."""
    a = np.ascontiguousarray(offsets, dtype=np.uint64)
    if a.ndim != 1 or (len(a) < 1 if n is None else len(a) != n + 1):
        raise ValueError("%s must be 1-D with %s entries" % (what, "n + 1 (n >= 0)" if n is None else n + 1))
    if ordered and bool((a[1:] < a[:-1]).any()):
        raise ValueError("%s must not decrease" % what)
    if limit is not None and len(a) >= limit_from and int(a[-1]) * unit > limit:
        raise ValueError("%s run past the end of %s" % (what, of))
    return a


def _shape_offsets(shape):
    """The offsets of the rows of a ``(frames, width)`` tensor, one segment, or of a ``(channels, frames, width)`` one,
    a segment per channel."""
    nseg, per = (int(shape[0]), int(shape[1])) if len(shape) == 3 else (1, int(shape[0]))
    return np.arange(nseg + 1, dtype=np.uint64) * np.uint64(per)


def _length_offsets(lengths):
    """``[0, l0, l0 + l1, ...]`` of a sequence of lengths."""
    a = np.zeros(len(lengths) + 1, dtype=np.uint64)
    if len(lengths):
        a[1:] = np.cumsum(lengths, dtype=np.uint64)
    return a


def _indices(idx, n_all):
    """The index list of a ``flush`` / ``reset``: ``(uint64 array, its length)``, or ``(None, n_all)`` for ``None`` = all."""
    if idx is None:
        return None, n_all
    s = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
    return s, len(s)


def _host_samples(x, sample_format, what, ndim=None):
    """``x`` as a contiguous NumPy array, or TypeError: the dtype is not the one of ``sample_format``, or (``ndim``
    given) the rank is not ``ndim``."""
    x = np.ascontiguousarray(x)
    dtype = np.dtype(_SAMPLE[sample_format][1])
    if x.dtype != dtype or (ndim is not None and x.ndim != ndim):
        want, got = (dtype.name, x.dtype) if ndim is None else ("%d-D %s" % (ndim, dtype.name), "%d-D %s" % (x.ndim, x.dtype))
        if sample_format == "s16":
            raise TypeError("%s must be %s (the core's sink is signed 16 bit, mfcc.py:29)" % (what, want))
        raise TypeError("%s must be %s for sample_format=%r, not %s" % (what, want, sample_format, got))
    return x


def _out(like, out, want, dtype, make):
    """``out`` checked -- shape ``want`` (``None`` in it: any capacity), dtype, contiguous, on the device of ``like`` --
    or, without one, what ``make()`` returns.  The kernels get raw pointers: anything else would be an out-of-bounds write."""
    if out is None:
        return make()
    shape = tuple(out.shape)
    fits = shape == want or (len(shape) == len(want) and all(w is None or w == n for w, n in zip(want, shape)))
    if not fits or out.dtype != dtype or not out.is_contiguous() or out.device != like.device:
        shape = "(%s)" % ", ".join("capacity" if w is None else str(w) for w in want) if None in want else str(want)
        raise ValueError("out must be a contiguous %s tensor of shape %s on %s"
                         % (str(dtype).split(".")[-1], shape, like.device))
    return out


def _numpy_if(from_numpy, *tensors):
    """The results of a call whose input was a NumPy array: NumPy arrays as well (one copy out)."""
    return tuple(t.cpu().numpy() for t in tensors) if from_numpy else tensors


class _Owner:
    """Owns one object of the library: a subclass names the attribute that holds its pointer and the entry point that
    destroys it."""
    _ptr = _destroy = None

    def close(self):
        # either order is safe: a handle closed first is kept alive by the library until its last session / bank / gate goes
        if getattr(self, self._ptr, None):
            getattr(self._lib, self._destroy)(getattr(self, self._ptr))
        setattr(self, self._ptr, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class MFCC(_Owner):
    """``MFCC(width=16, nfft=512, samplerate=16e3, nfilters=16, nceptrums=16)`` -- same
    constructor arguments as ``mfcc/core/mfcc.py:20-21``; extra keyword arguments select the
    host driver's framing (``pad_mode``), the float path's power scale / lifter and the device.

    ``hop`` defaults to ``nfft // 3`` like the core (``mfcc.py:43``); the notebook and the host
    driver hard-code 170 for nfft 512, which is the same number.

    ``win_length=L`` frames the audio the way speech front ends do: frame ``f`` is samples ``[f * hop, f * hop + L)``,
    multiplied by the periodic Hamming window of length ``L`` and zero-padded to ``nfft`` -- a 25 ms window advancing by
    10 ms at 16 kHz is ``MFCC(nfft=512, hop=160, win_length=400, ...)``.  ``hop <= L <= nfft``; ``None`` (and ``nfft``)
    is the reference's framing.  Frame counts, sessions and banks count ``L`` samples per frame; :attr:`win_length` is
    always the effective length.  Float path only: the fixed-point entries raise ``UNSUPPORTED`` when ``L < nfft``.

    ``mel="htk"`` replaces the notebook's filterbank (integer filter points between 0 and ``samplerate / 2``) by the
    HTK / Kaldi style one: ``nfilters`` triangles equally spaced on the mel axis ``1127 ln(1 + f / 700)`` between
    ``fmin`` and ``fmax`` Hz (``None``: ``samplerate / 2``), evaluated at the bin frequencies, no area normalisation
    (include/mfcc_hip.h has the contract).  Kaldi's 23 bands from 20 Hz are ``MFCC(nfft=512, hop=160, win_length=400,
    nfilters=23, nceptrums=13, mel="htk", fmin=20)``.  :attr:`mel`, :attr:`fmin` and :attr:`fmax` hold the effective
    bank.  Float path only, like ``win_length``; sessions, banks and the post-passes take the rows as they are.

    ``output="logmel"`` makes every float entry point return rows of ``nfilters`` log2 mel band energies
    (the notebook's ``audio_log.T``, -inf for a silent band) instead of ``nceptrums`` cepstra; the width of a
    row is :attr:`num_features` either way.  The fixed-point path and ``convert`` refuse such a handle.

    ``normalize="mean"`` / ``"meanvar"`` standardizes every channel / utterance of every float result over its own
    frames, column by column (CMVN: ``sklearn.preprocessing.scale`` of the reference's ``software/genlibrosa.py``;
    -inf / NaN of silent frames are left out and left as they are) -- ``process``, ``process_batch`` and
    ``process_packed``.  ``process_fixed``, :meth:`stream`, ``convert*`` and ``halo=1`` then raise ``UNSUPPORTED``.

    ``deltas=1`` / ``2`` appends the first (and second) time derivatives to every float row, ``[s | D | DD]``, over
    ``delta_window`` frames on each side (1..8, default 2; HTK's regression formula, indices clamped to the channel /
    utterance).  The static part is what the handle returns with deltas off, normalization included, and
    :attr:`num_features` counts the expanded width.  The same entry points as normalization refuse such a handle.

    ``vad="select"`` drops the frames an energy VAD calls unvoiced (Kaldi's compute-vad-energy and select-voiced-frames:
    ``vad_energy_threshold + vad_energy_mean_scale * mean`` of column ``vad_column`` of the raw rows, then at least
    ``vad_proportion_threshold`` of the frames within ``vad_frames_context`` above it; the thresholds are in this
    library's log2 units, a Kaldi value times ``1 / ln 2``).  Normalization and deltas still see every frame; the rows
    that come back are the voiced ones.  ``process`` then takes ONE utterance and returns ``(voiced, num_features)``;
    ``process_batch`` / ``process_packed`` return the shorter utterances; everything that returns a dense
    ``(channels, frames, ...)`` result, ``process_fixed``, :meth:`stream` and ``convert*`` raise ``UNSUPPORTED``.

    ``pcen=True`` or ``pcen=dict(s=... | time_constant=..., alpha=..., delta=..., r=..., eps=...)`` (with
    ``output="logmel"``) replaces the log of every band by per-channel energy normalization (Wang et al. 2017,
    ``librosa.pcen``): ``M_t = (1 - s) M_{t-1} + s E_t`` from ``M_0 = E_0`` over the channel / utterance and
    ``y = (E / (eps + M)^alpha + delta)^r - delta^r``, a silent band counting as ``E = 0``.  Defaults 0.025, 0.98, 2,
    0.5, 1e-6; ``time_constant`` is in seconds and converts like librosa's.  ``eps`` and ``delta`` are in the units of
    this handle's mel energies (they carry ``power_scale``); nothing is rescaled.  It runs before normalization and
    deltas, the VAD still decides on the raw rows; the entry points a normalizing handle refuses refuse it too.

    ``sample_format`` is what a sample array holds: ``"s16"`` (int16, the default: nothing changes), ``"ulaw"`` /
    ``"alaw"`` (G.711 bytes, uint8), ``"u8"`` (offset binary, uint8), ``"i2s32"`` (int32 I2S words as the reference's
    receiver cuts them: bits 25..10), ``"s32"`` (int32 full scale) or ``"f32"`` (float32 in [-1, 1), rounded to
    nearest even and saturated).  The samples are decoded to int16 on the device in front of the kernels
    (include/mfcc_hip.h has every rule, :func:`decode` applies them alone) and every method -- ``process``,
    ``process_fixed``, ``process_batch``, ``process_packed``, :meth:`stream`, :meth:`stream_bank` -- then REQUIRES the
    matching dtype (``TypeError`` otherwise) and returns, bit for bit, what an ``"s16"`` handle returns on the decoded
    samples.  ``convert*`` keep reading 16-bit WAV files.

    ``input_rate`` (an integer number of samples per second, e.g. 8000 on a 16 kHz handle) is the rate the sample
    arrays of the one-shot methods are at: they are converted to ``samplerate`` on the device, behind the decode and in
    front of the kernels, by the integer polyphase rule of include/mfcc_hip.h (:func:`resample` applies it alone), and
    every method returns, bit for bit, what the handle without it returns on the resampled samples -- every channel and
    every utterance on its own.  ``None``, 0 or ``samplerate`` itself: off.  ``process(..., halo=1)``, :meth:`stream` and
    :meth:`stream_bank` raise ``UNSUPPORTED`` on such a handle (live lines go through :meth:`resampler`); ``convert*``
    expect WAV files of that rate.

    ``center`` (``None`` / ``False``: off; ``True`` / ``"reflect"``; ``"zeros"``) is the framing of ``librosa.stft``,
    ``torch.stft``, ``torchaudio.transforms.MelSpectrogram`` and Whisper's log-mel (``center=True``): frame ``t`` is
    centred on sample ``t * hop``, the edges of every channel / utterance are reflected (or zero-padded) and ``n``
    samples give ``1 + n // hop`` frames.  The padding is done on the device, behind decode and resample and in front of
    the kernels (include/mfcc_hip.h has the rule, :func:`center_pad` applies it alone), and every one-shot float method
    returns, bit for bit, what the handle without it returns on the padded samples.  A signal of at most
    ``ceil(win_length / 2)`` samples cannot be reflected and gives no frames.  :meth:`stream`, :meth:`stream_bank`,
    :meth:`resampler`, ``process_fixed`` and ``halo=1`` raise ``UNSUPPORTED`` on such a handle, and so does
    ``pad_mode="stream"`` with ``center``.

    ``window`` (``"hamming"``, ``"hann"``, ``"povey"``, ``"blackman"``, ``"rectangular"``), ``window_periodic`` and
    ``preemph`` are the handle's front: the window function over the frame, in its periodic (``True``: denominator
    ``win_length``) or symmetric (``win_length - 1``) form, and the pre-emphasis ``y[i] = x[i] - preemph x[i-1]``.
    ``preemph`` is a float or an exact ``(num, den)`` pair of integers with ``0 <= num <= den`` and ``num + den <= 255``
    (a float becomes ``Fraction(x).limit_denominator(128)`` and must be that fraction to 1e-9); 0 switches it off.  The
    defaults are the reference's, Hamming / periodic / 31/32, and give today's bits.  torchaudio / librosa style:
    ``window="hann", preemph=0``; Kaldi style: ``window="povey", window_periodic=False, preemph=(32, 33)`` -- (32, 33) is
    the pair next to 0.97 that the fused kernels serve (``num + den <= 127``); the exact ``(97, 100)`` runs the generic
    kernels.  :attr:`front` reads the effective front back.  Float path only: the fixed-point entries raise
    ``UNSUPPORTED`` on any other front than the default.
    """

    deltas, delta_window = 0, 2                 # the state after mfcc_hip_create
    vad = None
    sample_format = "s16"
    input_rate = None
    center = None
    _ptr, _destroy = "_h", "mfcc_hip_destroy"

    def _sample_np(self):
        """The NumPy dtype a sample array of this handle must have."""
        return np.dtype(_SAMPLE[self.sample_format][1])

    def _samples_dev_ok(self, t):
        """Whether a torch tensor is a CUDA(HIP) tensor of the handle's sample dtype."""
        import torch
        return t.is_cuda and t.dtype == getattr(torch, self._sample_np().name)

    def _dev_what(self):
        return "CUDA(HIP) %s" % self._sample_np().name

    def __init__(self, width=16, nfft=512, samplerate=16e3, nfilters=16, nceptrums=16, *, hop=None,
                 pad_mode="notebook", power_scale=512.0, lifter=0.0, device=-1, impl="auto", output="cepstra",
                 normalize=None, deltas=0, delta_window=2, normalize_window=None, normalize_min_window=_MIN_WINDOW,
                 normalize_center=True, vad=None, vad_column=0, vad_energy_threshold=5.0, vad_energy_mean_scale=0.5,
                 vad_frames_context=0, vad_proportion_threshold=0.6, win_length=None, mel="notebook", fmin=0.0,
                 fmax=None, pcen=None, sample_format="s16", input_rate=None, window="hamming", window_periodic=True,
                 preemph=31 / 32, center=None):
        if width != 16:
            raise ValueError("only width=16 (int16 PCM) is supported, like every reference target")
        center_mode(center)
        fmt_name, fmt_code, _ = _sample_args(sample_format)
        _pcen_args(pcen, samplerate, hop or int(nfft) // 3)
        self.win_length = _win_length(win_length, nfft, hop)
        self.mel, self.fmin, self.fmax, bank = _mel_bank(mel, fmin, fmax, samplerate, nfilters)
        norm = normalize_mode(normalize)
        _window_args(normalize_window, normalize_min_window, normalize_center)
        order, dwindow = _delta_args(deltas, delta_window)
        vad_args = _vad_args(vad, vad_column, vad_energy_threshold, vad_energy_mean_scale, vad_frames_context,
                             vad_proportion_threshold)
        self.width = width
        self.nfft = int(nfft)
        self.samplerate = samplerate
        self.nfilters = int(nfilters)
        self.nceptrums = int(nceptrums)
        self._lib = _lib.load()
        self._params = make_params(nfft=nfft, hop=hop, nfilters=nfilters, nceptrums=nceptrums,
                                   samplerate=int(samplerate), pad_mode=pad_mode, power_scale=power_scale,
                                   lifter=lifter, device=device, impl=impl, output=output, window=window,
                                   window_periodic=window_periodic, preemph=preemph)
        self.hop = self._params.hop or self.nfft // 3
        self.output = "logmel" if self._params.output == _lib.OUTPUT_LOGMEL else "cepstra"
        h = _lib.Handle()
        self._device_index = None
        if int(device) < 0:
            # "the current device" is resolved NOW, by the library, from torch's current device
            try:
                import torch
                if torch.cuda.is_available():
                    self._device_index = torch.cuda.current_device()
            except ImportError:
                pass
        _lib.check(self._lib.mfcc_hip_create_fronted(C.byref(self._params), self.win_length, C.byref(bank),
                                                     C.byref(self._params.front), C.byref(h)), "mfcc_hip_create")
        self._h = h
        if fmt_code != _lib.SAMPLE_S16:
            self.set_sample_format(fmt_name)
        if input_rate is not None:
            self.set_input_rate(input_rate)
        if center_mode(center) != _lib.CENTER_OFF:
            self.set_center(center)
        self.pcen = None
        if pcen is not None and pcen is not False:
            self.set_pcen(pcen)
        self.normalize = None
        if norm != _lib.NORMALIZE_NONE:
            self.set_normalize(normalize)
        self.deltas, self.delta_window = 0, dwindow
        if order:
            self.set_deltas(order, dwindow)
        self.normalize_window, self.normalize_min_window, self.normalize_center = None, _MIN_WINDOW, True
        if normalize_window is not None:
            self.set_normalize_window(normalize_window, normalize_min_window, normalize_center)
        self.vad = None
        (self.vad_column, self.vad_energy_threshold, self.vad_energy_mean_scale, self.vad_frames_context,
         self.vad_proportion_threshold) = _vad_args()[1:]
        if vad_args[0] != _lib.VAD_OFF:
            self.set_vad(vad, vad_column, vad_energy_threshold, vad_energy_mean_scale, vad_frames_context,
                         vad_proportion_threshold)

    @property
    def front(self):
        """``(window, window_periodic, (num, den))`` as the handle holds them (``mfcc_hip_front_of``): the pair reduced."""
        f = _lib.Front()
        _lib.check(self._lib.mfcc_hip_front_of(self._h, C.byref(f)), "front_of")
        return _WINDOW_NAMES[f.window], not f.symmetric, (int(f.preemph_num), int(f.preemph_den))

    def set_sample_format(self, sample_format):
        """What the sample arrays of every call after this one hold (``"s16"``, ``"ulaw"``, ``"alaw"``, ``"u8"``,
        ``"i2s32"``, ``"s32"``, ``"f32"``); ``BUSY`` while sessions or banks of this handle live."""
        name, code, _ = _sample_args(sample_format)
        _lib.check(self._lib.mfcc_hip_set_sample_format(self._h, code), "set_sample_format")
        self.sample_format = name

    def _own_rate(self):
        """``samplerate`` as the integer the resampler needs, or ``INVALID_PARAM``."""
        if float(self.samplerate) != int(self.samplerate):
            raise MfccHipError(_lib.ERROR_INVALID_PARAM, "a sample-rate conversion needs an integer samplerate, not %r"
                               % (self.samplerate,))
        return int(self.samplerate)

    def set_input_rate(self, input_rate):
        """The rate the sample arrays of every call after this one are at (``None``, 0 or ``samplerate``: the handle's own,
        no conversion); ``BUSY`` while sessions, banks or gates of this handle live, ``UNSUPPORTED`` for a ratio
        :func:`resample` refuses."""
        rate = 0 if input_rate is None else input_rate
        if rate != 0:
            rate = _rate(rate, "input_rate")
            self._own_rate()
        _lib.check(self._lib.mfcc_hip_set_input_rate(self._h, rate), "set_input_rate")
        self.input_rate = int(self._lib.mfcc_hip_input_rate(self._h)) or None

    def set_center(self, center):
        """The framing of every one-shot float call after this one: ``None`` / ``False`` (frame ``t`` starts at sample
        ``t * hop``), ``True`` / ``"reflect"`` or ``"zeros"`` (frame ``t`` is centred on it, the edges padded);
        ``BUSY`` while sessions, banks or gates of this handle live, ``UNSUPPORTED`` on a ``pad_mode="stream"`` handle."""
        _lib.check(self._lib.mfcc_hip_set_center(self._h, center_mode(center)), "set_center")
        self.center = _CENTER_NAMES[int(self._lib.mfcc_hip_center(self._h))]

    def set_vad(self, mode, column=0, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0,
                proportion_threshold=0.6):
        """The handle's frame selection for every float call after this one: ``None`` (every frame) or ``"select"``
        (the voiced frames only, by Kaldi's energy rule on column ``column`` of the raw rows)."""
        a = _vad_args(mode, column, energy_threshold, energy_mean_scale, frames_context, proportion_threshold)
        _lib.check(self._lib.mfcc_hip_set_vad(self._h, *a), "set_vad")
        self.vad = "select" if a[0] == _lib.VAD_SELECT else None
        (self.vad_column, self.vad_energy_threshold, self.vad_energy_mean_scale, self.vad_frames_context,
         self.vad_proportion_threshold) = a[1:]

    def _segments(self, rows, frame_offsets):
        """The checks :meth:`normalize_rows` makes on ``rows`` and the segment offsets as a uint64 array."""
        import torch
        if rows.dtype != torch.float32 or not rows.is_cuda or not rows.is_contiguous() or rows.dim() not in (2, 3):
            raise TypeError("rows must be a contiguous 2-D or 3-D CUDA(HIP) float32 tensor")
        if frame_offsets is None:
            return _shape_offsets(rows.shape)
        # a decreasing list is the library's to refuse; one entry is no segment: nothing is read, whatever it says
        return _offsets(frame_offsets, "frame_offsets", "rows", limit=rows.numel(), unit=int(rows.shape[-1]),
                        ordered=False, limit_from=2)

    def vad_rows(self, rows, frame_offsets=None, column=0, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0,
                 proportion_threshold=0.6, out=None):
        """The energy VAD decision on a CUDA float32 tensor of RAW static rows, on the current torch stream: a uint8
        tensor of ``rows.shape[:-1]``, 1 where the frame is voiced.  ``rows`` and the segments as in
        :meth:`normalize_rows`; ``width`` 1..64, independent of this handle's own rows.  Entries of ``out`` outside the
        segments are left as they are (0 in a tensor made here)."""
        import torch
        fo = self._segments(rows, frame_offsets)
        width = int(rows.shape[-1])
        a = _vad_args("select", column, energy_threshold, energy_mean_scale, frames_context, proportion_threshold,
                      width=width)
        want = tuple(rows.shape[:-1])
        make = torch.zeros if frame_offsets is not None else torch.empty
        out = _out(rows, out, want, torch.uint8, lambda: make(want, device=rows.device, dtype=torch.uint8))
        self._check_device(rows)
        self._call(rows.device, "vad_dev", self._h, ptr(rows), width, a[1], ptr(fo), len(fo) - 1, a[2], a[3], a[4], a[5],
                   ptr(out))
        return out

    def select_rows(self, rows, voiced, frame_offsets=None, out=None):
        """The rows of a CUDA float32 tensor whose ``voiced`` byte (uint8 tensor of ``rows.shape[:-1]``, e.g. from
        :meth:`vad_rows`) is not 0, packed in order: returns ``(out[:total], offsets)`` with segment ``u`` of the result
        in rows ``offsets[u]:offsets[u + 1]``.  ``rows`` and the segments as in :meth:`normalize_rows`, ``width``
        1..192.  ``out``: a ``(capacity, width)`` tensor with room for EVERY row of the segments; its rows beyond the
        total are left as they are.  Waits for the stream: the offsets depend on the data."""
        import torch
        fo = self._segments(rows, frame_offsets)
        width = int(rows.shape[-1])
        if voiced.dtype != torch.uint8 or not voiced.is_contiguous() or voiced.device != rows.device or \
                tuple(voiced.shape) != tuple(rows.shape[:-1]):
            raise ValueError("voiced must be a contiguous uint8 tensor of shape %s on %s"
                             % (tuple(rows.shape[:-1]), rows.device))
        need = int(fo[-1]) - int(fo[0])
        out = _out(rows, out, (None, width), torch.float32,
                   lambda: torch.empty((need, width), device=rows.device, dtype=torch.float32))
        self._check_device(rows)
        oo = np.zeros(len(fo), dtype=np.uint64)
        self._call(rows.device, "select_dev", self._h, ptr(rows), width, ptr(voiced), ptr(fo), len(fo) - 1, ptr(out),
                   int(out.shape[0]), ptr(oo))
        return out[:int(oo[-1])], oo

    def set_normalize_window(self, window, min_window=_MIN_WINDOW, center=True):
        """The window of the handle's normalization for every float call after this one: ``None`` (statistics over
        the whole channel / utterance) or ``window`` frames around each frame (``center``) or before it (causal, with
        at least ``min_window`` frames at the start): Kaldi's sliding-window CMVN, for long channels."""
        w, m, c = _window_args(window, min_window, center)
        _lib.check(self._lib.mfcc_hip_set_normalize_window(self._h, w, m, c), "set_normalize_window")
        self.normalize_window, self.normalize_min_window, self.normalize_center = (w or None), m, bool(c)

    def set_deltas(self, order, window=2):
        """The handle's delta order (0 = off, 1 = D, 2 = D and DD) and window for every float call after this one."""
        order, window = _delta_args(order, window)
        _lib.check(self._lib.mfcc_hip_set_deltas(self._h, order, window), "set_deltas")
        self.deltas, self.delta_window = order, window

    def deltas_rows(self, rows, frame_offsets=None, order=2, window=2, out=None):
        """Delta coefficients of a CUDA float32 tensor of static rows, on the current torch stream: returns ``out``,
        the rows expanded to ``width * (1 + order)`` ([s | D | DD]).  ``rows`` and the segments as in
        :meth:`normalize_rows`; ``width`` 1..64, independent of this handle's own rows.  Rows of ``out`` outside the
        segments are left as they are."""
        import torch
        order, window = _delta_args(order, window, orders=(1, 2))
        fo = self._segments(rows, frame_offsets)
        width = int(rows.shape[-1])
        want = tuple(rows.shape[:-1]) + (width * (1 + order),)
        out = _out(rows, out, want, torch.float32, lambda: torch.empty(want, device=rows.device, dtype=torch.float32))
        self._check_device(rows)
        self._call(rows.device, "deltas_dev", self._h, ptr(rows), width, ptr(out), ptr(fo), len(fo) - 1, order, window)
        return out

    def set_pcen(self, pcen=True, **params):
        """The handle's PCEN for every float call after this one: ``None`` / ``False`` (off), ``True`` (the paper's
        parameters) or a dict of ``s`` (or ``time_constant`` in seconds), ``alpha``, ``delta``, ``r``, ``eps``; keywords
        go on top.  Needs ``output="logmel"``.  :attr:`pcen` holds the effective parameters, or ``None``."""
        p = _pcen_args(pcen, self.samplerate, self.hop, **params)
        _lib.check(self._lib.mfcc_hip_set_pcen(self._h, C.byref(p) if p is not None else None), "set_pcen")
        self.pcen = None if p is None else dict(s=p.s, alpha=p.alpha, delta=p.delta, r=p.r, eps=p.eps)

    def pcen_rows(self, rows, frame_offsets=None, **params):
        """PCEN of a CUDA float32 tensor of log2 energies in place, on the current torch stream; returns it.  ``rows``
        and the segments as in :meth:`normalize_rows`; ``width`` 1..64, independent of this handle's own rows.  The
        parameters are :meth:`set_pcen`'s keywords (default: the paper's), not the handle's setting."""
        p = _pcen_args(True, self.samplerate, self.hop, **params)
        fo = self._segments(rows, frame_offsets)
        self._check_device(rows)
        self._call(rows.device, "pcen_dev", self._h, ptr(rows), int(rows.shape[-1]), ptr(fo), len(fo) - 1, C.byref(p))
        return rows

    def set_normalize(self, mode):
        """The handle's normalization for every float call after this one (None, ``"mean"``, ``"meanvar"``)."""
        _lib.check(self._lib.mfcc_hip_set_normalize(self._h, normalize_mode(mode)), "set_normalize")
        self.normalize = None if normalize_mode(mode) == _lib.NORMALIZE_NONE else mode

    def normalize_rows(self, rows, frame_offsets=None, mode="meanvar", window=None, min_window=_MIN_WINDOW, center=True,
                       out=None):
        """Normalize a CUDA float32 tensor of rows in place, on the current torch stream, and return it.  ``rows``:
        ``(frames, width)`` with ``frame_offsets`` (segment ``u`` = rows ``fo[u]:fo[u + 1]``, e.g. what
        :meth:`process_packed` returns) or, without them, one segment; ``(channels, frames, width)``: one segment per
        channel.  ``width`` 1..64, independent of this handle's own rows.  With a ``window`` (sliding statistics, see
        :meth:`set_normalize_window`) the pass is out of place: ``rows`` is left alone and a new tensor (or ``out``,
        same shape, not overlapping ``rows``) is returned; rows of it outside the segments are left as they are."""
        import torch
        w, m, c = _window_args(window, min_window, center)
        if not w and out is not None:
            raise ValueError("out is for the sliding form (window=...); without a window rows are normalized in place")
        fo = self._segments(rows, frame_offsets)
        width = int(rows.shape[-1])
        self._check_device(rows)
        if w:
            def make():         # a new tensor: rows the segments do not cover (and every row, for mode None) are copies of the input
                whole = frame_offsets is None and normalize_mode(mode) != _lib.NORMALIZE_NONE
                return torch.empty_like(rows) if whole else rows.clone()
            out = _out(rows, out, tuple(rows.shape), torch.float32, make)
            self._call(rows.device, "normalize_sliding_dev", self._h, ptr(rows), width, ptr(out), ptr(fo), len(fo) - 1,
                       normalize_mode(mode), w, m, c)
            return out
        self._call(rows.device, "normalize_dev", self._h, ptr(rows), width, ptr(fo), len(fo) - 1, normalize_mode(mode))
        return rows

    @property
    def num_features(self) -> int:
        """Width of an output row of the float path: ``nfilters`` for ``output="logmel"``, else ``nceptrums``; times
        ``1 + deltas``."""
        return (self.nfilters if self.output == "logmel" else self.nceptrums) * (1 + self.deltas)

    @property
    def num_bins(self) -> int:
        """Width of a ``power_spectrum`` row: ``nfft // 2 + 1``."""
        return int(self.nfft) // 2 + 1

    @property
    def num_bands(self) -> int:
        """Width of a ``filterbank`` row: the bands of the matrix ``set_filterbank`` gave, 0 without one."""
        n = C.c_size_t(0)
        _lib.check(self._lib.mfcc_hip_fbank_bands(self._h, C.byref(n)), "fbank_bands")
        return int(n.value)

    _ENTRIES = (None, "spectrum", "fbank")

    def _row(self, fixed, entry=None):
        """Width of a row.  ``entry`` names the family of entry points a call goes to, here and in ``_host``, ``_dev``
        and ``_packed``: None (``process``), ``"spectrum"`` (``power_spectrum``) or ``"fbank"`` (``filterbank``) -- the
        word between ``mfcc_hip_`` and ``_i16`` in the C names."""
        if entry not in self._ENTRIES:
            raise ValueError("unknown entry %r" % (entry,))
        if entry == "fbank":
            return self.num_filterbank_columns
        if entry == "spectrum":
            return self.num_bins
        return self.nceptrums if fixed else self.num_features

    def num_frames(self, n_samples) -> int:
        """Frames of ``n_samples`` samples of one channel or utterance (at ``input_rate`` where one is set; centred
        where ``center`` is)."""
        if self.input_rate:
            n_samples = resample_count(n_samples, self.input_rate, int(self.samplerate))
        if self.center:
            return center_geometry(n_samples, self.center, self._params, self.win_length)[0]
        out = C.c_size_t(0)
        _lib.check(self._lib.mfcc_hip_num_frames_framed(C.byref(self._params), self.win_length, int(n_samples),
                                                        C.byref(out)))
        return int(out.value)

    def kernel_name(self, fixed=False) -> str:
        return self._lib.mfcc_hip_kernel_name(self._h, int(fixed)).decode()

    def spectrum_kernel_name(self) -> str:
        """The kernel ``power_spectrum`` runs: ``mfcc_spectrum512_kernel`` or ``mfcc_spectrum_generic_kernel``."""
        return self._lib.mfcc_hip_spectrum_kernel_name(self._h).decode()

    def is_fallback(self, fixed=False) -> bool:
        """True when this parameter set runs on a generic kernel (one frame per wave, 3-6 x slower than the fused kernels
        that cover the reference's own configurations): bench.py puts it into its line as ``config.fallback``."""
        name = self.kernel_name(fixed)
        return "generic" in name or name == "mfcc_fixed_kernel"

    def set_stream(self, stream_ptr):
        """Launch on a caller-provided hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``;
        0 / None is the HIP null stream, torch's default)."""
        _lib.check(self._lib.mfcc_hip_set_stream(self._h, stream_ptr or None))

    def use_own_stream(self):
        _lib.check(self._lib.mfcc_hip_use_own_stream(self._h))

    def synchronize(self):
        _lib.check(self._lib.mfcc_hip_synchronize(self._h))

    # -- the hot path ---------------------------------------------------------------
    def _host(self, pcm, fixed, entry=None):
        pcm = _host_samples(pcm, self.sample_format, "pcm")
        squeeze = pcm.ndim == 1
        if squeeze:
            pcm = pcm[None, :]
        if pcm.ndim != 2:
            raise ValueError("pcm must be (n,) or (channels, n)")
        nch, n = pcm.shape
        nf = self.num_frames(n)
        out = np.empty((nch, nf, self._row(fixed, entry)), dtype=np.int16 if fixed else np.float32)
        got = C.c_size_t(0)
        fn = (getattr(self._lib, "mfcc_hip_%s_i16" % entry) if entry else
              self._lib.mfcc_hip_process_fixed_i16 if fixed else self._lib.mfcc_hip_process_i16)
        _lib.check(fn(self._h, ptr(pcm), n, nch, ptr(out), out.size, C.byref(got)),
                   entry if entry else "process" if not self.vad else self._DENSE_VAD)
        assert got.value == nf
        return out[0] if squeeze else out

    def _dev(self, pcm, fixed, halo, out, entry=None):
        import torch
        if not self._samples_dev_ok(pcm):
            raise TypeError("device path needs a %s tensor" % self._dev_what())
        squeeze = pcm.dim() == 1
        if squeeze:
            pcm = pcm[None, :]
        if pcm.stride(1) != 1:
            pcm = pcm.contiguous()
        nch, n_tot = pcm.shape
        if halo not in (0, 1) or n_tot < int(halo):
            raise ValueError("halo must be 0 or 1 and counted in the samples")
        n = n_tot - int(halo)
        nf = self.num_frames(n)
        self._check_device(pcm)
        odt = torch.int16 if fixed else torch.float32
        row = self._row(fixed, entry)
        want = (nf, row) if squeeze and out is not None and out.dim() == 2 else (nch, nf, row)
        out = _out(pcm, out, want, odt, lambda: torch.empty(want, device=pcm.device, dtype=odt))
        got = C.c_size_t(0)
        self._call(pcm.device, entry + "_i16_dev" if entry else
                   "process_fixed_i16_dev" if fixed else "process_i16_dev",
                   self._h, ptr(pcm), n, pcm.stride(0), nch, int(halo), ptr(out), C.byref(got),
                   what=entry + "_dev" if entry else "process_dev" if not self.vad else self._DENSE_VAD)
        if squeeze and out.dim() == 3:
            return out[0]
        return out

    _DENSE_VAD = ("process: a vad='select' handle returns a different number of rows per channel; pass one 1-D "
                  "utterance, or use process_batch / process_packed")

    def _device(self):
        """The handle's GPU as a torch device -- its tables, stream and scratch live on ONE: what the handle allocates
        or copies in goes there.  ``device=-1`` was resolved from torch's current device when the handle was made."""
        import torch
        if self._device_index is None:
            self._device_index = torch.cuda.current_device() if self._params.device < 0 else int(self._params.device)
        return torch.device("cuda", self._device_index)

    def _check_device(self, t):
        """Refuse tensors of another GPU than the handle's."""
        if t.device.index != (self._device_index if self._device_index is not None else self._device().index):
            raise ValueError("tensor on %s but this MFCC handle was created on cuda:%d" % (t.device, self._device_index))

    @contextlib.contextmanager
    def _on_torch_stream(self, device):
        """Context: launch on torch's current stream of `device`, then go back to the handle's own stream, so
        that later host-path calls do not run on (or outlive) a stream torch owns."""
        import torch
        self.set_stream(torch.cuda.current_stream(device).cuda_stream)
        try:
            yield
        finally:
            self.use_own_stream()

    def _call(self, device, name, obj, *args, what=None, ok=()):
        """``mfcc_hip_<name>(obj, *args)`` on torch's current stream of ``device``; ``obj`` is this handle's ``_h`` or the
        pointer of one of its sessions, banks or gates.  A code that is neither success nor in ``ok`` raises
        ``MfccHipError`` with ``what`` (default: the name); the code is returned."""
        with self._on_torch_stream(device):
            rc = getattr(self._lib, "mfcc_hip_" + name)(obj, *args)
        if rc not in ok:
            _lib.check(rc, what or name)
        return rc

    def process(self, pcm, halo=0, out=None):
        """Float contract: int16 PCM ``(n,)`` / ``(channels, n)`` -> float32 ``(.., frames, num_features)``.
        NumPy in -> NumPy out (H2D, kernel, D2H); torch CUDA tensor in -> torch tensor out, asynchronous
        on the current stream.  ``halo=1`` (device path): sample 0 of every channel is history only.
        On a ``vad="select"`` handle a 1-D input goes through the ragged entry as one utterance and comes back as
        ``(voiced, num_features)``; a 2-D one raises ``UNSUPPORTED``."""
        if self.vad and (pcm.dim() if _is_torch(pcm) else np.ndim(pcm)) == 1 and not halo and out is None:
            return self.process_batch([pcm])[0]
        if _is_torch(pcm):
            return self._dev(pcm, False, halo, out)
        if halo:
            raise ValueError("halo is only available on the device path")
        return self._host(pcm, False)

    def power_spectrum(self, pcm, halo=0, out=None):
        """The power spectrum every float output starts from: PCM ``(n,)`` / ``(channels, n)`` in the handle's sample
        format and rate -> float32 ``(.., frames, nfft // 2 + 1)``, row ``f`` = ``|FFT(window * preemph(frame f)) /
        power_scale|**2`` with the handle's framing and window.  NumPy in -> NumPy out; torch CUDA tensor in -> torch
        tensor out, asynchronous on the current stream, ``halo`` and ``out`` as for ``process``.  The handle's filterbank,
        output kind, normalization, deltas, PCEN and VAD do not apply: ``torch.matmul(rows, W.T)`` with any mel matrix
        ``W`` gives the band energies."""
        if _is_torch(pcm):
            return self._dev(pcm, False, halo, out, entry="spectrum")
        if halo:
            raise ValueError("halo is only available on the device path")
        if out is not None:
            raise ValueError("out is only available on the device path")
        return self._host(pcm, False, entry="spectrum")

    def power_spectrum_packed(self, flat, offsets, out=None):
        """``power_spectrum`` of a corpus that lies in HBM, as ``process_packed`` takes it: ``(rows, frame_offsets)`` with
        ``rows`` the dense ``(sum frames, nfft // 2 + 1)`` tensor, bit-identical to one ``power_spectrum`` per utterance."""
        return self._packed(flat, offsets, False, out, "spectrum")

    def set_filterbank(self, weights, scale="log2", floor=0.0, *, normalize=None, normalize_window=None,
                       normalize_min_window=_MIN_WINDOW, normalize_center=True, deltas=0, delta_window=2, pcen=None):
        """Give the handle a filter matrix for ``filterbank``: ``weights`` a NumPy array or a torch tensor of shape
        ``(n_bands, nfft // 2 + 1)``, 1..128 bands, every weight finite and not negative (copied to the host once, as
        float32); ``scale`` one of ``"energy"``, ``"log2"``, ``"ln"``, ``"log10"``; ``floor`` the log scales' floor
        (finite, >= 0; with 0 an empty band gives ``-inf``).  ``None`` removes the matrix.  Calls enqueued before keep the
        matrix they were enqueued with.

        The keywords are the matrix's own post-passes behind ``filterbank`` / ``filterbank_packed``, with the meaning and
        defaults of the handle's keywords of the same names (which still do not apply to filterbank rows): PCEN
        (``pcen``: ``True`` or a dict, ``"log2"`` only), then utterance or sliding CMVN (``normalize``,
        ``normalize_window`` ...), then deltas -- on up to 128 bands, one segment per channel or utterance, rows
        ``num_filterbank_columns = num_bands * (1 + deltas)`` wide.  Every ``set_filterbank`` replaces them (``None`` and
        a call without keywords: none).  With them ``halo=1`` and ``stream_bank(filterbank=True)`` raise
        ``UNSUPPORTED``."""
        mode = normalize_mode(normalize)
        w_, m_, c_ = _window_args(normalize_window, normalize_min_window, normalize_center)
        order, dwin = _delta_args(deltas, delta_window)
        pc = _pcen_args(pcen, self.samplerate, self.hop)
        post = mode != _lib.NORMALIZE_NONE or w_ or order or pc is not None
        if weights is None:
            if post:
                raise ValueError("filterbank post-passes need a matrix: weights=None takes no keywords")
            _lib.check(self._lib.mfcc_hip_set_fbank(self._h, None, None), "set_fbank")
            return
        if pc is not None and scale != "log2":
            raise ValueError("pcen reads log2 band energies: scale must be 'log2', not %r" % (scale,))
        p, w = _fbank_args(weights, scale, floor, self.num_bins)
        _lib.check(self._lib.mfcc_hip_set_fbank(self._h, C.byref(p), ptr(w)), "set_fbank")
        if not post:
            return                  # mfcc_hip_set_fbank has reset them
        q = _lib.FilterbankPost()
        q.struct_size = C.sizeof(_lib.FilterbankPost)
        q.normalize, q.normalize_window, q.normalize_min_window, q.normalize_center = mode, w_, m_, c_
        q.delta_order, q.delta_window = order, dwin
        if pc is not None:
            q.pcen_on, q.pcen = 1, pc
        _lib.check(self._lib.mfcc_hip_set_filterbank_post(self._h, C.byref(q)), "set_filterbank_post")

    @property
    def num_filterbank_columns(self) -> int:
        """Width of a ``filterbank`` row as the calls return it: ``num_bands * (1 + deltas)`` with the ``deltas`` of
        ``set_filterbank``; 0 without a matrix."""
        return int(self._lib.mfcc_hip_filterbank_row_width(self._h))

    def filterbank_kernel_name(self) -> str:
        """The kernel ``filterbank`` runs: ``mfcc_fbank512_kernel``, ``mfcc_fbank_generic_kernel``, or ``""`` without a
        matrix."""
        return self._lib.mfcc_hip_fbank_kernel_name(self._h).decode()

    def filterbank(self, pcm, halo=0, out=None):
        """Band energies under the matrix of ``set_filterbank``: PCM ``(n,)`` / ``(channels, n)`` in the handle's sample
        format and rate -> float32 ``(.., frames, num_bands)``, row ``f`` = ``W @ power_spectrum row f`` in the matrix's
        scale, contracted on the chip.  Arguments, device checks, streams and ``out`` as for ``power_spectrum``.  The
        handle's own filterbank, output kind, normalization, deltas, PCEN and VAD do not apply; the post-passes given to
        ``set_filterbank`` do, one segment per channel, and make the rows ``num_filterbank_columns`` wide."""
        if _is_torch(pcm):
            return self._dev(pcm, False, halo, out, entry="fbank")
        if halo:
            raise ValueError("halo is only available on the device path")
        if out is not None:
            raise ValueError("out is only available on the device path")
        return self._host(pcm, False, entry="fbank")

    def filterbank_packed(self, flat, offsets, out=None):
        """``filterbank`` of a corpus that lies in HBM, as ``power_spectrum_packed`` takes it: ``(rows, frame_offsets)``
        with ``rows`` the dense ``(sum frames, num_filterbank_columns)`` tensor, bit-identical to one ``filterbank`` per
        utterance (``set_filterbank``'s post-passes included: every utterance is a segment)."""
        return self._packed(flat, offsets, False, out, "fbank")

    def process_fixed(self, pcm, halo=0, out=None):
        """Fixed contract (RTL arithmetic): int16 PCM -> int16 coefficients, bit-exact."""
        if _is_torch(pcm):
            return self._dev(pcm, True, halo, out)
        if halo:
            raise ValueError("halo is only available on the device path")
        return self._host(pcm, True)

    def process_batch(self, utterances, fixed=False):
        """Many utterances of different lengths in ONE launch (the batched form of the driver's directory
        walk, main.c:206-247).  ``utterances``: sequence of 1-D int16 arrays.  Returns a list of
        ``(frames_u, num_features)`` arrays (views of one result buffer), bit-identical to calling
        ``process`` / ``process_fixed`` on each utterance."""
        if len(utterances) and _is_torch(utterances[0]):
            return self._batch_dev(utterances, fixed)
        if self.sample_format == "s16":
            utts = [np.ascontiguousarray(u, dtype=np.int16).reshape(-1) for u in utterances]
        else:
            utts = [_host_samples(u, self.sample_format, "utterances").reshape(-1) for u in utterances]
        n = len(utts)
        offsets = _length_offsets([u.size for u in utts])
        flat = np.concatenate(utts) if n and int(offsets[-1]) else np.zeros(0, dtype=self._sample_np())
        fo = np.zeros(n + 1, dtype=np.uint64)
        nf = sum(self.num_frames(u.size) for u in utts)
        out = np.empty((nf, self._row(fixed)), dtype=np.int16 if fixed else np.float32)
        fn = self._lib.mfcc_hip_process_ragged_fixed_i16 if fixed else self._lib.mfcc_hip_process_ragged_i16
        _lib.check(fn(self._h, ptr(flat), ptr(offsets), n, ptr(out), out.size, ptr(fo)), "process_ragged")
        assert int(fo[-1]) == nf or (self.vad and not fixed and int(fo[-1]) <= nf)
        return [out[int(fo[i]):int(fo[i + 1])] for i in range(n)]

    def _batch_dev(self, utterances, fixed):
        """``process_batch`` for torch CUDA int16 tensors: stays on the device, asynchronous on the current stream."""
        import torch
        utts = [u.reshape(-1) for u in utterances]
        if any(not self._samples_dev_ok(u) for u in utts):
            raise TypeError("device path needs %s tensors" % self._dev_what())
        n = len(utts)
        offsets = _length_offsets([u.numel() for u in utts])
        # utterances that are consecutive views of one buffer (a corpus already laid out in HBM) are used in place
        in_place = n > 0 and all(u.is_contiguous() for u in utts) and all(
            utts[i].data_ptr() + utts[i].element_size() * utts[i].numel() == utts[i + 1].data_ptr() and
            utts[i].untyped_storage().data_ptr() == utts[0].untyped_storage().data_ptr() for i in range(n - 1))
        if in_place:
            base = utts[0]
            flat = torch.as_strided(base, (int(offsets[-1]),), (1,), storage_offset=base.storage_offset())
        else:
            flat = torch.cat(utts) if int(offsets[-1]) else torch.zeros(0, dtype=utts[0].dtype, device=utts[0].device)
        out, fo = self.process_packed(flat, offsets, fixed=fixed)
        return [out[int(fo[i]):int(fo[i + 1])] for i in range(n)]

    def process_packed(self, flat, offsets, fixed=False, out=None):
        """A corpus that already lies in HBM: ``flat`` = all utterances back to back (1-D CUDA int16 tensor),
        utterance ``u`` = ``flat[offsets[u]:offsets[u + 1]]``.  ONE launch (``mfcc_hip_process_ragged_*_dev``),
        asynchronous on the current stream.  Returns ``(out, frame_offsets)``: the dense ``(sum frames, num_features)``
        result tensor and the row range of every utterance (``out[fo[u]:fo[u + 1]]``).  Equal-length utterances run
        as channels of one multi-channel launch (no packing copy); the bits are the same.  On a ``vad="select"`` handle
        ``out`` still needs room for every frame; what is returned is ``(out[:fo[-1]], fo)``, the voiced rows."""
        return self._packed(flat, offsets, fixed, out, None)

    def _packed(self, flat, offsets, fixed, out, entry):
        """``process_packed`` and ``power_spectrum_packed``: the checks, the output and the ragged device entry."""
        import torch
        if not self._samples_dev_ok(flat) or flat.dim() != 1 or not flat.is_contiguous():
            raise TypeError("flat must be a contiguous 1-D %s tensor" % self._dev_what())
        offsets = _offsets(offsets, "offsets", "flat", limit=flat.numel(), ordered=False)
        n = len(offsets) - 1
        self._check_device(flat)
        lens = np.diff(offsets.astype(np.int64))             # the order is checked here: the lengths are needed anyway
        if n and int(lens.min()) < 0:
            raise ValueError("offsets must not decrease")
        fo = np.zeros(n + 1, dtype=np.uint64)
        # this runs once per step of a sharded corpus (bench.py enqueue_us_per_step): equal lengths -- config 5 as
        # BASELINE defines it -- need one frame count, not a table of them
        if n and int(lens.min()) == int(lens.max()):
            nf = self.num_frames(int(lens[0])) * n
        else:
            uniq, counts = np.unique(lens, return_counts=True)
            nf = int(sum(self.num_frames(int(v)) * int(c) for v, c in zip(uniq, counts)))
        odt = torch.int16 if fixed else torch.float32
        row = self._row(fixed, entry)
        out = _out(flat, out, (nf, row), odt, lambda: torch.empty((nf, row), device=flat.device, dtype=odt))
        name = (entry + "_ragged_i16_dev" if entry else
                "process_ragged_fixed_i16_dev" if fixed else "process_ragged_i16_dev")
        self._call(flat.device, name, self._h, ptr(flat), ptr(offsets), n, ptr(out), out.numel(), ptr(fo),
                   what=entry + "_ragged_dev" if entry else "process_ragged_dev")
        if self.vad and not fixed and not entry:
            return out[:int(fo[-1])], fo                 # the voiced rows; the entry point has waited for the stream
        assert int(fo[-1]) == nf
        return out, fo

    def time_launches(self, pcm, out, fixed=False, warmup=2, iters=10) -> float:
        """Average kernel time in ms over ``iters`` launches, HIP events on the launch stream."""
        if pcm.dim() == 1:
            pcm = pcm[None, :]
        self._check_device(pcm)
        ms = C.c_float(0)
        self._call(pcm.device, "time_dev", self._h, int(fixed), ptr(pcm), pcm.shape[1], pcm.stride(0), pcm.shape[0], ptr(out),
                   warmup, iters, C.byref(ms))
        return float(ms.value)

    # -- online mode: the core's own interface, sink / source / reset (mfcc/core/mfcc.py:28-30) -----
    def stream(self, fixed=False) -> "MfccStream":
        """A streaming session on this handle: feed chunks, get the frames they complete."""
        return MfccStream(self, fixed)

    def stream_bank(self, n_streams, fixed=False, *, filterbank=False, normalize=None, normalize_window=None, deltas=0,
                    delta_window=2, pcen=None) -> "MfccStreamBank":
        """``n_streams`` streaming sessions on this handle that advance together: one launch per push.

        ``normalize`` (``"mean"`` / ``"meanvar"``, with ``normalize_window=N``) and ``deltas`` (1 or 2, with
        ``delta_window``) make it an ONLINE bank on a raw float handle: rows are standardized over the causal window
        ``[max(0, t - N), t + 1)`` of their own stream and expanded to ``[s | D | DD]``; row ``t`` is returned once
        row ``t + deltas * delta_window`` is known, :meth:`MfccStreamBank.flush` returns the rest.  Pushes followed
        by a flush equal ``MFCC(..., normalize=..., normalize_window=N, normalize_min_window=1,
        normalize_center=False, deltas=..., delta_window=...).process`` of the whole signal, bit for bit.

        ``pcen`` (``True`` or a dict, see :meth:`set_pcen`; a raw ``output="logmel"`` handle) runs PCEN on every
        stream's rows before that, the smoother carried from push to push: two floats per stream and band.  The
        one-shot call it equals then has ``pcen=`` the same parameters.

        ``filterbank=True`` makes the rows those of :meth:`filterbank` under the matrix the handle carries now
        (``set_filterbank``; ``UNSUPPORTED`` without one): up to 128 bands, ``num_features = num_bands * (1 + deltas)``.
        Pushes followed by a flush equal ``filterbank`` of the whole signal, bit for bit; ``normalize`` / ``deltas`` /
        ``pcen`` (a ``"log2"`` matrix) are the bank's own and work column by column as on the narrow banks, while the
        handle's own output kind, normalization, deltas, PCEN and VAD do not apply.  Float only: with ``fixed=True`` it
        raises ``ValueError``.  While such a bank lives ``set_filterbank`` raises ``BUSY``.  There is no separate session
        class: ``stream_bank(1, filterbank=True)`` is the streaming session on filterbank rows."""
        return MfccStreamBank(self, n_streams, fixed, filterbank=filterbank, normalize=normalize,
                              normalize_window=normalize_window, deltas=deltas, delta_window=delta_window, pcen=pcen)

    # -- the receiver's power gate on fixed-point rows (software/cepstrum.c:93-183; include/mfcc_hip.h) -----
    def _int16_rows_in(self, rows):
        """``(rows, False)`` for a torch tensor; a NumPy int16 array is copied to the handle's GPU: ``(the copy, True)``,
        and :func:`_numpy_if` then copies the results out."""
        if _is_torch(rows):
            return rows, False
        import torch
        rows = np.ascontiguousarray(rows)
        if rows.dtype != np.int16:
            raise TypeError("rows must be int16 (what process_fixed returns)")
        return torch.from_numpy(rows).to(self._device()), True

    def _gate_rows_in(self, rows, frame_offsets):
        """``rows`` as a contiguous CUDA int16 tensor (a NumPy array is copied in: the flag says so), its segment
        offsets as a uint64 array and the row width."""
        import torch
        rows, from_numpy = self._int16_rows_in(rows)
        if rows.dtype != torch.int16 or not rows.is_cuda or not rows.is_contiguous() or rows.dim() not in (2, 3):
            raise TypeError("rows must be a contiguous 2-D or 3-D CUDA(HIP) int16 tensor")
        width = int(rows.shape[-1])
        if not 1 <= width <= 64:
            raise ValueError("rows must be 1..64 wide, not %d" % width)
        if frame_offsets is None:
            fo = _shape_offsets(rows.shape)
        else:
            fo = _offsets(frame_offsets, "frame_offsets", "rows", limit=rows.numel(), unit=width)
        self._check_device(rows)
        return rows, fo, width, from_numpy

    def gate_rows(self, rows, frame_offsets=None, n_frames=93, stride=1, threshold=None):
        """The receiver's power gate for EVERY window of int16 rows, on the current torch stream.  ``rows``: a CUDA int16
        tensor ``(rows, n_cep)`` with ``frame_offsets`` (segment ``u`` = rows ``fo[u]:fo[u + 1]``, e.g. what
        ``process_packed(..., fixed=True)`` returns) or, without them, one segment; ``(channels, rows, n_cep)``: one
        segment per channel.  Window ``j`` of a segment is its rows ``[j * stride, j * stride + n_frames)``.  Returns
        ``(power, gate, gate_ref, win_offsets)``: per window the exact int64 sum of squares the reference's loop forms,
        ``power >= threshold`` (uint8) and the same test on the sum as the reference's 32-bit ``int`` holds it (uint8);
        segment ``u``'s windows are entries ``win_offsets[u]:win_offsets[u + 1]``.  ``threshold`` defaults to
        ``wire.POWER_THRESHOLD``.  A NumPy array goes through one copy in and one copy out."""
        import torch
        from . import wire
        nfr, st, thr = wire.gate_args(n_frames, stride, wire.POWER_THRESHOLD if threshold is None else threshold)
        rows, fo, width, from_numpy = self._gate_rows_in(rows, frame_offsets)
        wo = wire.gate_count(fo, nfr, st, offsets=True)
        n = int(wo[-1])
        power = torch.empty(n, device=rows.device, dtype=torch.int64)
        gate = torch.empty(n, device=rows.device, dtype=torch.uint8)
        gate_ref = torch.empty(n, device=rows.device, dtype=torch.uint8)
        self._call(rows.device, "gate_dev", self._h, ptr(rows), width, ptr(fo), len(fo) - 1, nfr, st, thr, ptr(power),
                   ptr(gate), ptr(gate_ref))
        return _numpy_if(from_numpy, power, gate, gate_ref) + (wo,)

    def gate_windows(self, rows, mask, frame_offsets=None, n_frames=93, stride=1, out=None):
        """The windows of ``rows`` (as in :meth:`gate_rows`) whose ``mask`` byte is not 0 -- ``mask``: uint8, one entry per
        window in the order of :meth:`gate_rows`' outputs, e.g. its ``gate`` or ``gate_ref`` -- copied whole and packed in
        order: returns ``(windows (n, n_frames, n_cep), starts, out_offsets)`` with ``starts`` (int64) the first row of
        every kept window as an index into ``rows`` (flattened to 2-D) and segment ``u``'s windows in
        ``out_offsets[u]:out_offsets[u + 1]``.  Without ``out`` a first call asks for the count
        (``MFCC_HIP_ERROR_BUFFER_SMALL`` fills the offsets) and the result is sized from it; with ``out``
        (``(capacity, n_frames, n_cep)``) too small a capacity raises that error.  Waits for the stream once: the count
        depends on the data."""
        import torch
        from . import wire
        nfr, st, _ = wire.gate_args(n_frames, stride)
        rows, fo, width, from_numpy = self._gate_rows_in(rows, frame_offsets)
        wo = wire.gate_count(fo, nfr, st, offsets=True)
        if not _is_torch(mask):
            mask = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(rows.device)
        if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.device != rows.device or \
                mask.numel() != int(wo[-1]):
            raise ValueError("mask must be a contiguous uint8 tensor of %d entries on %s" % (int(wo[-1]), rows.device))
        oo = np.zeros(len(fo), dtype=np.uint64)

        def call(o, starts, cap, ok=()):
            self._call(rows.device, "gate_windows_dev", self._h, ptr(rows), width, ptr(fo), len(fo) - 1, nfr, st, ptr(mask),
                       ptr(o), ptr(starts), cap, ptr(oo), ok=ok)

        def sized():                                    # the count is asked for: BUFFER_SMALL fills the offsets
            call(None, None, 0, ok=(_lib.ERROR_BUFFER_SMALL,))
            return torch.empty((int(oo[-1]), nfr, width), device=rows.device, dtype=torch.int16)
        out = _out(rows, out, (None, nfr, width), torch.int16, sized)
        starts = torch.empty(int(out.shape[0]), device=rows.device, dtype=torch.int64)
        call(out, starts, int(out.shape[0]))
        n = int(oo[-1])
        return _numpy_if(from_numpy, out[:n], starts[:n]) + (oo,)

    def power_gate(self, n_lines, n_cep=None, n_frames=93, stride=1, threshold=None) -> "MfccPowerGate":
        """A gate tracker for ``n_lines`` live lines on this handle: the receiver's circular window of ``n_frames`` rows
        of ``n_cep`` (default: this handle's ``nceptrums``) coefficients per line, fed with what a fixed
        :meth:`stream_bank` returns."""
        return MfccPowerGate(self, n_lines, self.nceptrums if n_cep is None else n_cep, n_frames, stride, threshold)

    def resampler(self, n_lines, in_rate, sample_format="s16") -> "MfccResampler":
        """A sample-rate converter for ``n_lines`` live lines from ``in_rate`` to this handle's ``samplerate``: chunks in
        ``sample_format`` in, int16 at ``samplerate`` out, ready for ``stream_bank(n_lines).push_packed`` of an ``"s16"``
        handle.  This handle only lends its device, stream and scratch areas: its own ``sample_format`` and
        ``input_rate`` are not read."""
        return MfccResampler(self, n_lines, in_rate, sample_format)

    # -- file level: mfcc_convert(sess, path_in, path_out), software/main.c:100-177 -----
    def convert_many(self, paths_in, paths_out, fixed=True):
        """``mfcc_convert`` for many files in one ragged launch; returns the frame count of each file."""
        n = len(paths_in)
        assert n == len(paths_out)
        a_in = (C.c_char_p * n)(*[os.fsencode(p) for p in paths_in])
        a_out = (C.c_char_p * n)(*[os.fsencode(p) for p in paths_out])
        nf = (C.c_size_t * n)()
        _lib.check(self._lib.mfcc_hip_convert_wavs(self._h, a_in, a_out, n, int(fixed), nf), "convert_wavs")
        return [int(v) for v in nf]

    def convert(self, path_in, path_out, fixed=True) -> int:
        """``x.wav -> x.mfcc``: raw int16 LE ``[frame][nceptrums]``.  Returns the frame count."""
        nf = C.c_size_t(0)
        _lib.check(self._lib.mfcc_hip_convert_wav(self._h, os.fsencode(path_in), os.fsencode(path_out),
                                                  int(fixed), C.byref(nf)), "convert %s" % path_in)
        return int(nf.value)


class MfccStream(_Owner):
    """Online mode -- the stream interface of the nMigen core (``sink`` in, ``source`` out, ``reset``;
    mfcc/core/mfcc.py:28-30,116) and of its targets (wav2mfcc.py:27-42: bit 31 = soft reset; mic2mfcc.py:19-30).
    The session keeps the core's cross-frame state on the device: one pre-emphasis history sample and the
    samples of the frame in progress.  Any chunking gives the one-shot result, frame for frame, bit for bit."""

    _ptr, _destroy = "_s", "mfcc_hip_stream_destroy"

    def __init__(self, mfcc: MFCC, fixed=False):
        self._m = mfcc
        self._lib = mfcc._lib
        self.fixed = bool(fixed)
        s = _lib.Handle()
        _lib.check(self._lib.mfcc_hip_stream_create(mfcc._h, int(self.fixed), C.byref(s)), "stream_create")
        self._s = s

    @property
    def pending(self) -> int:
        return int(self._lib.mfcc_hip_stream_pending(self._s))

    def _out(self, nf):
        return np.empty((nf, self._m._row(self.fixed)), dtype=np.int16 if self.fixed else np.float32)

    def push(self, samples) -> np.ndarray:
        """``sink``: int16 samples in; returns the ``(frames, num_features)`` they complete (possibly 0 rows)."""
        samples = _host_samples(samples, self._m.sample_format, "samples", ndim=1)
        out = self._out(int(self._lib.mfcc_hip_stream_max_frames(self._s, samples.size)))
        nf = C.c_size_t(0)
        _lib.check(self._lib.mfcc_hip_stream_push(self._s, ptr(samples), samples.size, ptr(out),
                                                  out.size, C.byref(nf)), "stream_push")
        return out[:nf.value]

    def flush(self) -> np.ndarray:
        """End of the stream: the zero-padded tail frame of the host driver (main.c:134-144) with
        ``pad_mode="stream"``, nothing with ``"notebook"``; the session is reset afterwards."""
        out = self._out(1)
        nf = C.c_size_t(0)
        _lib.check(self._lib.mfcc_hip_stream_flush(self._s, ptr(out), out.size, C.byref(nf)), "stream_flush")
        return out[:nf.value]

    def reset(self):
        """``MFCC.reset`` / ``mfcc_softreset`` (main.c:21-34): drop pending samples, history back to 0."""
        _lib.check(self._lib.mfcc_hip_stream_reset(self._s), "stream_reset")


class MfccStreamBank(_Owner):
    """``n_streams`` independent :class:`MfccStream` sessions (N live lines) whose state lives on the device and which
    advance together: one push takes one chunk per stream and runs ONE launch of the frame kernels.  Every stream gets
    the rows a session of its own would have returned for the same chunks, bit for bit.  Equal chunks (lines in
    lockstep) compute exactly the frames returned; a mixed push computes ``active streams x most frames of any``."""

    _ptr, _destroy = "_b", "mfcc_hip_bank_destroy"

    def __init__(self, mfcc: MFCC, n_streams, fixed=False, *, filterbank=False, normalize=None, normalize_window=None,
                 deltas=0, delta_window=2, pcen=None):
        self._m = mfcc
        self._lib = mfcc._lib
        self.fixed = bool(fixed)
        self.filterbank = bool(filterbank)
        if self.filterbank and self.fixed:
            raise ValueError("a filterbank bank is float only: fixed=True does not go with filterbank=True")
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError("a bank needs at least one stream")
        mode = normalize_mode(normalize)
        order, dwin = _delta_args(deltas, delta_window)
        if mode != _lib.NORMALIZE_NONE:
            if normalize_window is None:
                raise ValueError("a stream bank normalizes over the causal window [max(0, t - N), t + 1) of each "
                                 "stream only: normalize needs normalize_window=N (per-utterance statistics need the "
                                 "stream's end)")
            window = _window_args(normalize_window, 1, False)[0]
        else:
            window = 0
        p = None if pcen is None or pcen is False else _pcen_args(pcen, mfcc.samplerate, mfcc.hop)
        self.online = mode != _lib.NORMALIZE_NONE or order != 0 or normalize_window is not None or p is not None
        if self.online and self.fixed:
            raise ValueError("pcen / normalize / deltas of a stream bank are float only: fixed=True takes none of them")
        self.pcen = None if p is None else dict(s=p.s, alpha=p.alpha, delta=p.delta, r=p.r, eps=p.eps)
        self.normalize, self.normalize_window = (normalize if mode != _lib.NORMALIZE_NONE else None), (window or None)
        self.deltas, self.delta_window = order, dwin
        b = _lib.Handle()
        if self.filterbank:
            _lib.check(self._lib.mfcc_hip_bank_create_filterbank(mfcc._h, self.n_streams, None if p is None else C.byref(p), mode,
                                                            window, order, dwin, C.byref(b)), "bank_create_filterbank")
        elif p is not None:
            _lib.check(self._lib.mfcc_hip_bank_create_online_pcen(mfcc._h, self.n_streams, C.byref(p), mode, window, order,
                                                                  dwin, C.byref(b)), "bank_create_online_pcen")
        elif self.online:
            _lib.check(self._lib.mfcc_hip_bank_create_online(mfcc._h, self.n_streams, mode, window, order, dwin,
                                                             C.byref(b)), "bank_create_online")
        else:
            _lib.check(self._lib.mfcc_hip_bank_create(mfcc._h, int(self.fixed), self.n_streams, C.byref(b)),
                       "bank_create")
        self._b = b

    def __len__(self):
        return self.n_streams

    @property
    def pending(self) -> np.ndarray:
        """Samples every stream holds back for its frame in progress: uint64 ``(n_streams,)``, each below ``win_length``."""
        p = np.zeros(self.n_streams, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_bank_pending(self._b, ptr(p)), "bank_pending")
        return p

    @property
    def num_features(self) -> int:
        """Elements per row: the handle's row width (a filterbank bank: ``num_bands``) times ``1 + deltas``."""
        return int(self._lib.mfcc_hip_bank_row_width(self._b))

    @property
    def lag(self) -> int:
        """Rows a stream is behind: row ``t`` is returned once row ``t + lag`` is known (``deltas * delta_window``)."""
        return int(self._lib.mfcc_hip_bank_lag(self._b))

    @property
    def held(self) -> np.ndarray:
        """Finished rows every stream has not returned yet: uint64 ``(n_streams,)``, each at most ``lag``."""
        p = np.zeros(self.n_streams, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_bank_held(self._b, ptr(p)), "bank_held")
        return p

    def _plan(self, offsets):
        fo = np.zeros(self.n_streams + 1, dtype=np.uint64)
        pending, held = self.pending, self.held
        _lib.check(self._lib.mfcc_hip_bank_plan_online_framed(C.byref(self._m._params), self._m.win_length, self.lag,
                                                              ptr(pending), ptr(held), ptr(offsets), self.n_streams,
                                                              ptr(fo), None, None), "bank_plan_online")
        return fo

    def num_frames(self, lengths) -> np.ndarray:
        """``frame_offsets`` (rows RETURNED, the lag counted) a push of chunks of these lengths would give now (host
        only: ``mfcc_hip_bank_plan_online``, which is ``mfcc_hip_bank_plan`` on a plain bank)."""
        lengths = np.asarray(lengths, dtype=np.uint64).reshape(-1)
        if len(lengths) != self.n_streams:
            raise ValueError("one length per stream: %d, not %d" % (self.n_streams, len(lengths)))
        return self._plan(_length_offsets(lengths))

    def _row(self):
        return self.num_features

    def push(self, chunks) -> list:
        """``sink`` of every stream: ``n_streams`` 1-D int16 arrays (any may be empty).  Returns a list of
        ``(frames_u, num_features)`` arrays, the frames each stream completed (views of one buffer).  Synchronous."""
        if len(chunks) != self.n_streams:
            raise ValueError("one chunk per stream: %d, not %d" % (self.n_streams, len(chunks)))
        cs = [_host_samples(c, self._m.sample_format, "chunks", ndim=1) for c in chunks]
        n = self.n_streams
        offsets = _length_offsets([c.size for c in cs])
        flat = np.concatenate(cs) if int(offsets[-1]) else np.zeros(0, dtype=self._m._sample_np())
        nf = int(self._plan(offsets)[-1])
        out = np.empty((nf, self._row()), dtype=np.int16 if self.fixed else np.float32)
        fo = np.zeros(n + 1, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_bank_push(self._b, ptr(flat), ptr(offsets), ptr(out), out.size, ptr(fo)), "bank_push")
        assert int(fo[-1]) == nf
        return [out[int(fo[u]):int(fo[u + 1])] for u in range(n)]

    def push_packed(self, flat, offsets, out=None):
        """Chunks that already lie in HBM: ``flat`` is a 1-D CUDA int16 tensor, stream ``u`` gets
        ``flat[offsets[u]:offsets[u + 1]]``.  Asynchronous on the current torch stream, nothing is copied to the host.
        Returns ``(out, frame_offsets)``: the ``(sum frames, num_features)`` tensor and, as a uint64 array, the row range
        of every stream.  Lines in lockstep pass ``x.reshape(-1)`` with ``arange`` offsets and view the result as
        ``(n_streams, frames, num_features)``."""
        import torch
        if not self._m._samples_dev_ok(flat) or flat.dim() != 1 or not flat.is_contiguous():
            raise TypeError("flat must be a contiguous 1-D %s tensor" % self._m._dev_what())
        offsets = _offsets(offsets, "offsets", "flat", n=self.n_streams, limit=flat.numel())
        m = self._m
        m._check_device(flat)
        nf = int(self._plan(offsets)[-1])
        odt = torch.int16 if self.fixed else torch.float32
        row = self._row()
        out = _out(flat, out, (nf, row), odt, lambda: torch.empty((nf, row), device=flat.device, dtype=odt))
        fo = np.zeros(self.n_streams + 1, dtype=np.uint64)
        m._call(flat.device, "bank_push_dev", self._b, ptr(flat), ptr(offsets), ptr(out), out.numel(), ptr(fo))
        assert int(fo[-1]) == nf
        return out, fo

    def flush(self, streams=None) -> list:
        """End of the listed streams (``None``: all): per stream, in the order listed, what :meth:`MfccStream.flush`
        returns -- one zero-padded tail frame with ``pad_mode="stream"``, no row with ``"notebook"``.  An online bank
        returns the rows the stream still holds (:attr:`held`) first, with the tail frame as the stream's last row and
        the delta indices clamped there: arrays of different lengths (``mfcc_hip_bank_flush_ragged``).  They are reset
        afterwards; the other streams are not touched."""
        s, n = _indices(streams, self.n_streams)
        out = np.empty((n * (self.lag + 1), self._row()), dtype=np.int16 if self.fixed else np.float32)
        fo = np.zeros(n + 1, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_bank_flush_ragged(self._b, ptr(s), n, ptr(out), out.size, ptr(fo)), "bank_flush_ragged")
        return [out[int(fo[i]):int(fo[i + 1])] for i in range(n)]

    def reset(self, streams=None):
        """``MFCC.reset`` for the listed streams (``None``: all): drop pending samples, history back to 0."""
        s, n = _indices(streams, self.n_streams)
        _lib.check(self._lib.mfcc_hip_bank_reset(self._b, ptr(s), n), "bank_reset")


class MfccPowerGate(_Owner):
    """The receiver's circular window and power gate (``cepstrum_refill_window`` + ``cepstrum_eval_power``,
    software/cepstrum.c:93-183) for ``n_lines`` live lines, state on the device.  Window ``j`` of a line is its rows
    ``[j * stride, j * stride + n_frames)`` counted from create / reset; any chunking gives the windows, bit for bit, of
    :meth:`MFCC.gate_rows` on the line's whole row sequence."""

    _ptr, _destroy = "_g", "mfcc_hip_gate_destroy"

    def __init__(self, mfcc: MFCC, n_lines, n_cep, n_frames=93, stride=1, threshold=None):
        from . import wire
        self._m = mfcc
        self._lib = mfcc._lib
        self.n_lines = int(n_lines)
        if self.n_lines < 1:
            raise ValueError("a gate needs at least one line")
        self.n_frames, self.stride, self.threshold = wire.gate_args(
            n_frames, stride, wire.POWER_THRESHOLD if threshold is None else threshold, n_cep=n_cep)
        self.n_cep = int(n_cep)
        g = _lib.Handle()
        _lib.check(self._lib.mfcc_hip_gate_create(mfcc._h, self.n_lines, self.n_cep, self.n_frames, self.stride,
                                                  self.threshold, C.byref(g)), "gate_create")
        self._g = g

    def __len__(self):
        return self.n_lines

    @property
    def seen(self) -> np.ndarray:
        """Frames every line has received since create / reset: uint64 ``(n_lines,)`` (a host mirror)."""
        p = np.zeros(self.n_lines, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_gate_seen(self._g, ptr(p)), "gate_seen")
        return p

    def num_windows(self, frame_offsets) -> np.ndarray:
        """``win_offsets`` a push with these ``frame_offsets`` would give now (host only: ``mfcc_hip_gate_plan``)."""
        fo = _offsets(frame_offsets, "frame_offsets", "rows", n=self.n_lines)
        wo = np.zeros(self.n_lines + 1, dtype=np.uint64)
        seen = self.seen
        _lib.check(self._lib.mfcc_hip_gate_plan(self.n_frames, self.stride, ptr(seen), ptr(fo), self.n_lines, ptr(wo), None),
                   "gate_plan")
        return wo

    def push(self, rows, frame_offsets):
        """Feed every line its new rows: ``rows`` int16 ``(sum rows, n_cep)`` with line ``u``'s in
        ``rows[fo[u]:fo[u + 1]]`` -- exactly what ``MfccStreamBank.push_packed`` of a fixed bank returns.  A CUDA tensor
        is used in place, asynchronously on the current torch stream (nothing is copied to the host, nothing waits); a
        NumPy array goes through one copy in and one copy out.  Returns ``(power, gate, gate_ref, win_offsets)`` for the
        windows this push completed, line ``u``'s in entries ``win_offsets[u]:win_offsets[u + 1]``."""
        import torch
        rows, from_numpy = self._m._int16_rows_in(rows)
        if rows.dtype != torch.int16 or not rows.is_cuda or not rows.is_contiguous() or rows.dim() != 2 or \
                int(rows.shape[1]) != self.n_cep:
            raise TypeError("rows must be a contiguous CUDA(HIP) int16 tensor of shape (rows, %d)" % self.n_cep)
        fo = _offsets(frame_offsets, "frame_offsets", "rows", n=self.n_lines, limit=int(rows.shape[0]))
        self._m._check_device(rows)
        n = int(self.num_windows(fo)[-1])
        power = torch.empty(n, device=rows.device, dtype=torch.int64)
        gate = torch.empty(n, device=rows.device, dtype=torch.uint8)
        gate_ref = torch.empty(n, device=rows.device, dtype=torch.uint8)
        wo = np.zeros(self.n_lines + 1, dtype=np.uint64)
        self._m._call(rows.device, "gate_push_dev", self._g, ptr(rows), ptr(fo), ptr(power), ptr(gate), ptr(gate_ref), n,
                      ptr(wo))
        assert int(wo[-1]) == n
        return _numpy_if(from_numpy, power, gate, gate_ref) + (wo,)

    def reset(self, lines=None):
        """The listed lines (``None``: all) start again at frame 0."""
        s, n = _indices(lines, self.n_lines)
        _lib.check(self._lib.mfcc_hip_gate_reset(self._g, ptr(s), n), "gate_reset")

    def last_windows(self, lines):
        """The rows of the last completed window of every listed line: a CUDA int16 tensor
        ``(len(lines), n_frames, n_cep)`` on the current torch stream.  A line that has completed no window since
        create / reset raises ``INVALID_PARAM``."""
        import torch
        s, n = _indices(np.arange(self.n_lines) if lines is None else lines, self.n_lines)
        dev = self._m._device()
        out = torch.empty((n, self.n_frames, self.n_cep), device=dev, dtype=torch.int16)
        self._m._call(dev, "gate_window_dev", self._g, ptr(s), n, ptr(out))
        return out


class MfccResampler(_Owner):
    """The streaming form of :func:`resample` for ``n_lines`` live lines, state on the device.  A line emits its outputs
    ``H`` input samples late (``H = K / 2``); :meth:`flush` emits the rest on zeros beyond the end and restarts the
    line.  The pushes plus the flush of a line, concatenated, are :func:`resample` of its concatenated chunks, bit for
    bit, whatever the chunking."""

    _ptr, _destroy = "_r", "mfcc_hip_resampler_destroy"

    def __init__(self, mfcc: MFCC, n_lines, in_rate, sample_format="s16"):
        self._m = mfcc
        self._lib = mfcc._lib
        self.n_lines = int(n_lines)
        if self.n_lines < 1:
            raise ValueError("a resampler needs at least one line")
        self.sample_format, code, self._dtype = _sample_args(sample_format)
        self.in_rate, self.out_rate = _rate(in_rate, "in_rate"), mfcc._own_rate()
        r = _lib.Handle()
        _lib.check(self._lib.mfcc_hip_resampler_create(mfcc._h, self.n_lines, code, self.in_rate, self.out_rate, C.byref(r)),
                   "resampler_create")
        self._r = r

    def __len__(self):
        return self.n_lines

    @property
    def seen(self) -> np.ndarray:
        """Samples every line has received since create / reset / flush: uint64 ``(n_lines,)`` (a host mirror)."""
        p = np.zeros(self.n_lines, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_resampler_seen(self._r, ptr(p)), "resampler_seen")
        return p

    def plan(self, offsets=None, flush=False) -> np.ndarray:
        """``out_offsets`` a :meth:`push_packed` with these ``offsets`` would give now, or (``flush=True``) a flush of
        every line behind it (host only: ``mfcc_hip_resampler_plan``)."""
        off = None if offsets is None else _offsets(offsets, "offsets", "flat", n=self.n_lines)
        oo = np.zeros(self.n_lines + 1, dtype=np.uint64)
        seen = self.seen
        _lib.check(self._lib.mfcc_hip_resampler_plan(self.in_rate, self.out_rate, ptr(seen), ptr(off), self.n_lines, int(flush),
                                                     ptr(oo)), "resampler_plan")
        return oo

    def push_packed(self, flat, offsets):
        """One chunk per line, line ``u`` = ``flat[offsets[u]:offsets[u + 1]]`` (a contiguous 1-D CUDA tensor of the
        format's dtype; a chunk may be empty).  One launch, asynchronous on the current torch stream.  Returns ``(out,
        out_offsets)``: a CUDA int16 tensor and the range of every line in it."""
        import torch
        if not flat.is_cuda or flat.dtype != getattr(torch, self._dtype.name) or flat.dim() != 1 or not flat.is_contiguous():
            raise TypeError("flat must be a contiguous 1-D CUDA(HIP) %s tensor" % self._dtype.name)
        off = _offsets(offsets, "offsets", "flat", n=self.n_lines, limit=flat.numel())
        self._m._check_device(flat)
        n = int(self.plan(off)[-1])
        out = torch.empty(n, device=flat.device, dtype=torch.int16)
        oo = np.zeros(self.n_lines + 1, dtype=np.uint64)
        self._m._call(flat.device, "resampler_push_dev", self._r, ptr(flat), ptr(off), ptr(out), n, ptr(oo))
        assert int(oo[-1]) == n
        return out, oo

    def push(self, chunks) -> list:
        """``chunks``: one NumPy array per line (``None`` or empty: nothing for that line).  One copy in, one launch, one
        copy out; returns every line's new int16 samples."""
        import torch
        if len(chunks) != self.n_lines:
            raise ValueError("one chunk per line (%d), not %d" % (self.n_lines, len(chunks)))
        arrs = [np.zeros(0, self._dtype) if c is None else _host_samples(c, self.sample_format, "chunk", ndim=1) for c in chunks]
        off = _length_offsets([a.size for a in arrs])
        flat = torch.from_numpy(np.concatenate(arrs) if arrs else np.zeros(0, self._dtype)).to(self._m._device())
        out, oo = self.push_packed(flat, off)
        out = out.cpu().numpy()
        return [out[int(oo[u]):int(oo[u + 1])] for u in range(self.n_lines)]

    def flush_packed(self, lines=None):
        """The end of the listed lines (``None``: all): ``(out, out_offsets)`` like :meth:`push_packed`, entry ``i`` for
        ``lines[i]``; the lines start again at sample 0.  Asynchronous on the current torch stream."""
        import torch
        s, n = _indices(lines, self.n_lines)
        seen = self.seen if s is None else self.seen[s.astype(np.int64)]
        oo = np.zeros(n + 1, dtype=np.uint64)
        _lib.check(self._lib.mfcc_hip_resampler_plan(self.in_rate, self.out_rate, ptr(seen), None, n, 1, ptr(oo)),
                   "resampler_plan")
        dev = self._m._device()
        out = torch.empty(int(oo[-1]), device=dev, dtype=torch.int16)
        self._m._call(dev, "resampler_flush_dev", self._r, ptr(s), n, ptr(out), out.numel(), ptr(oo))
        return out, oo

    def flush(self, lines=None) -> list:
        """:meth:`flush_packed` to the host: the last int16 samples of every listed line."""
        out, oo = self.flush_packed(lines)
        out = out.cpu().numpy()
        return [out[int(oo[i]):int(oo[i + 1])] for i in range(len(oo) - 1)]

    def reset(self, lines=None):
        """The listed lines (``None``: all) start again at sample 0, without output."""
        s, n = _indices(lines, self.n_lines)
        _lib.check(self._lib.mfcc_hip_resampler_reset(self._r, ptr(s), n), "resampler_reset")


_decode_handles = {}          # device index -> the handle decode() launches on (mfcc_hip_decode_dev takes any)


def decode(x, sample_format, mfcc=None):
    """The int16 samples a handle with ``sample_format`` computes on, by the rules of include/mfcc_hip.h, same shape as
    ``x`` (whose dtype must be the format's: uint8, int32, float32 or int16).  A NumPy array goes through
    ``mfcc_hip_decode_host`` (no GPU needed); a CUDA tensor through ``mfcc_hip_decode_dev``, asynchronous on the current
    torch stream, on ``mfcc`` (any handle of that device) or on a handle this function keeps per device."""
    name, code, dtype = _sample_args(sample_format)
    lib = _lib.load()
    if not _is_torch(x):
        x = _host_samples(x, name, "x")
        out = np.empty(x.shape, dtype=np.int16)
        _lib.check(lib.mfcc_hip_decode_host(code, ptr(x), x.size, ptr(out)), "decode_host")
        return out
    import torch
    if not x.is_cuda or x.dtype != getattr(torch, dtype.name):
        raise TypeError("x must be a CUDA(HIP) %s tensor for sample_format=%r" % (dtype.name, name))
    x = x.contiguous()
    if mfcc is None:
        mfcc = _decode_handles.get(x.device.index)
        if mfcc is None:
            mfcc = _decode_handles[x.device.index] = MFCC(nfft=512, nfilters=32, nceptrums=13, device=x.device.index)
    mfcc._check_device(x)
    out = torch.empty(x.shape, device=x.device, dtype=torch.int16)
    mfcc._call(x.device, "decode_dev", mfcc._h, code, ptr(x), x.numel(), ptr(out))
    return out


def _rate(v, what):
    """``v`` as an int that fits the C ABI's ``int``, or TypeError / ValueError."""
    if not _is_int(v):
        raise TypeError("%s must be an integer number of samples per second, not %r" % (what, v))
    if not 0 < int(v) < 2 ** 31:
        raise ValueError("%s must be positive and below 2**31, not %r" % (what, v))
    return int(v)


def resample_count(n, in_rate, out_rate) -> int:
    """Samples :func:`resample` returns for ``n`` input samples: ``ceil(n * L / M)`` (include/mfcc_hip.h)."""
    out = C.c_size_t(0)
    _lib.check(_lib.load().mfcc_hip_resample_count(_rate(in_rate, "in_rate"), _rate(out_rate, "out_rate"), int(n), C.byref(out)),
               "resample_count")
    return int(out.value)


def resample_taps(in_rate, out_rate):
    """The Q14 tap table of a ratio, ``(L, K)`` int16: row ``p`` is phase ``p`` (include/mfcc_hip.h has the design)."""
    lib, i, o = _lib.load(), _rate(in_rate, "in_rate"), _rate(out_rate, "out_rate")
    L, K = C.c_int(0), C.c_int(0)
    _lib.check(lib.mfcc_hip_resample_geometry(i, o, C.byref(L), None, C.byref(K)), "resample_geometry")
    t = np.empty((L.value, K.value), dtype=np.int16)
    _lib.check(lib.mfcc_hip_resample_taps(i, o, ptr(t), t.size, None), "resample_taps")
    return t


def resample(x, in_rate, out_rate, mfcc=None):
    """``x`` (1-D int16 at ``in_rate`` samples per second) at ``out_rate``: the integer polyphase rule of
    include/mfcc_hip.h, the same bits on both routes.  A NumPy array goes through ``mfcc_hip_resample_host`` (no GPU
    needed); a CUDA tensor through ``mfcc_hip_resample_dev``, asynchronous on the current torch stream, on ``mfcc``
    (any handle of that device) or on a handle this function keeps per device."""
    i, o = _rate(in_rate, "in_rate"), _rate(out_rate, "out_rate")
    lib = _lib.load()
    if not _is_torch(x):
        x = _host_samples(x, "s16", "x", ndim=1)
        out = np.empty(resample_count(x.size, i, o), dtype=np.int16)
        _lib.check(lib.mfcc_hip_resample_host(i, o, ptr(x), x.size, ptr(out), out.size), "resample_host")
        return out
    import torch
    if not x.is_cuda or x.dtype != torch.int16 or x.dim() != 1:
        raise TypeError("x must be a 1-D CUDA(HIP) int16 tensor")
    x = x.contiguous()
    if mfcc is None:
        mfcc = _decode_handles.get(x.device.index)
        if mfcc is None:
            mfcc = _decode_handles[x.device.index] = MFCC(nfft=512, nfilters=32, nceptrums=13, device=x.device.index)
    mfcc._check_device(x)
    out = torch.empty(resample_count(x.numel(), i, o), device=x.device, dtype=torch.int16)
    mfcc._call(x.device, "resample_dev", mfcc._h, i, o, ptr(x), x.numel(), ptr(out), out.numel())
    return out


def center_pad(x, mode="reflect", nfft=512, hop=None, win_length=None, mfcc=None):
    """The padded signal a ``center=mode`` handle frames (include/mfcc_hip.h, "centring"): ``ceil(L / 2)`` samples in
    front and up to the end of frame ``n // hop`` behind, reflected (``"reflect"`` / ``True``) or zero (``"zeros"``);
    empty where the signal gives no frame.  A 1-D int16 NumPy array goes through ``mfcc_hip_center_host`` (no GPU needed)
    with ``nfft``, ``hop`` (``None``: ``nfft // 3``) and ``win_length``; a 1-D CUDA tensor through
    ``mfcc_hip_center_dev`` on ``mfcc``, asynchronous on the current torch stream, with that handle's framing and in
    that handle's ``sample_format`` (decoded while it is padded): int16 comes back on both routes."""
    code = center_mode(mode)
    if code == _lib.CENTER_OFF:
        raise ValueError("mode must be True, 'reflect' or 'zeros'")
    lib = _lib.load()
    if not _is_torch(x):
        x = _host_samples(x, "s16", "x", ndim=1)
        L = _win_length(win_length, nfft, hop)
        p = make_params(nfft=nfft, hop=hop)
        out = np.empty(center_geometry(x.size, mode, p, L)[2], dtype=np.int16)
        _lib.check(lib.mfcc_hip_center_host(C.byref(p), L, code, ptr(x), x.size, ptr(out), out.size, None), "center_host")
        return out
    import torch
    if mfcc is None:
        raise ValueError("center_pad of a device tensor needs mfcc=: the handle whose framing and device it uses")
    if not mfcc._samples_dev_ok(x) or x.dim() != 1:
        raise TypeError("x must be a 1-D %s tensor" % mfcc._dev_what())
    x = x.contiguous()
    mfcc._check_device(x)
    np_ = center_geometry(x.numel(), mode, mfcc._params, mfcc.win_length)[2]
    out = torch.empty(np_, device=x.device, dtype=torch.int16)
    mfcc._call(x.device, "center_dev", mfcc._h, code, _sample_args(mfcc.sample_format)[1], ptr(x), x.numel(), ptr(out),
               out.numel(), None)
    return out


def lift_file(mfcc_in, lift_out, nceptrums=32, L=22) -> int:
    """``x.mfcc -> x.lift`` like the loop of software/lift.py:28-40 (host only); returns the frame count."""
    nf = C.c_size_t(0)
    _lib.check(_lib.load().mfcc_hip_lift_file(os.fsencode(mfcc_in), os.fsencode(lift_out), int(nceptrums), float(L),
                                              C.byref(nf)), "lift_file %s" % mfcc_in)
    return int(nf.value)


# ---- software/main.c names ---------------------------------------------------------------

def mfcc_open(**kw) -> MFCC:
    """``mfcc_open`` (main.c:36): a session with the host driver's constants
    ``NFFT 512, STEPSIZE 170, NCEPSTRUMS 32, SAMPLERATE 16000`` (main.c:11-14) and its
    zero-padded tail frame (main.c:134-144)."""
    args = dict(nfft=512, samplerate=16000, nfilters=32, nceptrums=32, pad_mode="stream")
    args.update(kw)
    return MFCC(**args)


def mfcc_convert(sess: MFCC, path_in, path_out, fixed=True) -> int:
    """``mfcc_convert(sess, path_in, path_out)`` (main.c:100); 0 on success like the original."""
    sess.convert(path_in, path_out, fixed=fixed)
    return 0


def mfcc_close(sess: MFCC) -> None:
    sess.close()


def show_dir_content(sess: MFCC, path, fixed=True, batch_bytes=1 << 30):
    """Recursive ``*.wav -> *.mfcc`` walk of ``show_dir_content`` (main.c:206-247).  The files are
    converted in ragged batches -- one launch per ``batch_bytes`` of WAV data instead of one USB
    ping-pong per frame -- and the ``.mfcc`` files are byte-identical to per-file ``mfcc_convert``.
    Returns the list of (wav, mfcc) pairs converted."""
    pairs = []
    for root, _dirs, files in os.walk(path):
        for name in sorted(files):
            if name.endswith(".wav"):
                src = os.path.join(root, name)
                pairs.append((src, src[:-3] + "mfcc"))
    batch, size = [], 0
    for i, (src, dst) in enumerate(pairs):
        batch.append((src, dst))
        size += os.path.getsize(src)
        if size >= batch_bytes or i == len(pairs) - 1:
            sess.convert_many([b[0] for b in batch], [b[1] for b in batch], fixed=fixed)
            batch, size = [], 0
    return pairs


def lifter(cepstra, L=22):
    """``lifter(cepstra, L=22)`` of software/lift.py:12-26 on a ``.mfcc`` array (host-side post
    step on files; the float kernel can fold the same lifter in via ``MFCC(lifter=L)``)."""
    cepstra = np.asarray(cepstra)
    if L > 0:
        n = np.arange(cepstra.shape[1])
        return (1 + (L / 2.) * np.sin(np.pi * n / L)) * cepstra
    return cepstra
