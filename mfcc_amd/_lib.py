"""ctypes binding of libmfcc_hip.so (include/mfcc_hip.h).  No compute happens in Python.

The library is built in-tree (``mfcc_amd/libmfcc_hip.so``) by ``__graft_entry__.build()`` /
``make -C mfcc_amd/csrc``.  If it is missing this module raises -- there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MFCC_HIP_LIB: diagnostic override for A/B runs of experimental builds of the same ABI (tools/ab.sh)
LIB_PATH = os.environ.get("MFCC_HIP_LIB") or os.path.join(_HERE, "libmfcc_hip.so")

ABI_VERSION = 2

# enum mfcc_hip_error
SUCCESS = 0
ERROR_INVALID_PARAM = -101
ERROR_NOT_FOUND = -102
ERROR_NO_MEM = -103
ERROR_BUSY = -104
ERROR_UNSUPPORTED = -105
ERROR_BUFFER_SMALL = -106
ERROR_IO = -107
ERROR_OTHER = -200

PAD_NOTEBOOK = 0
PAD_STREAM = 1

IMPL_AUTO = 0
IMPL_GENERIC = 1
IMPL_FUSED512 = 2

OUTPUT_CEPSTRA = 0
OUTPUT_LOGMEL = 1

NORMALIZE_NONE = 0
NORMALIZE_MEAN = 1
NORMALIZE_MEAN_VAR = 2

VAD_OFF = 0
VAD_SELECT = 1

MAX_DELTA_WINDOW = 8
MAX_VAD_CONTEXT = 64
MAX_NORMALIZE_WINDOW = 16384
MAX_GATE_WINDOW = 4096
POWER_THRESHOLD = 100000000

MEL_NOTEBOOK = 0
MEL_HTK = 1

# enum mfcc_hip_sample_format
SAMPLE_S16 = 0
SAMPLE_ULAW = 1
SAMPLE_ALAW = 2
SAMPLE_U8 = 3
SAMPLE_I2S32 = 4
SAMPLE_S32 = 5
SAMPLE_F32 = 6

# enum mfcc_hip_center
CENTER_OFF = 0
CENTER_REFLECT = 1
CENTER_ZEROS = 2

TABLE_WINDOW_F32 = 0
TABLE_MEL_POINTS_I32 = 1
TABLE_MEL_DENSE_F32 = 2
TABLE_DCT_F32 = 3
TABLE_FX_CURVE_I32 = 4
TABLE_FX_TWIDDLE_I32 = 5
TABLE_FX_MEL_DENSE_U32 = 6


class Params(C.Structure):
    """struct mfcc_hip_params"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nfft", C.c_int32),
        ("hop", C.c_int32),
        ("n_mel", C.c_int32),
        ("n_cep", C.c_int32),
        ("sample_rate", C.c_int32),
        ("pad_mode", C.c_int32),
        ("power_scale", C.c_float),
        ("lifter", C.c_float),
        ("device", C.c_int32),
        ("float_impl", C.c_int32),
        ("output", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class MelBank(C.Structure):
    """struct mfcc_hip_mel_bank"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("kind", C.c_int32),
        ("low_hz", C.c_float),
        ("high_hz", C.c_float),
        ("reserved", C.c_int32 * 4),
    ]


# enum mfcc_hip_window
WINDOW_HAMMING, WINDOW_HANN, WINDOW_POVEY, WINDOW_BLACKMAN, WINDOW_RECTANGULAR = 0, 1, 2, 3, 4
MAX_PREEMPH_SUM = 255


class Front(C.Structure):
    """struct mfcc_hip_front"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("window", C.c_int32),
        ("symmetric", C.c_int32),
        ("preemph_num", C.c_int32),
        ("preemph_den", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class Pcen(C.Structure):
    """struct mfcc_hip_pcen"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("s", C.c_float),
        ("alpha", C.c_float),
        ("delta", C.c_float),
        ("r", C.c_float),
        ("eps", C.c_float),
        ("reserved", C.c_int32 * 3),
    ]


class Fbank(C.Structure):
    """struct mfcc_hip_fbank"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_bands", C.c_int32),
        ("scale", C.c_int32),
        ("floor", C.c_float),
        ("reserved", C.c_int32 * 4),
    ]


class FilterbankPost(C.Structure):
    """struct mfcc_hip_filterbank_post"""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("normalize", C.c_int32),
        ("normalize_window", C.c_int32),
        ("normalize_min_window", C.c_int32),
        ("normalize_center", C.c_int32),
        ("delta_order", C.c_int32),
        ("delta_window", C.c_int32),
        ("pcen_on", C.c_int32),
        ("pcen", Pcen),
        ("reserved", C.c_int32 * 4),
    ]


MAX_FBANK_BANDS = 128
FBANK_ENERGY, FBANK_LOG2, FBANK_LN, FBANK_LOG10 = 0, 1, 2, 3

PCEN_TILE = 128

Handle = C.c_void_p           # what a create call fills in: Handle(), passed with byref


def ptr(x):
    """The address of a NumPy array's or a torch tensor's first element as the plain integer every ``c_void_p`` argument
    below takes; ``None`` stays ``None``, a NULL pointer.  The caller keeps ``x`` alive over the call."""
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


# every symbol include/mfcc_hip.h declares: name -> (restype, argtypes)
_H = Handle
_SZ = C.c_size_t
_PSZ = C.POINTER(C.c_size_t)
SYMBOLS = {
    "mfcc_hip_serial_packed_size": (C.c_size_t, [C.c_size_t, C.c_int]),
    "mfcc_hip_serial_pack": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]),
    "mfcc_hip_serial_unpack": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "mfcc_hip_eval_power": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_longlong)]),
    "mfcc_hip_process_ragged_i16": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                              C.c_void_p]),
    "mfcc_hip_process_ragged_fixed_i16": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                    C.c_size_t, C.c_void_p]),
    "mfcc_hip_convert_wavs": (C.c_int, [_H, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_size_t, C.c_int,
                                        C.c_void_p]),
    "mfcc_hip_process_ragged_i16_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_void_p]),
    "mfcc_hip_process_ragged_fixed_i16_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                        C.c_size_t, C.c_void_p]),
    "mfcc_hip_abi_version": (C.c_int, []),
    "mfcc_hip_default_params": (C.c_int, [C.POINTER(Params)]),
    "mfcc_hip_create": (C.c_int, [C.POINTER(Params), C.POINTER(_H)]),
    "mfcc_hip_destroy": (None, [_H]),
    "mfcc_hip_set_stream": (C.c_int, [_H, C.c_void_p]),
    "mfcc_hip_use_own_stream": (C.c_int, [_H]),
    "mfcc_hip_synchronize": (C.c_int, [_H]),
    "mfcc_hip_num_frames": (C.c_int, [C.POINTER(Params), _SZ, _PSZ]),
    "mfcc_hip_strerror": (C.c_char_p, [C.c_int]),
    "mfcc_hip_last_hip_error": (C.c_int, [_H]),
    "mfcc_hip_get_table": (C.c_int, [C.POINTER(Params), C.c_int, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_process_i16": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_process_fixed_i16": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_process_i16_dev": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, _SZ, C.c_int, C.c_void_p, _PSZ]),
    "mfcc_hip_process_fixed_i16_dev": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, _SZ, C.c_int, C.c_void_p, _PSZ]),
    "mfcc_hip_time_dev": (C.c_int, [_H, C.c_int, C.c_void_p, _SZ, _SZ, _SZ, C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(C.c_float)]),
    "mfcc_hip_kernel_name": (C.c_char_p, [_H, C.c_int]),
    "mfcc_hip_set_normalize": (C.c_int, [_H, C.c_int]),
    "mfcc_hip_normalize_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, _SZ, C.c_int]),
    "mfcc_hip_set_normalize_window": (C.c_int, [_H, C.c_int, C.c_int, C.c_int]),
    "mfcc_hip_normalize_sliding_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _SZ, C.c_int, C.c_int,
                                                 C.c_int, C.c_int]),
    "mfcc_hip_set_deltas": (C.c_int, [_H, C.c_int, C.c_int]),
    "mfcc_hip_deltas_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _SZ, C.c_int, C.c_int]),
    "mfcc_hip_set_vad": (C.c_int, [_H, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float]),
    "mfcc_hip_vad_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_int, C.c_void_p, _SZ, C.c_float, C.c_float, C.c_int,
                                   C.c_float, C.c_void_p]),
    "mfcc_hip_select_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _SZ, C.c_void_p, _SZ,
                                      C.c_void_p]),
    "mfcc_hip_convert_wav": (C.c_int, [_H, C.c_char_p, C.c_char_p, C.c_int, _PSZ]),
    "mfcc_hip_stream_create": (C.c_int, [_H, C.c_int, C.POINTER(_H)]),
    "mfcc_hip_stream_destroy": (None, [_H]),
    "mfcc_hip_stream_reset": (C.c_int, [_H]),
    "mfcc_hip_stream_pending": (C.c_size_t, [_H]),
    "mfcc_hip_stream_max_frames": (C.c_size_t, [_H, _SZ]),
    "mfcc_hip_stream_push": (C.c_int, [_H, C.c_void_p, _SZ, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_stream_flush": (C.c_int, [_H, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_bank_create": (C.c_int, [_H, C.c_int, _SZ, C.POINTER(_H)]),
    "mfcc_hip_bank_destroy": (None, [_H]),
    "mfcc_hip_bank_size": (C.c_size_t, [_H]),
    "mfcc_hip_bank_pending": (C.c_int, [_H, C.c_void_p]),
    "mfcc_hip_bank_plan": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_void_p, _SZ, C.c_void_p, C.c_void_p]),
    "mfcc_hip_bank_push": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_bank_push_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_bank_flush": (C.c_int, [_H, C.c_void_p, _SZ, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_bank_reset": (C.c_int, [_H, C.c_void_p, _SZ]),
    "mfcc_hip_bank_create_online": (C.c_int, [_H, _SZ, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    "mfcc_hip_bank_row_width": (C.c_size_t, [_H]),
    "mfcc_hip_bank_lag": (C.c_int, [_H]),
    "mfcc_hip_bank_held": (C.c_int, [_H, C.c_void_p]),
    "mfcc_hip_bank_plan_online": (C.c_int, [C.POINTER(Params), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _SZ,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "mfcc_hip_bank_flush_ragged": (C.c_int, [_H, C.c_void_p, _SZ, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_lift_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_double, _PSZ]),
    "mfcc_hip_eval_power32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int32)]),
    "mfcc_hip_gate_count": (C.c_int, [C.c_int, C.c_int, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_gate_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, _SZ, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "mfcc_hip_gate_windows_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, _SZ, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_gate_create": (C.c_int, [_H, _SZ, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(_H)]),
    "mfcc_hip_gate_destroy": (None, [_H]),
    "mfcc_hip_gate_seen": (C.c_int, [_H, C.c_void_p]),
    "mfcc_hip_gate_plan": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, _SZ, C.c_void_p, C.c_void_p]),
    "mfcc_hip_gate_push_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _SZ,
                                         C.c_void_p]),
    "mfcc_hip_gate_reset": (C.c_int, [_H, C.c_void_p, _SZ]),
    "mfcc_hip_gate_window_dev": (C.c_int, [_H, C.c_void_p, _SZ, C.c_void_p]),
    # frame length below nfft: mfcc_hip_create_framed and the _framed twins of the helpers that take a parameter block
    "mfcc_hip_create_framed": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(_H)]),
    "mfcc_hip_frame_length": (C.c_int, [_H]),
    "mfcc_hip_num_frames_framed": (C.c_int, [C.POINTER(Params), C.c_int, _SZ, _PSZ]),
    "mfcc_hip_get_table_framed": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_bank_plan_framed": (C.c_int, [C.POINTER(Params), C.c_int, C.c_void_p, C.c_void_p, _SZ, C.c_void_p,
                                            C.c_void_p]),
    "mfcc_hip_bank_plan_online_framed": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, _SZ, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the mel bank of a handle: mfcc_hip_create_banked and the table helper's _banked twin
    "mfcc_hip_create_banked": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(MelBank), C.POINTER(_H)]),
    "mfcc_hip_get_table_banked": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(MelBank), C.c_int, C.c_void_p, _SZ,
                                            _PSZ]),
    "mfcc_hip_mel_bank_of": (C.c_int, [_H, C.POINTER(MelBank)]),
    # the front of a handle (window function, pre-emphasis pair): mfcc_hip_create_fronted and the table helper's twin
    "mfcc_hip_create_fronted": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(MelBank), C.POINTER(Front),
                                          C.POINTER(_H)]),
    "mfcc_hip_get_table_fronted": (C.c_int, [C.POINTER(Params), C.c_int, C.POINTER(MelBank), C.POINTER(Front), C.c_int,
                                             C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_front_of": (C.c_int, [_H, C.POINTER(Front)]),
    # PCEN: the host-only helpers, the handle's setting and the kernels' direct entry
    "mfcc_hip_pcen_defaults": (C.c_int, [C.POINTER(Pcen)]),
    "mfcc_hip_pcen_constants": (C.c_int, [C.POINTER(Pcen), C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mfcc_hip_set_pcen": (C.c_int, [_H, C.POINTER(Pcen)]),
    "mfcc_hip_pcen_dev": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, _SZ, C.POINTER(Pcen)]),
    "mfcc_hip_bank_create_online_pcen": (C.c_int, [_H, _SZ, C.POINTER(Pcen), C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(_H)]),
    # sample formats: the host-only helpers, the kernels' direct entry and the handle's setting
    "mfcc_hip_sample_size": (C.c_size_t, [C.c_int]),
    "mfcc_hip_decode_host": (C.c_int, [C.c_int, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_decode_dev": (C.c_int, [_H, C.c_int, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_set_sample_format": (C.c_int, [_H, C.c_int]),
    "mfcc_hip_sample_format": (C.c_int, [_H]),
    # sample rates: the host-only helpers and the kernel's direct entry
    "mfcc_hip_resample_geometry": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mfcc_hip_resample_count": (C.c_int, [C.c_int, C.c_int, _SZ, C.POINTER(_SZ)]),
    "mfcc_hip_resample_taps": (C.c_int, [C.c_int, C.c_int, C.c_void_p, _SZ, C.POINTER(_SZ)]),
    "mfcc_hip_resample_host": (C.c_int, [C.c_int, C.c_int, C.c_void_p, _SZ, C.c_void_p, _SZ]),
    "mfcc_hip_resample_dev": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, _SZ, C.c_void_p, _SZ]),
    "mfcc_hip_set_input_rate": (C.c_int, [_H, C.c_int]),
    "mfcc_hip_input_rate": (C.c_int, [_H]),
    "mfcc_hip_center_geometry": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, _SZ, C.POINTER(_SZ), C.POINTER(_SZ),
                                           C.POINTER(_SZ)]),
    "mfcc_hip_center_host": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_void_p, _SZ, C.c_void_p, _SZ, C.POINTER(_SZ)]),
    "mfcc_hip_center_dev": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p, _SZ, C.c_void_p, _SZ, C.POINTER(_SZ)]),
    "mfcc_hip_set_center": (C.c_int, [_H, C.c_int]),
    "mfcc_hip_center": (C.c_int, [_H]),
    # live lines: the streaming resampler
    "mfcc_hip_resampler_create": (C.c_int, [_H, _SZ, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    "mfcc_hip_resampler_destroy": (None, [_H]),
    "mfcc_hip_resampler_seen": (C.c_int, [_H, C.c_void_p]),
    "mfcc_hip_resampler_reset": (C.c_int, [_H, C.c_void_p, _SZ]),
    "mfcc_hip_resampler_plan": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, _SZ, C.c_int, C.c_void_p]),
    "mfcc_hip_resampler_push_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, _SZ, C.c_void_p]),
    "mfcc_hip_resampler_flush_dev": (C.c_int, [_H, C.c_void_p, _SZ, C.c_void_p, _SZ, C.c_void_p]),
    # the power-spectrum output: the host-only helper, the three compute entries and the kernel's name
    "mfcc_hip_spectrum_bins": (C.c_int, [C.POINTER(Params), _PSZ]),
    "mfcc_hip_spectrum_i16_dev": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, _SZ, C.c_int, C.c_void_p, _PSZ]),
    "mfcc_hip_spectrum_ragged_i16_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_void_p]),
    "mfcc_hip_spectrum_i16": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_spectrum_kernel_name": (C.c_char_p, [_H]),
    # the filterbank output: the matrix, the three compute entries, the kernel's name and the host-only HTK matrix
    "mfcc_hip_set_fbank": (C.c_int, [_H, C.POINTER(Fbank), C.c_void_p]),
    "mfcc_hip_fbank_bands": (C.c_int, [_H, _PSZ]),
    "mfcc_hip_fbank_i16_dev": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, _SZ, C.c_int, C.c_void_p, _PSZ]),
    "mfcc_hip_fbank_ragged_i16_dev": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                C.c_void_p]),
    "mfcc_hip_fbank_i16": (C.c_int, [_H, C.c_void_p, _SZ, _SZ, C.c_void_p, _SZ, _PSZ]),
    "mfcc_hip_fbank_kernel_name": (C.c_char_p, [_H]),
    # ... and the bank of live lines on those rows (p may be NULL)
    "mfcc_hip_bank_create_filterbank": (C.c_int, [_H, _SZ, C.POINTER(Pcen), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_H)]),
    "mfcc_hip_htk_weights": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, _SZ, _PSZ]),
    # the post-passes behind the three compute entries (p may be NULL) and the row width they give
    "mfcc_hip_set_filterbank_post": (C.c_int, [_H, C.POINTER(FilterbankPost)]),
    "mfcc_hip_filterbank_row_width": (C.c_size_t, [_H]),
}

_lib = None


class MfccHipError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = load().mfcc_hip_strerror(code).decode()
        super().__init__("%s: %s (%d)" % (what, msg, code) if what else "%s (%d)" % (msg, code))


def load():
    """dlopen the in-tree library and type every entry point; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C mfcc_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7; if ours (linked
    # against /opt/rocm) were loaded first the process would end up with a runtime torch did
    # not initialise.  torch is this package's plumbing for device memory and streams, so
    # load it first and let libmfcc_hip.so bind to the runtime that is already resident.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.mfcc_hip_abi_version() != ABI_VERSION:
        raise ImportError("libmfcc_hip.so ABI %d != binding ABI %d" %
                          (lib.mfcc_hip_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def kernel_source_hash() -> str:
    """sha256 (first 16 hex digits) over the kernel sources in csrc/: stamps the rocprofv3 summaries kept in
    profiles/ so that bench.py can tell whether a committed counter figure still belongs to the kernels it runs."""
    import glob
    import hashlib
    hsh = hashlib.sha256()
    src = os.path.join(_HERE, "csrc")
    for f in sorted(glob.glob(os.path.join(src, "*.hpp")) + glob.glob(os.path.join(src, "*.hip"))):
        hsh.update(os.path.basename(f).encode())
        hsh.update(open(f, "rb").read())
    return hsh.hexdigest()[:16]


def check(code, what=""):
    if code != SUCCESS:
        raise MfccHipError(code, what)
