/*
 * mfcc_hip.h -- C ABI of the MI355X-native MFCC hot path (libmfcc_hip.so).
 *
 * Drop-in boundary for the per-frame MFCC math of lambdaconcept/mfcc's `mfcc/core`
 * (pre-emphasis -> framing -> Hamming -> FFT -> |.|^2 -> mel -> log2 -> DCT-II -> keep n_cep).
 * The reference has no software operator API for this path: it sits behind
 *   (1) the RTL stream interface  MFCC.sink / MFCC.source / MFCC.reset   mfcc/core/mfcc.py:28-30
 *   (2) the host driver's C calls  mfcc_open / mfcc_convert / mfcc_close  software/main.c:36,100,53
 *       over the transport           ft601_write / ft601_read             software/ft601.h:55-56
 * This header is the batch equivalent of (2): one call = whole utterance(s) instead of a
 * USB ping-pong per frame.  Plain pointers and sizes only; no C++ / torch types.
 *
 * Conventions kept from the reference:
 *   - 0 = success, negative error codes in the ft601_error range      software/ft601.h:25-32
 *   - caller owns every in/out buffer; the handle owns device tables/streams   main.c:109,40
 *   - output layout [frame][n_cep] row-major, i.e. the `.mfcc` file layout     main.c:162-165
 *     (raw, or standardized per channel / utterance: mfcc_hip_set_normalize);
 *     with output = MFCC_HIP_OUTPUT_LOGMEL the rows are [frame][n_mel] log2 mel energies instead
 *     (the stage before the DCT, notebook/MFCC.ipynb `audio_log`); every "n_cep" below that
 *     sizes an output row then reads "n_mel"
 *   - nothing is printed by the library (the reference printf's; a log hook exists there,
 *     ft601.h:43-51 -- here errors are returned and described by mfcc_hip_strerror)
 *   - a handle is not thread-safe; distinct handles are independent            ft601.c:185,197
 *
 * Two numeric contracts:
 *   float : notebook/MFCC.ipynb (float64 NumPy) evaluated in fp32 on the GPU, <= 1e-4 rel-err
 *   fixed : the nMigen RTL arithmetic of mfcc/core + mfcc/misc/fft.py, bit-exact int16
 */
#ifndef MFCC_HIP_H
#define MFCC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFCC_HIP_ABI_VERSION 2

/* error codes: same numbering family as `enum ft601_error` (software/ft601.h:25-32) */
enum mfcc_hip_error {
    MFCC_HIP_SUCCESS             = 0,
    MFCC_HIP_ERROR_INVALID_PARAM = -101,
    MFCC_HIP_ERROR_NOT_FOUND     = -102,   /* no usable HIP device                     */
    MFCC_HIP_ERROR_NO_MEM        = -103,
    MFCC_HIP_ERROR_BUSY          = -104,
    MFCC_HIP_ERROR_UNSUPPORTED   = -105,   /* parameter combination has no kernel      */
    MFCC_HIP_ERROR_BUFFER_SMALL  = -106,   /* caller's output capacity is too small    */
    MFCC_HIP_ERROR_IO            = -107,   /* file open/read/write (wav -> .mfcc)      */
    MFCC_HIP_ERROR_OTHER         = -200    /* HIP runtime error, see mfcc_hip_last_hip_error */
};

/* framing of the tail of a stream */
enum mfcc_hip_pad_mode {
    /* notebook/MFCC.ipynb cell 9: frames = int((n - nfft) / hop) + 1, tail samples dropped */
    MFCC_HIP_PAD_NOTEBOOK = 0,
    /* host driver + RTL bench: zeros are fed after EOF until the frame holding the last
     * sample is out: frames = (n - nfft) / hop + 2 (1 if n < nfft)   software/main.c:95,134-144 */
    MFCC_HIP_PAD_STREAM = 1
};

/* which float kernel to run (the results agree to fp32 rounding) */
enum mfcc_hip_float_impl {
    MFCC_HIP_IMPL_AUTO = 0,     /* fastest kernel that supports the parameters          */
    MFCC_HIP_IMPL_GENERIC = 1,  /* one frame per wave, any supported nfft / n_mel       */
    MFCC_HIP_IMPL_FUSED512 = 2  /* 512/170/32 specialised kernel; on a framed handle
                                   (mfcc_hip_create_framed) the 512 / hop 160 one       */
};

/* what a float output row holds */
enum mfcc_hip_output {
    MFCC_HIP_OUTPUT_CEPSTRA = 0,  /* [n_cep] DCT-II cepstra (x lifter): the `.mfcc` coefficients      */
    MFCC_HIP_OUTPUT_LOGMEL = 1    /* [n_mel] log2 of the mel band energies (MFCC.ipynb `audio_log.T`),
                                     -inf for a silent band.  Float path only: the fixed-point entry
                                     points, fixed streaming sessions and the .mfcc file writers
                                     return MFCC_HIP_ERROR_UNSUPPORTED; lifter must be 0; n_cep is
                                     validated but not used                                       */
};

/* per-segment normalization of float output rows (mfcc_hip_set_normalize / mfcc_hip_normalize_dev below).  A segment is
 * one channel of a dense call or one utterance of a ragged one; per column j of its rows, over the FINITE values F
 * (a silent frame's -inf / NaN are left out):  mu = mean(F),  sigma = sqrt(mean((F - mu)^2)) (population std, the
 * `sklearn.preprocessing.scale` of the reference's software/genlibrosa.py), both in float64, sigma' = 1 where
 * sigma < 10 * 2^-52 (a constant column gives 0).  y = (x - mu32) * r32 with mu and 1 / sigma' rounded once to fp32
 * (MEAN: r32 = 1); non-finite x are written back unchanged.  The result of a segment depends on its rows alone: it
 * is the same bits from every entry point, any chunking, any run.                                              */
enum mfcc_hip_normalize {
    MFCC_HIP_NORMALIZE_NONE = 0,      /* raw rows (the state after mfcc_hip_create)   */
    MFCC_HIP_NORMALIZE_MEAN = 1,      /* y = x - mu                                     */
    MFCC_HIP_NORMALIZE_MEAN_VAR = 2   /* y = (x - mu) / sigma'  (CMVN)                  */
};

/*
 * Parameters = the constructor arguments of `MFCC(width=16, nfft, samplerate, nfilters,
 * nceptrums)` (mfcc/core/mfcc.py:20-21) plus the host driver's constants
 * (`NFFT 512, STEPSIZE 170, NCEPSTRUMS, SAMPLERATE 16000`, software/main.c:11-14).
 */
typedef struct mfcc_hip_params {
    uint32_t struct_size;  /* = sizeof(mfcc_hip_params); set by mfcc_hip_default_params   */
    int32_t  nfft;         /* 512.  float and fixed: power of two 64..1024                */
    int32_t  hop;          /* 170.  1..nfft; 0 -> nfft / 3 (mfcc/core/mfcc.py:43).  At any
                              other hop than nfft / 3 the float path runs the generic kernel
                              and the fixed path refuses (MFCC_HIP_ERROR_UNSUPPORTED)     */
    int32_t  n_mel;        /* 32.   float: 1..64; fixed: 4*n_mel must be a power of two   */
    int32_t  n_cep;        /* 13.   1..n_mel; `Discard(first=0, count)` misc/discard.py   */
    int32_t  sample_rate;  /* 16000                                                       */
    int32_t  pad_mode;     /* enum mfcc_hip_pad_mode                                      */
    float    power_scale;  /* float path: P = |X / power_scale|^2.  The notebook hard-codes
                              512 (cell 22); 0 -> nfft                                    */
    float    lifter;       /* float path: sinusoidal lifter L (MFCC.ipynb cell 43,
                              software/lift.py:12); 0 = off                               */
    int32_t  device;       /* HIP device ordinal; -1 = the current device                 */
    int32_t  float_impl;   /* enum mfcc_hip_float_impl                                    */
    int32_t  output;       /* enum mfcc_hip_output; 0 = cepstra                           */
    int32_t  reserved[4];  /* must be zero                                                */
} mfcc_hip_params;

typedef struct mfcc_hip_handle mfcc_hip_handle;

/* ---- lifetime: replaces mfcc_open / mfcc_close (software/main.c:36-56) ------------- */

int  mfcc_hip_abi_version(void);
/* fills *p with nfft 512, hop 170, n_mel 32, n_cep 13, 16 kHz, NOTEBOOK, scale 512 */
int  mfcc_hip_default_params(mfcc_hip_params *p);
/* validates, builds the constant tables on the host, uploads them, creates a stream.
 * Fails with MFCC_HIP_ERROR_NOT_FOUND when no GPU is present: there is no CPU fallback. */
int  mfcc_hip_create(const mfcc_hip_params *p, mfcc_hip_handle **out);
/*
 * Frame length below nfft (float path): the speech front ends' framing, e.g. a 25 ms window advancing by 10 ms and
 * zero-padded to the next power of two -- 400 / 160 / 512 at 16 kHz.  For frame length L:
 *   - hop <= L <= nfft and L >= 2, else MFCC_HIP_ERROR_INVALID_PARAM (p->hop == 0 still means nfft / 3 and is refused
 *     when that exceeds L);
 *   - frame f is samples [f * hop, f * hop + L) of the pre-emphasised stream, multiplied by the periodic Hamming window
 *     of length L, w[i] = 0.54 - 0.46 cos(2 pi i / L) (or the window of the handle's front, mfcc_hip_create_fronted), and
 *     zero-padded at the end to nfft;
 *   - from the FFT on nothing changes: mel points, power_scale (0 -> nfft), DCT and lifter depend on nfft as before;
 *   - frame counts: NOTEBOOK (n - L) / hop + 1 (0 if n < L), STREAM (n - L) / hop + 2 (1 if n < L).
 * frame_length 0 or p->nfft IS mfcc_hip_create: the same kernels, the same bits.  The frame length is not part of
 * mfcc_hip_params (whose size, reserved words and ABI version stay as they are); every function below that takes a
 * parameter block has a _framed twin, and the plain one is its frame_length = 0 case.
 * Every float entry point, streaming session and stream bank works on a framed handle ("nfft" in their descriptions
 * reads "frame length" where it counts the samples of a frame: frame counts, pending < L).  The fixed-point path is the
 * RTL's, whose window is the ROM curve over nfft samples: on a handle with L < nfft every fixed entry point, fixed
 * session and fixed bank and the fixed .mfcc writers return MFCC_HIP_ERROR_UNSUPPORTED.
 * At nfft 512, hop 160, 160 <= L <= 511, n_mel 32 or 16, the handle runs mfcc_fused512_h160_kernel; float_impl GENERIC
 * forces the generic kernel, FUSED512 means that kernel or MFCC_HIP_ERROR_UNSUPPORTED.  A plain handle at hop 160 keeps
 * the generic kernel.
 */
int  mfcc_hip_create_framed(const mfcc_hip_params *p, int frame_length, mfcc_hip_handle **out);
/* the effective frame length of a handle (nfft for a plain one); 0 for NULL */
int  mfcc_hip_frame_length(const mfcc_hip_handle *h);
/*
 * The mel bank as a property of a handle (float path).  MFCC_HIP_MEL_NOTEBOOK is the reference notebook's bank: integer
 * filter points floor((nfft + 1) / sample_rate * f) between 0 and sample_rate / 2, ramps placed on those points.
 * MFCC_HIP_MEL_HTK is the bank of the HTK / Kaldi style front ends, with band limits.  Its contract, all of it float64
 * on the host:
 *   - mel(f) = 1127 ln(1 + f / 700);
 *   - edges e_j = mel(low) + j (mel(high) - mel(low)) / (n_mel + 1), j = 0 .. n_mel + 1;
 *   - bin k lies at m_k = mel(k * sample_rate / nfft), k = 0 .. nfft / 2;
 *   - W[j][k] = max(0, min((m_k - e_j) / (e_{j+1} - e_j), (e_{j+2} - m_k) / (e_{j+2} - e_{j+1}))), no area
 *     normalisation, rounded once to fp32 (MFCC_HIP_TABLE_MEL_DENSE_F32 returns exactly these floats);
 *   - 0 <= low < high <= sample_rate / 2 (high_hz 0 means sample_rate / 2) and 1 <= n_mel <= 64, else
 *     MFCC_HIP_ERROR_INVALID_PARAM;
 *   - a filter may be empty at a coarse bin grid (48 kHz with many filters): its band is then -inf in every frame, as
 *     the definition says;
 *   - everything outside the matrix is unchanged: pre-emphasis, window, power_scale, log2, DCT, lifter, frame counts.
 * bank == NULL, or kind NOTEBOOK with both edges 0, IS mfcc_hip_create_framed: the same kernel, the same bits.  NOTEBOOK
 * with a non-zero edge, an unknown kind, a wrong struct_size or a non-zero reserved word is INVALID_PARAM.
 * The bank is not part of mfcc_hip_params (whose size, reserved words and ABI version stay as they are).
 * On an HTK handle:
 *   - the fixed-point path refuses exactly as on a framed handle: every fixed entry point, fixed session, fixed bank and
 *     the fixed .mfcc writers return MFCC_HIP_ERROR_UNSUPPORTED;
 *   - MFCC_HIP_TABLE_MEL_POINTS_I32 and MFCC_HIP_TABLE_FX_MEL_DENSE_U32 are UNSUPPORTED (the bank has no integer points);
 *   - the float kernel is mfcc_fused512_h160_mb_kernel at nfft 512, hop 160, frame length 160 .. 511, 1 <= n_mel <= 64,
 *     any sample rate, for log-mel rows and for cepstra with n_cep <= 16 (and no filter weight on bin 0, which no HTK
 *     bank has); otherwise the generic kernel.  The other fused forms are built around the notebook bank and are never
 *     selected.  float_impl GENERIC forces the generic kernel, FUSED512 means mfcc_fused512_h160_mb_kernel or
 *     MFCC_HIP_ERROR_UNSUPPORTED.
 * Streaming sessions, stream banks, normalization, deltas and VAD work on an HTK handle as on any other.
 */
enum mfcc_hip_mel_kind { MFCC_HIP_MEL_NOTEBOOK = 0, MFCC_HIP_MEL_HTK = 1 };
typedef struct mfcc_hip_mel_bank {
    uint32_t struct_size;   /* sizeof(mfcc_hip_mel_bank) */
    int32_t  kind;          /* enum mfcc_hip_mel_kind */
    float    low_hz;        /* HTK: lower band edge, >= 0 */
    float    high_hz;       /* HTK: upper band edge; 0 -> sample_rate / 2 */
    int32_t  reserved[4];   /* must be zero */
} mfcc_hip_mel_bank;
int  mfcc_hip_create_banked(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank,
                            mfcc_hip_handle **out);
/* the bank of a handle: kind, low_hz and the effective high_hz (both 0 for a notebook bank) */
int  mfcc_hip_mel_bank_of(const mfcc_hip_handle *h, mfcc_hip_mel_bank *out);
/*
 * The front of a handle (float path): the window function over the frame and the pre-emphasis coefficient -- the two
 * constants between the samples and the spectrum.  front = (window kind, symmetric flag, preemph_num, preemph_den).
 * Windows, for frame length L (mfcc_hip_create_framed; nfft on a plain handle), with D = L for the periodic form
 * (symmetric = 0) and D = L - 1 for the symmetric one (symmetric = 1), evaluated in float64 on the host for i = 0 .. L - 1
 * and zero-padded to nfft:
 *   MFCC_HIP_WINDOW_HAMMING      0.54 - 0.46 cos(2 pi i / D)                          scipy get_window("hamming", L, fftbins)
 *   MFCC_HIP_WINDOW_HANN         0.5 - 0.5 cos(2 pi i / D)                            "hann" (librosa, torchaudio, Whisper)
 *   MFCC_HIP_WINDOW_POVEY        (0.5 - 0.5 cos(2 pi i / D)) ^ 0.85                   Kaldi's (symmetric there)
 *   MFCC_HIP_WINDOW_BLACKMAN     0.42 - 0.5 cos(2 pi i / D) + 0.08 cos(4 pi i / D)    "blackman"
 *   MFCC_HIP_WINDOW_RECTANGULAR  1
 * Pre-emphasis: y[i] = x[i] - (num / den) x[i-1], x[-1] the history sample (0 at a stream's start, or the halo sample).
 *   - 0 <= num <= den, den >= 1, num + den <= 255, else MFCC_HIP_ERROR_INVALID_PARAM; the pair is reduced by its gcd, so
 *     (62, 64) is (31, 32) and mfcc_hip_front_of returns the reduced pair;
 *   - the kernels form the exact integer e[i] = den x[i] - num x[i-1] (|e| < 2^23: exact in int32 and in fp32) and 1 / den
 *     is folded into the window table in float64 before its one rounding to fp32;
 *   - num = 0 switches pre-emphasis off: the history sample then has no influence on any bit.
 * The default is HAMMING, periodic, (31, 32): the reference's.  front == NULL, or the default front written out (in any
 * unreduced form), IS mfcc_hip_create_banked: the same kernel, the same bits.  An unknown kind, symmetric not 0 or 1, a
 * pair outside the constraints, a wrong struct_size or a non-zero reserved word is INVALID_PARAM.  The front is not part
 * of mfcc_hip_params (whose size, reserved words and ABI version stay as they are).
 * Everything behind the window is unchanged: FFT, power_scale, mel banks, log, DCT, lifter, frame counts, post-passes,
 * PCEN, VAD, sample formats, input rate; every float entry point, power spectrum, filterbank, session and stream bank
 * works on such a handle.  On a non-default front:
 *   - the fixed-point path refuses exactly as on a framed handle: every fixed entry point, fixed session, fixed bank and
 *     the fixed .mfcc writers return MFCC_HIP_ERROR_UNSUPPORTED (and so does MFCC_HIP_TABLE_FX_MEL_DENSE_U32);
 *   - with num + den <= 127 (0, 31/32, 15/16, 19/20, 32/33, 63/64 ...) the four-wave 512 kernels serve it where they
 *     serve the shape: mfcc_fused512_h160_kernel, mfcc_fused512_h160_mb_kernel, mfcc_fused512_kernel for cepstra at 512 /
 *     170 (log-mel rows there, and every 1024 shape, run the generic kernel), mfcc_spectrum512_kernel, mfcc_fbank512_kernel;
 *   - with num + den > 127 (97/100, the exact 0.97) every output runs the generic kernels, and float_impl FUSED512 is
 *     MFCC_HIP_ERROR_UNSUPPORTED.  (32, 33) is the fused stand-in for 0.97: the coefficient differs by 3.0e-4.
 */
enum mfcc_hip_window {
    MFCC_HIP_WINDOW_HAMMING = 0,
    MFCC_HIP_WINDOW_HANN = 1,
    MFCC_HIP_WINDOW_POVEY = 2,
    MFCC_HIP_WINDOW_BLACKMAN = 3,
    MFCC_HIP_WINDOW_RECTANGULAR = 4
};
typedef struct mfcc_hip_front {
    uint32_t struct_size;   /* sizeof(mfcc_hip_front) */
    int32_t  window;        /* enum mfcc_hip_window */
    int32_t  symmetric;     /* 0: periodic (D = L), 1: symmetric (D = L - 1) */
    int32_t  preemph_num;   /* 0 .. preemph_den; 0: no pre-emphasis */
    int32_t  preemph_den;   /* >= 1, preemph_num + preemph_den <= 255 */
    int32_t  reserved[3];   /* must be zero */
} mfcc_hip_front;
int  mfcc_hip_create_fronted(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank,
                             const mfcc_hip_front *front, mfcc_hip_handle **out);
/* the front of a handle, the pair reduced (HAMMING, 0, 31, 32 for a handle made without one) */
int  mfcc_hip_front_of(const mfcc_hip_handle *h, mfcc_hip_front *out);
/* Lifetime rule: a handle that still has streaming sessions (mfcc_hip_stream_create below) is only MARKED
 * by mfcc_hip_destroy -- its stream, tables and scratch stay valid for those sessions, no new session can be
 * opened on it and no other call may be made with it -- and is freed by the mfcc_hip_stream_destroy of its
 * last session.  Without live sessions it is freed at once.  Either order of the destroy calls is safe. */
void mfcc_hip_destroy(mfcc_hip_handle *h);
/* run on a caller-provided hipStream_t (e.g. torch's current stream).  NULL means the HIP
 * null (default) stream -- which is what torch uses unless told otherwise -- NOT "none". */
int  mfcc_hip_set_stream(mfcc_hip_handle *h, void *hip_stream);
/* go back to the handle's own (non-blocking) stream, the state after mfcc_hip_create */
int  mfcc_hip_use_own_stream(mfcc_hip_handle *h);
int  mfcc_hip_synchronize(mfcc_hip_handle *h);

/* ---- host-only helpers (work without a GPU) ------------------------------------------ */

/* frame count for a stream of n_samples under p->pad_mode (`nframes`, main.c:95) */
int  mfcc_hip_num_frames(const mfcc_hip_params *p, size_t n_samples, size_t *n_frames);
/* ... of a framed handle (mfcc_hip_create_framed; frame_length 0 or nfft: the call above) */
int  mfcc_hip_num_frames_framed(const mfcc_hip_params *p, int frame_length, size_t n_samples, size_t *n_frames);
const char *mfcc_hip_strerror(int err);
/* hipError_t of the last failing runtime call on this handle (0 if none); with h == NULL:
 * of the last failing mfcc_hip_create on this thread */
int  mfcc_hip_last_hip_error(const mfcc_hip_handle *h);

/* The constant tables the kernels use, as built on the host (no GPU needed) -- lets the
 * CPU test-suite check the table builders against the oracle.  `which`: */
enum mfcc_hip_table {
    MFCC_HIP_TABLE_WINDOW_F32      = 0,  /* float[nfft]            periodic Hamming, or the front's */
    MFCC_HIP_TABLE_MEL_POINTS_I32  = 1,  /* int32[n_mel + 2]       filter points          */
    MFCC_HIP_TABLE_MEL_DENSE_F32   = 2,  /* float[n_mel][nfft/2+1] weights (unscaled)     */
    MFCC_HIP_TABLE_DCT_F32         = 3,  /* float[n_cep][n_mel]    ortho DCT-II (x lifter)*/
    MFCC_HIP_TABLE_FX_CURVE_I32    = 4,  /* int32[nfft]            RTL window curve       */
    MFCC_HIP_TABLE_FX_TWIDDLE_I32  = 5,  /* int32[nfft/2][2]       RTL twiddle ROM re,im  */
    MFCC_HIP_TABLE_FX_MEL_DENSE_U32 = 6  /* uint32[n_mel][nfft/2]  RTL filterbank weights
                                            (x 2^-30), closed form of the accumulators    */
};
/* writes up to `cap_bytes`; *n_bytes = size of the table */
int  mfcc_hip_get_table(const mfcc_hip_params *p, int which, void *buf, size_t cap_bytes,
                        size_t *n_bytes);
/* ... of a framed handle.  Only MFCC_HIP_TABLE_WINDOW_F32 differs: still float[nfft], the first frame_length entries
 * are the periodic Hamming window of that length, the rest 0 (MFCC_HIP_TABLE_FX_MEL_DENSE_U32 is UNSUPPORTED) */
int  mfcc_hip_get_table_framed(const mfcc_hip_params *p, int frame_length, int which, void *buf, size_t cap_bytes,
                               size_t *n_bytes);
/* ... of a handle with a mel bank (mfcc_hip_create_banked; bank NULL: the call above).  On an HTK bank
 * MFCC_HIP_TABLE_MEL_DENSE_F32 is the matrix of the contract and MFCC_HIP_TABLE_MEL_POINTS_I32 and
 * MFCC_HIP_TABLE_FX_MEL_DENSE_U32 are UNSUPPORTED; the other tables do not depend on the bank */
int  mfcc_hip_get_table_banked(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank, int which,
                               void *buf, size_t cap_bytes, size_t *n_bytes);
/* ... of a handle with a front (mfcc_hip_create_fronted; front NULL: the call above).  Only MFCC_HIP_TABLE_WINDOW_F32
 * differs: the front's window over the frame length, WITHOUT the 1 / den the kernels' own tables carry, zeros up to nfft;
 * on a non-default front MFCC_HIP_TABLE_FX_MEL_DENSE_U32 is UNSUPPORTED */
int  mfcc_hip_get_table_fronted(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank,
                                const mfcc_hip_front *front, int which, void *buf, size_t cap_bytes, size_t *n_bytes);

/* ---- the hot path: replaces the per-frame ft601_write / ft601_read loop of
 *      mfcc_convert (software/main.c:128-166) ------------------------------------------ */

/*
 * Host buffers.  pcm: [n_channels][n_samples_per_ch] int16 (each channel is an independent
 * stream: pre-emphasis history starts at 0, as after `mfcc_softreset`, main.c:21-34).
 * out: [n_channels][n_frames][n_cep].  out_capacity counts elements of out.
 * Synchronous: returns after the results are in `out`.
 */
int  mfcc_hip_process_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n_samples_per_ch,
                          size_t n_channels, float *out, size_t out_capacity, size_t *n_frames);
int  mfcc_hip_process_fixed_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n_samples_per_ch,
                                size_t n_channels, int16_t *out, size_t out_capacity,
                                size_t *n_frames);

/*
 * Ragged batch (host buffers): n_utterances utterances of different lengths in one launch -- the
 * batched form of the driver's directory walk (show_dir_content -> mfcc_convert per file,
 * software/main.c:206-247), every utterance an independent stream starting from reset.
 * pcm: the utterances back to back; utterance u is pcm[offsets[u] .. offsets[u + 1]), offsets has
 * n_utterances + 1 entries.  out: the frames of all utterances back to back, [sum frames][n_cep];
 * utterance u's frames are rows frame_offsets[u] .. frame_offsets[u + 1] (n_utterances + 1 entries,
 * written even when out is too small, so a caller can size out from a first call with capacity 0:
 * MFCC_HIP_ERROR_BUFFER_SMALL).  Results are bit-identical to one mfcc_hip_process_* call per
 * utterance.  Synchronous.
 */
int  mfcc_hip_process_ragged_i16(mfcc_hip_handle *h, const int16_t *pcm, const size_t *offsets,
                                 size_t n_utterances, float *out, size_t out_capacity,
                                 size_t *frame_offsets);
int  mfcc_hip_process_ragged_fixed_i16(mfcc_hip_handle *h, const int16_t *pcm, const size_t *offsets,
                                       size_t n_utterances, int16_t *out, size_t out_capacity,
                                       size_t *frame_offsets);

/* The same with the utterances and the result in HBM (d_pcm: all utterances back to back, d_out: dense
 * [sum frames][n_cep]); offsets / frame_offsets stay host arrays.  Asynchronous on the handle's stream
 * like the other *_dev entry points; frame_offsets is complete on return. */
int  mfcc_hip_process_ragged_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets,
                                     size_t n_utterances, void *d_out, size_t out_capacity,
                                     size_t *frame_offsets);
int  mfcc_hip_process_ragged_fixed_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets,
                                           size_t n_utterances, void *d_out, size_t out_capacity,
                                           size_t *frame_offsets);

/*
 * Device-resident buffers (HBM in, HBM out), asynchronous on the handle's stream.
 * d_pcm:  channel c starts at d_pcm + c * ch_stride_samples (int16 units).
 * halo:   0 or 1.  1 = the first sample of every channel is only pre-emphasis history
 *         (x[-1] of a shard cut out of a longer stream); frames start at sample 1 and
 *         n_samples_per_ch does not count it.  Used for frame-range sharding.
 * d_out:  [n_channels][n_frames][n_cep], float (float path) or int16 (fixed path).
 */
int  mfcc_hip_process_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n_samples_per_ch,
                              size_t ch_stride_samples, size_t n_channels, int halo,
                              void *d_out, size_t *n_frames);
int  mfcc_hip_process_fixed_i16_dev(mfcc_hip_handle *h, const void *d_pcm,
                                    size_t n_samples_per_ch, size_t ch_stride_samples,
                                    size_t n_channels, int halo, void *d_out, size_t *n_frames);

/*
 * Measurement helper: `iters` back-to-back launches of the float (fixed = 0) or fixed
 * (fixed = 1) kernel on device-resident buffers, bracketed by HIP events recorded on the
 * stream the kernel is launched on; *avg_ms = elapsed / iters.  Used by bench.py for the
 * `roofline.achieved` figure.
 */
int  mfcc_hip_time_dev(mfcc_hip_handle *h, int fixed, const void *d_pcm, size_t n_samples_per_ch,
                       size_t ch_stride_samples, size_t n_channels, void *d_out,
                       int warmup, int iters, float *avg_ms);

/* ---- power spectrum ----------------------------------------------------------------------------------------------
 * The intermediate every float output starts from (the notebook's audio_power, MFCC.ipynb cell 22), as rows of
 * bins = nfft / 2 + 1 float32 values.  Element k of row f of a channel is
 *
 *     | FFT_nfft(w . y_f)[k] / power_scale |^2          k = 0 .. nfft / 2
 *
 * y: the pre-emphasised stream, y[i] = x[i] - 31/32 x[i - 1] (x[-1] = 0, or the halo sample; num / den of the handle's
 * front in place of 31/32, mfcc_hip_create_fronted); y_f: its nfft samples from sample f * hop on; w: the handle's window --
 * periodic Hamming (or the front's window function) over the handle's frame length, then zeros up to nfft
 * (mfcc_hip_create_framed).  Framing, padding and frame counts are the handle's (hop, pad_mode, frame length), exactly
 * those of mfcc_hip_process_i16*.  A frame whose samples (and history sample) are all zero gives +0.0 in every bin; every
 * value is finite and >= 0 for any int16 input.  With a mel matrix W [n][bins] the band energies of the float path are
 * W . row -- for any n, not only the 64 rows the fused kernels hold.
 *
 * The handle's sample format and input rate apply (they say what a sample pointer holds: the decode and the resampler
 * run in front, as for mfcc_hip_process_*).  The handle's n_mel, n_cep, output, lifter, mel bank, normalization, delta,
 * PCEN and VAD settings do NOT apply: they are ignored, and a handle with any of them returns the rows of a plain one.
 * float_impl = MFCC_HIP_IMPL_GENERIC selects the generic spectrum kernel.  There is no fixed-point form, and streaming
 * sessions and stream banks have no spectrum output.  The parameter block and the ABI version are unchanged.           */

/* bins of a row for this parameter block: nfft / 2 + 1.  Host only.  Invalid block or NULL bins:
 * MFCC_HIP_ERROR_INVALID_PARAM. */
int  mfcc_hip_spectrum_bins(const mfcc_hip_params *p, size_t *bins);
/* Device-resident buffers: the arguments, frame counts, halo rule, stream behaviour and refusals of
 * mfcc_hip_process_i16_dev.  d_out: float32 [n_channels][n_frames][bins], 4-byte aligned. */
int  mfcc_hip_spectrum_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n_samples_per_ch,
                               size_t ch_stride_samples, size_t n_channels, int halo, void *d_out, size_t *n_frames);
/* Ragged batch on the device: the arguments and refusals of mfcc_hip_process_ragged_i16_dev, MFCC_HIP_ERROR_BUFFER_SMALL
 * with frame_offsets filled included.  d_out: [sum frames][bins]; out_capacity counts floats.  Rows are bit-identical to
 * one mfcc_hip_spectrum_i16_dev call per utterance. */
int  mfcc_hip_spectrum_ragged_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets, size_t n_utterances,
                                      void *d_out, size_t out_capacity, size_t *frame_offsets);
/* Host buffers, synchronous: the arguments and refusals of mfcc_hip_process_i16.  out: [n_channels][n_frames][bins];
 * out_capacity counts floats. */
int  mfcc_hip_spectrum_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n_samples_per_ch, size_t n_channels,
                           float *out, size_t out_capacity, size_t *n_frames);
/* the kernel the handle's spectrum calls run: "mfcc_spectrum512_kernel" or "mfcc_spectrum_generic_kernel".  As with the
 * MFCC kernels, a single call whose tile count does not fit the fused kernel's 32-bit arithmetic (2^31 tiles of 16 frames,
 * or 2^26 tiles in one channel) runs the generic spectrum kernel instead, without an error; this name does not change.
 * The ragged entry packs utterances of different lengths into one stream, runs the kernel on it and gathers the rows
 * (equal lengths run as channels of one dense launch): its rows cross HBM twice and the handle holds scratch for
 * every packed frame x bins floats. */
const char *mfcc_hip_spectrum_kernel_name(const mfcc_hip_handle *h);

/* ---- filterbank -------------------------------------------------------------------------------------------------
 * A handle may carry a FILTER MATRIX W [n_bands][bins]: float32, given by the caller from host memory, with
 * bins = nfft / 2 + 1 and 1 <= n_bands <= MFCC_HIP_MAX_FBANK_BANDS = 128.  Every weight is finite and not negative
 * (-0.0 counts as 0); anything else is MFCC_HIP_ERROR_INVALID_PARAM.  Row f of a channel, element j:
 *
 *     E[f][j] = sum_k W[j][k] * P[f][k]        P: the power-spectrum row of section "power spectrum", exactly that contract
 *     y[f][j] = E                               scale ENERGY
 *               c * log2(max(E, floor))         scale LOG2 (c = 1), LN (c = (float)ln 2), LOG10 (c = (float)log10 2)
 *
 * log2 is v_log_f32, the log the mel kernels use, and there is one fp32 multiply by c.  floor is fp32, finite and >= 0;
 * with floor = 0, E = 0 gives -inf, as the log-mel output does.  Framing, window, pre-emphasis, padding, halo, sample
 * format and input rate are the handle's, as for mfcc_hip_spectrum_*.  The handle's n_mel, n_cep, output, lifter, mel
 * bank, normalization, deltas, PCEN and VAD do NOT apply.  Weight on bin 0 and on bin nfft / 2 is allowed.
 *
 * Two results are bit-exact: a band whose row of W is all zero gives E = +0.0 in every frame, and a frame whose samples
 * (and history sample) are all zero gives E = +0.0 in every band.  Every other value is finite and >= 0 in ENERGY scale
 * (as long as the sum itself stays inside fp32).
 *
 * The rows of a segment are the same bits from the dense, ragged and host-buffer entries, and from any chunking of the
 * copy pipeline.  The two kernels agree within the error bound, not bit for bit.  E is the
 * fp32 chain fmaf(W[j][k], P[k], acc) over k from the band's first to its last non-zero bin, ascending, with one
 * exception: at the shapes of "mfcc_fbank512_kernel", a matrix whose bands' first-to-last-non-zero ranges add up to more
 * than 3072 bins (a dense or learned matrix, filters with long tails) is contracted on the matrix cores, weights and
 * power each split into two bfloat16 terms and summed in fp32, about 2^-16 relative per band instead of 2^-24 per bin.
 * Where that is not wanted, MFCC_HIP_IMPL_GENERIC keeps the fp32 chain at about a third of the rate.
 *
 * There is no fixed-point form.  Live lines take these rows through mfcc_hip_bank_create_filterbank (a stream bank, with
 * causal CMVN, deltas and PCEN of its own; a bank of one line is the session).  The post-pass direct entries (mfcc_hip_normalize_dev,
 * mfcc_hip_deltas_dev, mfcc_hip_pcen_dev, mfcc_hip_vad_dev) keep their width limit of 64: rows of up to 64 bands may be
 * fed to them by the caller; wider rows get their post-passes behind the three compute entries below, from the settings
 * of section "filterbank post-passes".  The parameter block, ABI version 2, n_mel 1..64 and every limit of 64 are
 * unchanged. */
#define MFCC_HIP_MAX_FBANK_BANDS 128

enum mfcc_hip_fbank_scale {
    MFCC_HIP_FBANK_ENERGY = 0,
    MFCC_HIP_FBANK_LOG2 = 1,
    MFCC_HIP_FBANK_LN = 2,
    MFCC_HIP_FBANK_LOG10 = 3
};

typedef struct mfcc_hip_fbank {
    uint32_t struct_size;      /* sizeof(mfcc_hip_fbank) */
    int32_t  n_bands;          /* 1 .. MFCC_HIP_MAX_FBANK_BANDS */
    int32_t  scale;            /* enum mfcc_hip_fbank_scale */
    float    floor;            /* the log scales' floor: finite, >= 0 */
    int32_t  reserved[4];      /* must be 0 */
} mfcc_hip_fbank;

/* Sets (replaces) the handle's filter matrix: validates, builds the kernels' tables on the host and uploads them.
 * weights: [p->n_bands][nfft / 2 + 1] float32 in host memory, read before the call returns.  p == NULL removes the
 * matrix (weights is ignored).  A wrong struct_size, non-zero reserved words, n_bands out of range, an unknown scale, a
 * bad floor, a bad weight or weights == NULL: MFCC_HIP_ERROR_INVALID_PARAM, and the handle keeps what it had.  Calls
 * enqueued earlier, on any stream the handle had, keep their matrix: replacing or removing a matrix that a call has
 * used SYNCHRONIZES THE DEVICE (hipDeviceSynchronize) before the old tables are freed; its error is returned as
 * MFCC_HIP_ERROR_OTHER and the handle keeps what it had. */
int  mfcc_hip_set_fbank(mfcc_hip_handle *h, const mfcc_hip_fbank *p, const float *weights);
/* bands of the handle's matrix; 0 when none is set */
int  mfcc_hip_fbank_bands(const mfcc_hip_handle *h, size_t *n_bands);
/* The three compute entries: arguments, frame counts, halo rule, MFCC_HIP_ERROR_BUFFER_SMALL with frame_offsets filled,
 * stream behaviour and refusals of mfcc_hip_spectrum_i16_dev, mfcc_hip_spectrum_ragged_i16_dev and mfcc_hip_spectrum_i16;
 * rows are n_bands wide.  A handle without a matrix: MFCC_HIP_ERROR_UNSUPPORTED. */
int  mfcc_hip_fbank_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n_samples_per_ch, size_t ch_stride_samples,
                            size_t n_channels, int halo, void *d_out, size_t *n_frames);
int  mfcc_hip_fbank_ragged_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets, size_t n_utterances,
                                   void *d_out, size_t out_capacity, size_t *frame_offsets);
int  mfcc_hip_fbank_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n_samples_per_ch, size_t n_channels, float *out,
                        size_t out_capacity, size_t *n_frames);
/* the kernel the handle's filterbank calls run: "mfcc_fbank512_kernel" (nfft 512 at hop 170 with the full frame, or at
 * hop 160 with any frame of 160 .. 512 samples), "mfcc_fbank_generic_kernel", or "" when no matrix is set.  float_impl =
 * MFCC_HIP_IMPL_GENERIC selects the generic kernel; a call that does not fit the fused kernel's 32-bit tile arithmetic
 * runs the generic kernel without an error, as for the spectrum. */
const char *mfcc_hip_fbank_kernel_name(const mfcc_hip_handle *h);
/* Host only: the matrix of the MFCC_HIP_MEL_HTK contract (mfcc_hip_create_banked) for 1 .. 128 bands, [n_bands][nfft / 2
 * + 1] float32; high_hz 0 means sample_rate / 2.  For n_bands <= 64 these are the bits of MFCC_HIP_TABLE_MEL_DENSE_F32 of
 * an HTK handle.  n_floats (optional) receives the count; out may be NULL to ask for it; cap_floats too small:
 * MFCC_HIP_ERROR_BUFFER_SMALL. */
int  mfcc_hip_htk_weights(int nfft, int sample_rate, int n_bands, float low_hz, float high_hz, float *out,
                          size_t cap_floats, size_t *n_floats);

/* ---- filterbank post-passes ----------------------------------------------------------------
 * The matrix may carry post-pass settings OF ITS OWN: PCEN, per-segment or sliding normalization and deltas behind
 * mfcc_hip_fbank_i16_dev, mfcc_hip_fbank_ragged_i16_dev and mfcc_hip_fbank_i16, on rows of up to 128 bands, one segment
 * per channel or utterance.  They are the passes of the sections "per-segment normalization", "sliding-window
 * normalization", "PCEN" and "deltas" below, in that chain's order -- PCEN in place on the raw rows, then the
 * normalization, then deltas -- with those sections' arithmetic: a column of a row of 65 .. 128 floats gets the bits the
 * direct entries give the same column of a slice of at most 64 columns (sliding normalization, PCEN, deltas), and a
 * segment's per-segment statistics depend on the row width and the segment's rows alone.  The rows of a segment are the
 * same bits from the three entries and from any chunking of the copy pipeline.
 *
 * The handle's own settings (mfcc_hip_set_normalize, _set_normalize_window, _set_deltas, _set_pcen, _set_vad) still do
 * NOT apply to a filterbank call, and these do not apply to any other call.  There is no VAD and no selection here: the
 * energy VAD decides on C0 or one named band and a filterbank has no C0; rows of up to 64 bands can still go to
 * mfcc_hip_vad_dev.
 *
 * normalize: enum mfcc_hip_normalize; normalize_window 0 (per segment) or 1 .. MFCC_HIP_MAX_NORMALIZE_WINDOW with
 * 1 <= normalize_min_window <= normalize_window and normalize_center 0 / 1 (the rules of mfcc_hip_set_normalize_window);
 * delta_order 0 .. 2 and delta_window 1 .. MFCC_HIP_MAX_DELTA_WINDOW (those of mfcc_hip_set_deltas; the window is checked
 * at order 0 too); pcen_on 0 / 1, pcen as mfcc_hip_set_pcen takes it (looked at only with pcen_on).  Anything else, a
 * wrong struct_size or a non-zero reserved word: MFCC_HIP_ERROR_INVALID_PARAM.  p == NULL: none.  On a handle without
 * a matrix (p == NULL included), and with pcen_on unless the matrix's scale is MFCC_HIP_FBANK_LOG2 (PCEN reads log2
 * energies): MFCC_HIP_ERROR_UNSUPPORTED.  While a filterbank bank of the handle lives: MFCC_HIP_ERROR_BUSY.  A refused
 * call leaves the settings as they were.  mfcc_hip_set_fbank -- a new matrix or NULL -- RESETS them to none: they were
 * checked against the old matrix's scale and width.  mfcc_hip_bank_create_filterbank on a handle that has such settings:
 * MFCC_HIP_ERROR_UNSUPPORTED (a bank takes its settings at creation and its frame launch is the raw kernel).
 *
 * With settings, rows are mfcc_hip_filterbank_row_width(h) = n_bands * (1 + delta_order) floats wide, [ s | D | DD ]:
 * size buffers and out_capacity by it.  A call with halo = 1 and settings: MFCC_HIP_ERROR_UNSUPPORTED, as
 * mfcc_hip_process_i16_dev answers.  Sample format, input rate and centring in front compose as before.
 *
 * The struct embeds a mfcc_hip_pcen, so it and the two functions are declared behind section "PCEN":
 * mfcc_hip_filterbank_post, mfcc_hip_set_filterbank_post, mfcc_hip_filterbank_row_width. */

/* ---- per-segment normalization (enum mfcc_hip_normalize) -------------------------------------------------------
 * The handle's mode applies to every float call enqueued after it: mfcc_hip_process_i16, mfcc_hip_process_i16_dev,
 * both float mfcc_hip_process_ragged_* entry points and mfcc_hip_time_dev (which then times the launch AND the
 * normalization passes, what mfcc_hip_process_i16_dev enqueues) return normalized rows.  With a mode other than NONE
 * the fixed-point entry points, mfcc_hip_stream_create, mfcc_hip_convert_wav(s) and mfcc_hip_process_i16_dev with
 * halo = 1 (a shard of a longer stream: its statistics would not be the stream's) return MFCC_HIP_ERROR_UNSUPPORTED.
 * NULL handle or an unknown mode: MFCC_HIP_ERROR_INVALID_PARAM; a handle with live streaming sessions:
 * MFCC_HIP_ERROR_BUSY.  The parameter block and the ABI version are unchanged.                                  */
int  mfcc_hip_set_normalize(mfcc_hip_handle *h, int mode);
/* The kernels' direct entry: normalizes float32 rows [seg_offsets[n_segs]][row_width] in HBM in place, segment k =
 * rows seg_offsets[k] .. seg_offsets[k + 1] (host array, n_segs + 1 entries, must not decrease; rows before
 * seg_offsets[0] are not touched).  row_width 1..64, d_rows 4-byte aligned.  Asynchronous on the handle's stream;
 * mode NONE or n_segs = 0 is a no-op.  E.g. the rows of a frame-range-sharded stream after their gather. */
int  mfcc_hip_normalize_dev(mfcc_hip_handle *h, void *d_rows, int row_width, const size_t *seg_offsets, size_t n_segs,
                            int mode);

/* ---- sliding-window normalization -------------------------------------------------------
 * For long channels: with a window on and mode MEAN or MEAN_VAR, the row of frame t of a segment of T rows (one channel
 * of a dense call, one utterance of a ragged one) is standardized with the statistics of rows [a, b) of the SAME
 * segment instead of the whole segment.  With window N, minimum window M and center (Kaldi's SlidingWindowCmn rule):
 *     if center:  a = t - N / 2;  b = a + N
 *     else:       a = t - N;      b = t + 1            (the causal window holds N + 1 frames)
 *     if a < 0:   b -= a;  a = 0
 *     if not center and b > t:  b = max(t + 1, M)      (M only acts on the first frames of the causal form)
 *     if b > T:   a -= b - T;  b = T;  a = max(a, 0)
 * Everything else is the contract of enum mfcc_hip_normalize applied to rows [a, b): per column over the FINITE values
 * of those rows, mu and the population sigma in float64, sigma' = 1 where sigma < 10 * 2^-52 (a window with one finite
 * value, or a constant one, gives exactly 0; Kaldi floors the variance at 1e-10 instead: a documented difference),
 * y = (x - mu32) * r32, non-finite x written back unchanged and left out of every window that covers them.  The rows
 * read are the rows the handle returns with normalization off.  The result of a segment depends on its rows, the row
 * width, N, M, center and the mode alone: the same bits from every entry point, any chunking of a host call, any
 * 4-byte alignment, any run.  Deltas (mfcc_hip_set_deltas) run on the sliding-normalized statics.
 * window = 0: off (the state after mfcc_hip_create: per-segment statistics, bit for bit).  Otherwise
 * 1 <= min_window <= window <= MFCC_HIP_MAX_NORMALIZE_WINDOW, center 0 or 1; anything else, or a NULL handle:
 * MFCC_HIP_ERROR_INVALID_PARAM; live streaming sessions: MFCC_HIP_ERROR_BUSY.  A window with mode NONE is stored and has
 * no effect.  The refusals of a normalizing handle are those of mfcc_hip_set_normalize.  mfcc_hip_time_dev times this
 * pass too.  The parameter block and the ABI version are unchanged.                                             */
#define MFCC_HIP_MAX_NORMALIZE_WINDOW 16384
int  mfcc_hip_set_normalize_window(mfcc_hip_handle *h, int window, int min_window, int center);
/* The kernel's direct entry, OUT OF PLACE (the window of a row reaches into rows already rewritten): d_in rows
 * [seg_offsets[n_segs]][row_width] (rows before seg_offsets[0] not read), d_out rows at the same row indices; rows of
 * d_out outside the segments untouched.  Segment k = rows seg_offsets[k] .. seg_offsets[k + 1] (host array, n_segs + 1
 * entries, must not decrease).  row_width 1..64, window / min_window / center as above (window >= 1), both pointers
 * 4-byte aligned, the two byte ranges must not overlap: otherwise MFCC_HIP_ERROR_INVALID_PARAM.  Asynchronous on the
 * handle's stream; mode NONE or n_segs = 0 is a no-op.                                                         */
int  mfcc_hip_normalize_sliding_dev(mfcc_hip_handle *h, const void *d_in, int row_width, void *d_out,
                                    const size_t *seg_offsets, size_t n_segs, int mode, int window, int min_window,
                                    int center);

/* ---- delta and delta-delta coefficients -------------------------------------------------
 * With delta order K (1 or 2) and window N (1..MFCC_HIP_MAX_DELTA_WINDOW), the float row of frame t of a segment (one
 * channel of a dense call, one utterance of a ragged one) becomes W * (1 + K) wide, W = n_cep or n_mel:
 *     [ s_t (W) | D_t (W) | DD_t (W, order 2 only) ]
 * s_t is the static row the handle returns with deltas off (lifter, log-mel and normalization as set), bit for bit.
 *     D_t = r * sum_{n=1..N} n (s_{t+n} - s_{t-n}),  r = 1 / (2 sum_{n=1..N} n^2)
 * with indices clamped to the segment (s before its first row = its first row, after its last = its last: HTK's rule);
 * DD_t is the same formula on the D rows, clamped the same way.  In fp32, for every element: acc = 0; for n = 1..N
 * ascending: acc = fmaf((float)n, a_n - b_n, acc); then D = acc * (float)r, nothing else contracted -- every entry
 * point and every cut of the rows gives the same bits.  A non-finite static value (a silent band) makes every D
 * element that reads it non-finite, and DD follows from D the same way.  A segment of one row gives D = DD = 0 where
 * its statics are finite.
 *
 * The handle's order applies to every float call enqueued after it, as normalization does: mfcc_hip_process_i16,
 * mfcc_hip_process_i16_dev, both float mfcc_hip_process_ragged_* entry points and mfcc_hip_time_dev (which then times
 * the delta pass too).  Output capacities, BUFFER_SMALL and frame_offsets count rows of W * (1 + K).  With an order
 * other than 0 the fixed-point entry points, mfcc_hip_stream_create (a session would need 2 K N frames of lookahead),
 * mfcc_hip_convert_wav(s) (a .mfcc row is n_cep wide) and mfcc_hip_process_i16_dev with halo = 1 (a shard's edges
 * are not the stream's) return MFCC_HIP_ERROR_UNSUPPORTED.  NULL handle or a bad order / window:
 * MFCC_HIP_ERROR_INVALID_PARAM; a handle with live streaming sessions: MFCC_HIP_ERROR_BUSY.                      */
#define MFCC_HIP_MAX_DELTA_WINDOW 8
/* order 0 (off, the state after create), 1 (D) or 2 (D, DD); window 1..MFCC_HIP_MAX_DELTA_WINDOW */
int  mfcc_hip_set_deltas(mfcc_hip_handle *h, int order, int window);
/* The kernel's direct entry: d_in rows [seg_offsets[n_segs]][width] (rows before seg_offsets[0] not read), d_out rows
 * [..][width * (1 + order)] at the same row indices; rows of d_out outside the segments untouched.  Segment k = rows
 * seg_offsets[k] .. seg_offsets[k + 1] (host array, n_segs + 1 entries, must not decrease).  width 1..64, order 1..2,
 * window 1..MFCC_HIP_MAX_DELTA_WINDOW, both pointers 4-byte aligned, the two byte ranges must not overlap.
 * Asynchronous on the handle's stream; n_segs = 0 is a no-op.  E.g. the gathered rows of a frame-range-sharded
 * stream, after mfcc_hip_normalize_dev.                                                                        */
int  mfcc_hip_deltas_dev(mfcc_hip_handle *h, const void *d_in, int width, void *d_out,
                         const size_t *seg_offsets, size_t n_segs, int order, int window);

/* ---- energy VAD and voiced-frame selection -----------------------------------------------
 * Kaldi's compute-vad-energy and select-voiced-frames on float rows in HBM.  A segment is one channel or one utterance
 * of T rows; e_t is column `column` of the RAW static row of frame t -- the row the handle returns with normalization,
 * deltas and VAD all off.  With energy_threshold (fp32, finite), energy_mean_scale (fp32, >= 0), frames_context
 * (0..MFCC_HIP_MAX_VAD_CONTEXT) and proportion_threshold (fp32, 0 < p < 1), Kaldi's ComputeVadEnergy:
 *     F       = the finite e_t of the segment
 *     theta   = (double)energy_threshold + (double)energy_mean_scale * mean(F)      mean in float64; with scale 0 no mean
 *               is taken; with scale != 0 and F empty every frame is unvoiced
 *     above_t = isfinite(e_t) && (double)e_t > theta       a silent frame's -inf / NaN is never above and is left out of
 *                                                          the mean, as normalization leaves it out
 *     num     = the count of above frames over [t - ctx, t + ctx] n [0, T),  den = the size of that intersection
 *     voiced_t = ((float)num >= (float)den * p)            one fp32 multiply
 * The order of the mean's summation is a function of the segment's own rows and of the row width alone: the same bits
 * from every entry point, any chunking of a host call, any run.  No atomics are used anywhere.
 * The defaults are Kaldi's: 5.0, 0.5, 0, 0.6 -- applied in the column's OWN units.  This library's C0 is log2-based:
 * it is Kaldi's natural-log C0 divided by ln 2 (up to the constant that power_scale adds), so a threshold taken from a
 * Kaldi recipe converts by 1 / ln 2.  Column 0 is C0 on a cepstra handle; on a log-mel handle the caller names the band.
 *
 * mfcc_hip_set_vad: mode MFCC_HIP_VAD_OFF (the state after mfcc_hip_create; every entry point gives the bits it gave
 * before this call existed) or MFCC_HIP_VAD_SELECT: the four float ragged entry points (mfcc_hip_process_ragged_i16,
 * mfcc_hip_process_ragged_i16_dev; one utterance is a ragged call of one) return ONLY the voiced rows, packed back to
 * back in order, and frame_offsets describes them.  out_capacity is checked against the count of ALL frames, so a caller
 * sizes `out` as before; the device entry synchronizes the stream before it returns (frame_offsets depends on the data).
 * The order of the passes is fixed:  MFCC kernels -> decision on the raw rows -> normalization (per segment or sliding,
 * statistics over ALL frames of the segment: Kaldi's order) -> deltas over all frames -> selection of the final rows.
 * A SELECT handle answers MFCC_HIP_ERROR_UNSUPPORTED to the fixed-point entry points, mfcc_hip_stream_create,
 * mfcc_hip_convert_wav(s), the dense mfcc_hip_process_i16 / mfcc_hip_process_i16_dev and mfcc_hip_time_dev: a dense
 * [channel][frame][W] result cannot hold rows of different counts.  NULL handle, an unknown mode, a column outside the
 * handle's static row or a parameter outside its range (checked with either mode): MFCC_HIP_ERROR_INVALID_PARAM; live
 * streaming sessions: MFCC_HIP_ERROR_BUSY.  The parameter block and the ABI version are unchanged.                  */
#define MFCC_HIP_MAX_VAD_CONTEXT 64
enum mfcc_hip_vad_mode {
    MFCC_HIP_VAD_OFF = 0,       /* every frame is returned (the state after mfcc_hip_create) */
    MFCC_HIP_VAD_SELECT = 1     /* the float ragged entry points return the voiced frames only */
};
int  mfcc_hip_set_vad(mfcc_hip_handle *h, int mode, int column, float energy_threshold, float energy_mean_scale,
                      int frames_context, float proportion_threshold);
/* The decision's direct entry: d_rows float32 [seg_offsets[n_segs]][row_width] (rows before seg_offsets[0] not read),
 * d_voiced one uint8 0 / 1 per row at the same row indices; bytes outside the segments are left untouched.  Segment k =
 * rows seg_offsets[k] .. seg_offsets[k + 1] (host array, n_segs + 1 entries, must not decrease).  row_width 1..64,
 * column 0..row_width - 1, d_rows 4-byte aligned, the rows and the bytes must not overlap, the four parameters in the
 * ranges above: otherwise MFCC_HIP_ERROR_INVALID_PARAM.  Asynchronous on the handle's stream; n_segs = 0 is a no-op. */
int  mfcc_hip_vad_dev(mfcc_hip_handle *h, const void *d_rows, int row_width, int column, const size_t *seg_offsets,
                      size_t n_segs, float energy_threshold, float energy_mean_scale, int frames_context,
                      float proportion_threshold, void *d_voiced);
/* The selection's direct entry: copies the rows of d_in ([seg_offsets[n_segs]][row_width] float32) whose d_voiced byte
 * is not 0 to d_out, packed back to back from row 0 of d_out, in order; rows of d_out beyond out_offsets[n_segs] are
 * untouched.  out_offsets (HOST array, n_segs + 1 entries) receives the row range of every segment in the packed result:
 * this call therefore SYNCHRONIZES the handle's stream before it returns.  row_width 1..192 (three times the widest static
 * row), both row pointers 4-byte aligned, d_out must not overlap the rows or the bytes read: otherwise
 * MFCC_HIP_ERROR_INVALID_PARAM.  out_capacity_rows below the count of ALL rows of the segments
 * (seg_offsets[n_segs] - seg_offsets[0]): MFCC_HIP_ERROR_BUFFER_SMALL before anything runs.  n_segs = 0 is a no-op. */
int  mfcc_hip_select_dev(mfcc_hip_handle *h, const void *d_in, int row_width, const void *d_voiced,
                         const size_t *seg_offsets, size_t n_segs, void *d_out, size_t out_capacity_rows,
                         size_t *out_offsets);

/* ---- per-channel energy normalization, PCEN --------------------------------------------
 * An automatic gain control per mel band in place of the log (Wang et al. 2017): a first-order smoother over time and a
 * root compression.  It runs on the log-mel rows of an MFCC_HIP_OUTPUT_LOGMEL handle, [frame][n_mel], log2 energies;
 * a segment is one channel of a dense call or one utterance of a ragged one.  With E_t = 2^x_t (a non-finite x, the -inf
 * of a silent band included, counts as E = 0: a legitimate zero here, not a hole), per column:
 *     M_0 = E_0,   M_t = (1 - s) M_{t-1} + s E_t,   y_t = (E_t / (eps + M_t)^alpha + delta)^r - delta^r
 * The order of operations is fixed by tiles of T = MFCC_HIP_PCEN_TILE frames counted from the segment's first row
 * (frame t = slot k = t % T of tile i = t / T), all in fp32, nothing contracted but the fmaf's named:
 *     constants (mfcc_hip_pcen_constants, float64 rounded once):  a = (float)(1 - (double)s),
 *                 A_k = (float)((1 - (double)s)^(k + 1)), k = 0..T-1,  D_r = (float)(delta^r)
 *     local smoother  L_{i,-1} = 0,  L_{i,k} = fmaf(a, L_{i,k-1}, s * E_t)
 *     carry           C_0 = E_0,  M_t = fmaf(A_k, C_i, L_{i,k}),  C_{i+1} = M of slot T - 1 of tile i
 *     output          g = log2(eps + M_t),  q = exp2(-alpha * g),  u = fmaf(E_t, q, delta),
 *                     y_t = exp2(r * log2(u)) - D_r          (u = 0, only possible with delta = 0, gives y = 0)
 * exp2 / log2 are the hardware's (v_exp_f32 / v_log_f32, the log the mel kernels use): log2 energies are expected in
 * [-126, 127] or non-finite.  Every finite result is within |y - ref| <= c (|ref| + delta^r) of the float64 definition
 * (c: DESIGN.md section 4.13) and a segment's bits depend on its rows, the row width and the parameters alone: the same
 * from every entry point, any chunking of a host call, any 4-byte alignment, any run.
 * eps and delta are in the units of the handle's mel energies, which carry power_scale (default 512 with int16 samples:
 * speech bands are roughly 1e2 .. 1e7; librosa.pcen's defaults assume input scaled by 2^31).  Nothing is rescaled.
 * s is the smoother's coefficient itself (librosa: b).                                                            */
#define MFCC_HIP_PCEN_TILE 128
typedef struct mfcc_hip_pcen {
    uint32_t struct_size;   /* sizeof(mfcc_hip_pcen) */
    float s;                /* smoother coefficient, 0 < s <= 1              (0.025) */
    float alpha;            /* gain normalization strength, 0 <= alpha <= 1  (0.98)  */
    float delta;            /* bias before the root, delta >= 0              (2)     */
    float r;                /* root, 0 < r <= 1                              (0.5)   */
    float eps;              /* floor of the smoother, eps > 0                (1e-6)  */
    int32_t reserved[3];    /* must be 0 */
} mfcc_hip_pcen;
/* Host-only, no GPU needed.  defaults: the paper's values.  constants: decay[MFCC_HIP_PCEN_TILE] = A_k, *a, *delta_r as
 * defined above (any of the three may be NULL).  A NULL block, a wrong struct_size, a non-zero reserved word, a value
 * that is not finite or lies outside its range: MFCC_HIP_ERROR_INVALID_PARAM.                                    */
int  mfcc_hip_pcen_defaults(mfcc_hip_pcen *p);
int  mfcc_hip_pcen_constants(const mfcc_hip_pcen *p, float *decay, float *a, float *delta_r);
/* The handle's PCEN applies to every float call enqueued after it, like its normalization.  The passes of a call run in
 * this order: the MFCC kernels; the VAD decision on the raw log-mel rows (its thresholds are in log2 units); PCEN in
 * place; normalization (per segment or sliding); deltas; selection.  p = NULL switches it off: the state after
 * mfcc_hip_create, every entry point gives the bits it gave before.  A handle whose output is not
 * MFCC_HIP_OUTPUT_LOGMEL: MFCC_HIP_ERROR_UNSUPPORTED; live streaming sessions: MFCC_HIP_ERROR_BUSY; a bad block:
 * MFCC_HIP_ERROR_INVALID_PARAM.  A PCEN handle refuses what a normalizing handle refuses, for the same reasons (the
 * smoother of a shard or of a session is not the stream's): the fixed-point entry points, mfcc_hip_stream_create,
 * mfcc_hip_bank_create(_online, _online_pcen: a bank's PCEN is its own, on a raw handle), mfcc_hip_convert_wav(s) and
 * mfcc_hip_process_i16_dev with halo = 1 return MFCC_HIP_ERROR_UNSUPPORTED.  In the host-buffer entry points it takes
 * the route of per-segment normalization: frame-range chunks of a long channel are not independent.
 * mfcc_hip_time_dev times the pass too.  The parameter block of the handle and the ABI version are unchanged.     */
int  mfcc_hip_set_pcen(mfcc_hip_handle *h, const mfcc_hip_pcen *p);
/* The kernels' direct entry: PCEN of float32 rows [seg_offsets[n_segs]][row_width] in HBM in place, segment k = rows
 * seg_offsets[k] .. seg_offsets[k + 1] (host array, n_segs + 1 entries, must not decrease; rows before seg_offsets[0]
 * and behind the last segment are not touched).  row_width 1..64, d_rows 4-byte aligned, any handle.  Asynchronous on
 * the handle's stream; n_segs = 0 is a no-op.  E.g. the gathered rows of a frame-range-sharded stream.            */
int  mfcc_hip_pcen_dev(mfcc_hip_handle *h, void *d_rows, int row_width, const size_t *seg_offsets, size_t n_segs,
                       const mfcc_hip_pcen *p);

/* the settings of section "filterbank post-passes" */
typedef struct mfcc_hip_filterbank_post {
    uint32_t struct_size;          /* sizeof(mfcc_hip_filterbank_post) */
    int32_t  normalize;            /* enum mfcc_hip_normalize */
    int32_t  normalize_window;     /* 0: per segment */
    int32_t  normalize_min_window;
    int32_t  normalize_center;
    int32_t  delta_order;          /* 0 .. 2 */
    int32_t  delta_window;         /* 1 .. MFCC_HIP_MAX_DELTA_WINDOW */
    int32_t  pcen_on;              /* 0 / 1 */
    mfcc_hip_pcen pcen;
    int32_t  reserved[4];          /* must be 0 */
} mfcc_hip_filterbank_post;

int    mfcc_hip_set_filterbank_post(mfcc_hip_handle *h, const mfcc_hip_filterbank_post *p /* NULL: none */);
/* floats of a row of the three filterbank compute entries: n_bands * (1 + delta_order); 0 without a matrix or handle */
size_t mfcc_hip_filterbank_row_width(const mfcc_hip_handle *h);

/* ---- sample formats ----------------------------------------------------------------------
 * What a sample pointer holds is a property of the handle.  Every format is decoded to int16 on the device by one
 * streaming pass (decode_samples_kernel) in front of the kernels; from there on a call takes exactly the route it takes
 * on int16 input.  The rules, all integers 32-bit two's complement; b is the byte, w the 32-bit word, x the float:
 *   ULAW   (ITU-T G.711 mu-law)   u = ~b & 0xff;  t = (((u & 0x0f) << 3) + 0x84) << ((u & 0x70) >> 4);
 *                                 s = (u & 0x80) ? 0x84 - t : t - 0x84
 *                                 (0x00 -> -32124, 0x80 -> +32124, 0x7f and 0xff -> 0)
 *   ALAW   (ITU-T G.711 A-law)    a = b ^ 0x55;  seg = (a & 0x70) >> 4;  t = (a & 0x0f) << 4;
 *                                 seg == 0: t += 8;  seg == 1: t += 0x108;  otherwise t = (t + 0x108) << (seg - 1);
 *                                 s = (a & 0x80) ? t : -t
 *                                 (0x55 -> -8, 0xd5 -> +8, 0x2a -> -32256, 0xaa -> +32256)
 *   U8     (offset binary)        s = (b - 128) << 8
 *   I2S32                         s = (int16_t)(uint16_t)((uint32_t)w >> 10): bits 25..10 of the word, what the
 *                                 reference's I2S receiver keeps, `source.data.eq(da_shreg[-22:-6])`  mfcc/io/i2s_mic.py:62
 *   S32                           s = w >> 16, arithmetic shift
 *   F32                           v = x * 32768.0f (one fp32 multiply);  r = rintf(v) (ties to even);
 *                                 s = r < -32768 ? -32768 : r > 32767 ? 32767 : (int)r;  NaN gives 0, +-inf saturate
 *   S16                           identity                                                                          */
enum mfcc_hip_sample_format {
    MFCC_HIP_SAMPLE_S16   = 0,  /* int16: the state after mfcc_hip_create, today's bits */
    MFCC_HIP_SAMPLE_ULAW  = 1,  /* 1 byte, ITU-T G.711 mu-law */
    MFCC_HIP_SAMPLE_ALAW  = 2,  /* 1 byte, ITU-T G.711 A-law */
    MFCC_HIP_SAMPLE_U8    = 3,  /* 1 byte, offset binary (8-bit WAV) */
    MFCC_HIP_SAMPLE_I2S32 = 4,  /* 4 bytes, an I2S word as the reference's receiver cuts it */
    MFCC_HIP_SAMPLE_S32   = 5,  /* 4 bytes, int32 full scale */
    MFCC_HIP_SAMPLE_F32   = 6   /* 4 bytes, float in [-1, 1) */
};
/* bytes of one sample: 2, 1, 1, 1, 4, 4, 4; 0 for an unknown format */
size_t mfcc_hip_sample_size(int format);
/* Host only, no GPU, no handle: the rules above on n samples at `in` (any alignment) -> out[n].  An unknown format, or a
 * NULL pointer with n > 0: MFCC_HIP_ERROR_INVALID_PARAM.  For callers and for the CPU tests. */
int  mfcc_hip_decode_host(int format, const void *in, size_t n, int16_t *out);
/* The kernels' direct entry: n samples at d_in (aligned to the format's sample size; 1-byte formats take any address)
 * -> int16 at d_out (2-byte aligned).  The two byte ranges must not overlap; a misaligned or NULL pointer, an overlap or
 * an unknown format: MFCC_HIP_ERROR_INVALID_PARAM.  Asynchronous on the handle's stream; n = 0 is a no-op that looks at
 * no pointer; any handle (its own format is not read).  S16 is a copy. */
int  mfcc_hip_decode_dev(mfcc_hip_handle *h, int format, const void *d_in, size_t n, void *d_out);
/* The handle's input format, applied to every call enqueued after it: EVERY sample pointer of every entry point is read
 * in it -- dense, ragged, host and device buffers, float and fixed, mfcc_hip_stream_push, mfcc_hip_bank_push / _push_dev
 * and mfcc_hip_time_dev (which times the decode too).  The declared `const int16_t *` stays; the caller casts.  Sample
 * counts, strides, `offsets` and `halo` keep counting SAMPLES, not bytes; the halo sample is decoded like any other.
 * The result is, bit for bit, what the same call returns on an S16 handle given mfcc_hip_decode_host of the input.
 * A device pointer must be aligned to the format's sample size, else MFCC_HIP_ERROR_INVALID_PARAM.
 * A call on a handle with another format than S16 needs 2 * samples bytes of device memory for the decoded samples (a
 * scratch area of the handle that grows on demand and is never shrunk; a dense strided call rounds every channel up to 8
 * samples): MFCC_HIP_ERROR_NO_MEM if it cannot be had.  The host-buffer entry points copy the raw bytes through the
 * same chunked copy pipeline (chunks are cut by sample count, as for S16) and decode every chunk on the device.
 * MFCC_HIP_SAMPLE_S16 is the state after mfcc_hip_create: no decode is enqueued, every entry point gives the bits and
 * the launches it gives without this call, mfcc_hip_kernel_name does not depend on the format.
 * A session or a bank reads its samples in the format its handle had when it was created: like the other setters this
 * call answers MFCC_HIP_ERROR_BUSY while sessions live.  Unknown format or NULL handle: MFCC_HIP_ERROR_INVALID_PARAM.
 * mfcc_hip_convert_wav(s) read 16-bit PCM files whatever the format.  MFCC_HIP_ERROR_BUFFER_SMALL and
 * MFCC_HIP_ERROR_INVALID_PARAM still consume nothing.  The parameter block and the ABI version are unchanged. */
int  mfcc_hip_set_sample_format(mfcc_hip_handle *h, int format);
/* the handle's format (MFCC_HIP_SAMPLE_S16 for NULL) */
int  mfcc_hip_sample_format(const mfcc_hip_handle *h);

/* ---- sample rates ------------------------------------------------------------------------
 * An integer polyphase resampler: int16 in, int16 out, the same bits from the host entry and from the kernel.
 * in_rate, out_rate: positive integers.  g = gcd(in_rate, out_rate), L = out_rate / g, M = in_rate / g.
 * Constants: Z = 16 zero crossings, Kaiser beta = 7.5, roll-off 0.90.  s = min(1, L / M), fc = 0.90 s,
 * H = ceil(Z / s) (in integers: 16 for L >= M, else (16 M + L - 1) div L), K = 2 H taps per phase, L phases.
 * Design, in double:  g(d) = fc sinc(fc d) I0(beta sqrt(1 - (d / H)^2)) / I0(beta) for |d| <= H, else 0, with
 *   sinc(x) = sin(pi x) / (pi x) and I0 the modified Bessel function of order 0.
 * Phase p, tap k: d = k - H + 1 - p / L.
 * Table T[p][k], int16, Q14: rint(16384 g / sum_k g) per phase (ties to even); the residual 16384 - sum_k T[p][k] is
 *   then added to the phase's largest tap (the first of them), so every phase sums to exactly 16384.
 * Output m >= 0:  q = (m M) div L,  p = (m M) mod L  (the product 64-bit),
 *   acc = sum_{k < K} T[p][k] x[q - H + 1 + k], with x[i] = 0 outside [0, n), a 32-bit integer,
 *   y[m] = sat16((acc + 8192) >> 14), arithmetic shift.
 *   The table is only accepted if sum_k |T[p][k]| <= 65535 for every phase, so acc cannot wrap on any int16 input.
 * Count: n_out = (n L + M - 1) div M.
 * MFCC_HIP_ERROR_UNSUPPORTED if L > 1024, M > 1024 or the table (2 L K bytes) exceeds 64 KiB;
 * MFCC_HIP_ERROR_INVALID_PARAM for a rate <= 0, a NULL pointer that is needed, or n >= 2^40.
 * in_rate == out_rate is L = M = 1, K = 32: the roll-off filter at the rate's own Nyquist, NOT a copy. */
/* L, M and K of a ratio (any may be NULL).  Host only. */
int  mfcc_hip_resample_geometry(int in_rate, int out_rate, int *L, int *M, int *K);
/* *n_out = outputs of n input samples.  Host only. */
int  mfcc_hip_resample_count(int in_rate, int out_rate, size_t n, size_t *n_out);
/* the table, L rows of K taps: *n (may be NULL) = L K also on MFCC_HIP_ERROR_BUFFER_SMALL (cap < L K, nothing written;
 * buf may then be NULL).  Host only. */
int  mfcc_hip_resample_taps(int in_rate, int out_rate, int16_t *buf, size_t cap, size_t *n);
/* Host only, no GPU, no handle: the rule on the n samples at `in` -> out[n_out].  cap < n_out:
 * MFCC_HIP_ERROR_BUFFER_SMALL, nothing written.  For callers and for the CPU tests. */
int  mfcc_hip_resample_host(int in_rate, int out_rate, const int16_t *in, size_t n, int16_t *out, size_t cap);
/* The kernel's direct entry: n int16 at d_in -> n_out int16 at d_out, both 2-byte aligned at any int16 offset, the byte
 * ranges [d_in, d_in + 2 n) and [d_out, d_out + 2 n_out) not overlapping (a misaligned or NULL pointer or an overlap:
 * MFCC_HIP_ERROR_INVALID_PARAM); cap < n_out: MFCC_HIP_ERROR_BUFFER_SMALL, nothing enqueued.  Asynchronous on the
 * handle's stream; n = 0 is a no-op that looks at no pointer; any handle (its own rate and format are not read).  The
 * handle keeps the table of the last ratio on its device: a call with another ratio builds and copies a new one and
 * waits for the stream once. */
int  mfcc_hip_resample_dev(mfcc_hip_handle *h, int in_rate, int out_rate, const void *d_in, size_t n, void *d_out, size_t cap);
/* The handle's input rate, applied to every call enqueued after it: every sample pointer of the one-shot entry points
 * holds samples at in_rate, and the call returns, bit for bit, what the same handle without an input rate returns on
 * mfcc_hip_resample_host(in_rate, params.sample_rate) of the (decoded) input.  The order is decode -> resample ->
 * route; the resampled samples go to a scratch area of the handle that grows on demand and is never shrunk (2 bytes per
 * output sample, a dense strided call rounds every channel up to 8 samples; MFCC_HIP_ERROR_NO_MEM if it cannot be had).
 * in_rate = 0 or params.sample_rate: off, the state after mfcc_hip_create -- no pass is enqueued, every entry point is
 * the code it was.  Sample counts, strides and `offsets` keep counting the CALLER's samples; frame counts are those of
 * the resampled lengths, count_frames(mfcc_hip_resample_count(n)).
 *   - dense device calls and mfcc_hip_time_dev (which times the pass too): every channel on its own, zeros outside it;
 *   - ragged device calls: every utterance on its own, zeros outside it, by one launch; the new offsets on the host;
 *   - the fixed-point entry points likewise;
 *   - the host-buffer entry points take the unchunked route: one copy in, the device route, one copy back
 *     (MFCC_HIP_ERROR_NO_MEM where that does not fit);
 *   - mfcc_hip_convert_wav(s) expect a WAV of in_rate.
 * MFCC_HIP_ERROR_UNSUPPORTED with a rate set: dense calls with halo = 1 (a shard's edge would need its neighbour's
 * samples), mfcc_hip_stream_create and every mfcc_hip_bank_create* (a line's conversion keeps state between pushes).
 * A ratio mfcc_hip_resample_geometry refuses is refused alike; in_rate < 0 or a NULL handle:
 * MFCC_HIP_ERROR_INVALID_PARAM; MFCC_HIP_ERROR_BUSY while sessions, banks or gates live.  The call copies the ratio's
 * table to the device (and waits for the handle's stream once if it held another ratio's). */
int  mfcc_hip_set_input_rate(mfcc_hip_handle *h, int in_rate);
/* the handle's input rate, 0 where none is set (and for NULL) */
int  mfcc_hip_input_rate(const mfcc_hip_handle *h);

/* Live lines: the streaming form of the same rule, an object of its own that is composed with a bank on the device
 * (as mfcc_hip_gate is, behind one).  After c input samples a line has emitted E(c) = count(max(c - H, 0)) outputs: the
 * latency is H input samples.  The line keeps c on the host and its last K - 1 samples on the device.  A flush emits
 * the outputs E(c) .. count(c) - 1 on zeros beyond the end and puts the line back to c = 0.  Pushes plus flush,
 * concatenated, are the one-shot result of the concatenated chunks, bit for bit, whatever the chunking.
 * The chunks are in sample_format and are decoded in front, like a bank's; the int16 output and out_offsets go straight
 * into mfcc_hip_bank_push_dev of an S16 handle's bank at out_rate (a line's flush output is pushed to the bank before
 * the bank's own flush).  The object lives on the handle's device and stream and uses its scratch areas; while it lives
 * the handle's setters answer MFCC_HIP_ERROR_BUSY and mfcc_hip_destroy is deferred, as with a session. */
typedef struct mfcc_hip_resampler mfcc_hip_resampler;
/* n_lines >= 1 lines from c = 0.  A ratio mfcc_hip_resample_geometry refuses is refused alike; an unknown format, no
 * line or a NULL pointer: MFCC_HIP_ERROR_INVALID_PARAM. */
int  mfcc_hip_resampler_create(mfcc_hip_handle *h, size_t n_lines, int sample_format, int in_rate, int out_rate,
                               mfcc_hip_resampler **out);
void mfcc_hip_resampler_destroy(mfcc_hip_resampler *r);
/* seen[n_lines]: every line's c */
int  mfcc_hip_resampler_seen(const mfcc_hip_resampler *r, size_t *seen);
/* the listed lines (distinct; NULL: every line) back to c = 0 without output.  Host only, takes effect in stream order. */
int  mfcc_hip_resampler_reset(mfcc_hip_resampler *r, const size_t *lines, size_t n);
/* From lengths alone, no device: out_offsets[n_lines + 1] of lines that have seen seen[u] samples,
 *   flush = 0: for a push of the chunks offsets[u] .. offsets[u + 1]:   E(seen + len) - E(seen) outputs each;
 *   flush != 0: for a flush behind those chunks (offsets NULL: no chunks): count(seen + len) - E(seen + len) each. */
int  mfcc_hip_resampler_plan(int in_rate, int out_rate, const size_t *seen, const size_t *offsets, size_t n_lines, int flush,
                             size_t *out_offsets);
/* One chunk per line, line u = samples offsets[u] .. offsets[u + 1] of d_in (in sample_format, aligned to its sample
 * size; a chunk may be empty), one launch (two with a decode).  Line u's outputs land at d_out[out_offsets[u] ..
 * out_offsets[u + 1]) (int16, 2-byte aligned), out_offsets[n_lines + 1] is filled on the host before the call returns:
 * asynchronous on the handle's stream, no synchronization.  cap (in int16) below out_offsets[n_lines]:
 * MFCC_HIP_ERROR_BUFFER_SMALL with out_offsets filled; that and MFCC_HIP_ERROR_INVALID_PARAM (decreasing offsets, a NULL
 * or misaligned pointer that is needed) consume nothing and enqueue nothing.  d_in and d_out must not overlap. */
int  mfcc_hip_resampler_push_dev(mfcc_hip_resampler *r, const void *d_in, const size_t *offsets, void *d_out, size_t cap,
                                 size_t *out_offsets);
/* The end of the listed lines (distinct; NULL: every line, then n is ignored): line lines[i]'s last outputs at
 * d_out[out_offsets[i] .. out_offsets[i + 1]), out_offsets[n + 1]; the lines are at c = 0 afterwards.  Asynchronous;
 * refusals as above. */
int  mfcc_hip_resampler_flush_dev(mfcc_hip_resampler *r, const size_t *lines, size_t n, void *d_out, size_t cap,
                                  size_t *out_offsets);

/* ---- centring ---------------------------------------------------------------------------
 * The framing of librosa.stft / torch.stft / torchaudio / Whisper (center=True): frame t is centred on sample t hop,
 * the signal's edges are reflected (or zero-padded), and n samples give 1 + n div hop frames.
 * L: the handle's frame length (nfft, or frame_length of a framed handle), hop: its hop, n: the samples of one channel
 * or utterance at the handle's own rate (after decode and resample).  All divisions are integer divisions.
 *     PL    = nfft / 2 - (nfft - L) / 2                         (= ceil(L / 2); torch.stft's placement of a short window)
 *     F(n)  = 0               if n <= PL (REFLECT)  or  n == 0 (ZEROS)
 *           = 1 + n / hop     otherwise
 *     N'(n) = (F - 1) hop + L                                   (0 when F = 0)
 *     p[i], 0 <= i < N':   j = i - PL
 *           REFLECT:  j < 0 -> -j;  j >= n -> 2 (n - 1) - j     (the edge sample is not repeated: numpy / torch "reflect")
 *           ZEROS:    0 where j < 0 or j >= n
 *           else      x[j]
 * With n > PL one reflection suffices on both sides.  The rows of a centred handle are the rows the same handle gives
 * uncentred (MFCC_HIP_PAD_NOTEBOOK) on p, bit for bit, F of them.  Pre-emphasis runs over p with p[-1] = 0. */
enum mfcc_hip_center { MFCC_HIP_CENTER_OFF = 0, MFCC_HIP_CENTER_REFLECT = 1, MFCC_HIP_CENTER_ZEROS = 2 };
/* The geometry: *n_frames = F(n), *left = PL, *padded = N'(n) (any may be NULL).  frame_length as in
 * mfcc_hip_create_framed (0: nfft); mode REFLECT or ZEROS.  Bad params, frame length or mode:
 * MFCC_HIP_ERROR_INVALID_PARAM.  Host only, no GPU. */
int  mfcc_hip_center_geometry(const mfcc_hip_params *p, int frame_length, int mode, size_t n, size_t *n_frames, size_t *left,
                              size_t *padded);
/* The rule on int16: the n samples at `in` -> out[N'].  *n_out (may be NULL) = N', also on MFCC_HIP_ERROR_BUFFER_SMALL
 * (cap < N', nothing written).  N' = 0 looks at no pointer; else a NULL in or out: MFCC_HIP_ERROR_INVALID_PARAM.  Host
 * only, no GPU, no handle. */
int  mfcc_hip_center_host(const mfcc_hip_params *p, int frame_length, int mode, const int16_t *in, size_t n, int16_t *out,
                          size_t cap, size_t *n_out);
/* The kernel's direct entry on one row, with the handle's L and hop: n samples in `format` (any of enum
 * mfcc_hip_sample_format; the decode rule is applied while padding) at d_in, aligned to the format's sample size -> N'
 * int16 at d_out, 2-byte aligned at any int16 offset.  *n_out (may be NULL) = N', also on MFCC_HIP_ERROR_BUFFER_SMALL
 * (cap < N', nothing enqueued).  A NULL or misaligned pointer that is needed, an overlap of the two byte ranges, an
 * unknown format, a mode other than REFLECT or ZEROS: MFCC_HIP_ERROR_INVALID_PARAM.  Asynchronous on the handle's stream;
 * N' = 0 is a no-op.  The handle's own mode, format and rate are not read. */
int  mfcc_hip_center_dev(mfcc_hip_handle *h, int mode, int format, const void *d_in, size_t n, void *d_out, size_t cap,
                         size_t *n_out);
/* The handle's mode, applied to every call enqueued after it: every one-shot float entry point (mfcc_hip_process_i16,
 * _i16_dev, _ragged_i16, _ragged_i16_dev, mfcc_hip_spectrum_*, mfcc_hip_fbank_*, mfcc_hip_time_dev, mfcc_hip_convert_wav(s)
 * in float) returns, bit for bit, what the same handle with MFCC_HIP_CENTER_OFF returns on p of every channel or
 * utterance.  The order is decode -> resample -> centre -> route: a handle with a sample format and no input rate runs
 * ONE pass in front (decode and centre together), a plain int16 handle one, a handle with an input rate three.  The
 * padded samples go to a scratch area of the handle that grows on demand and is never shrunk (2 bytes per padded sample,
 * a dense call of several channels rounds every channel up to 8 samples; MFCC_HIP_ERROR_NO_MEM if it cannot be had).
 * Sample counts, strides and `offsets` keep counting the CALLER's samples; frame counts and frame_offsets count F.
 *   - ragged calls: an utterance with F = 0 (REFLECT: up to PL samples) gives no rows and the call succeeds;
 *   - normalization, sliding normalization, deltas, PCEN and VAD run behind the kernels on the F rows as they do on any;
 *   - the host-buffer entry points take the unchunked route: one copy in, the device route, one copy back
 *     (MFCC_HIP_ERROR_NO_MEM where that does not fit).
 * MFCC_HIP_CENTER_OFF: the state after mfcc_hip_create -- no pass is enqueued, every entry point is the code it was.
 * MFCC_HIP_ERROR_UNSUPPORTED, before anything is read or allocated, on a centred handle: dense calls with halo = 1 (a
 * shard of a longer stream has no edges), every fixed-point entry point (the RTL's framing is its contract),
 * mfcc_hip_stream_create, every mfcc_hip_bank_create* and mfcc_hip_resampler_create (a centred line must hold back its
 * first PL + 1 samples and flushes several frames).  mfcc_hip_set_center itself: MFCC_HIP_ERROR_UNSUPPORTED for a mode
 * other than OFF on a MFCC_HIP_PAD_STREAM handle; MFCC_HIP_ERROR_BUSY while sessions, banks or gates live; another value
 * or a NULL handle: MFCC_HIP_ERROR_INVALID_PARAM.  A refused call leaves the handle as it was.  The parameter block and
 * the ABI version are unchanged. */
int  mfcc_hip_set_center(mfcc_hip_handle *h, int mode);
/* the handle's mode, MFCC_HIP_CENTER_OFF for NULL */
int  mfcc_hip_center(const mfcc_hip_handle *h);

/* name of the kernel symbol process_*_dev launches for this handle (to match rocprofv3 rows).  A log-mel handle runs
 * the log-mel instantiation of the kernel named (the default form: MFCC_HIP_FUSED512 / MFCC_HIP_FUSED1024 do not
 * apply to it) */
const char *mfcc_hip_kernel_name(const mfcc_hip_handle *h, int fixed);

/* ---- file-level convenience: mfcc_convert(sess, wav_in, mfcc_out)  software/main.c:100 --- */

/* 16-bit mono PCM WAV at p->sample_rate -> raw int16 LE `.mfcc` file [frame][n_cep]
 * (fixed = 1: RTL-exact values, what the FPGA would have written; fixed = 0: float
 * coefficients truncated to int16 like software/lift.py:39).  *n_frames_out may be NULL. */
int  mfcc_hip_convert_wav(mfcc_hip_handle *h, const char *wav_in, const char *mfcc_out,
                          int fixed, size_t *n_frames_out);

/* The same for n_files files at once -- the whole directory walk of show_dir_content (main.c:206-247)
 * as ONE ragged launch; every file is an independent stream, the files written are byte-identical to
 * n_files calls of mfcc_hip_convert_wav.  n_frames_each (n_files entries) may be NULL. */
int  mfcc_hip_convert_wavs(mfcc_hip_handle *h, const char *const *wav_in, const char *const *mfcc_out,
                           size_t n_files, int fixed, size_t *n_frames_each);

/* ---- online / streaming session: the core's real interface is a stream with state --------------
 * `MFCC.sink` (samples in), `MFCC.source` (coefficients out, one `first..last` burst per frame) and
 * `MFCC.reset` (mfcc/core/mfcc.py:28-30,116); the targets feed it chunk by chunk
 * (mfcc/targets/wav2mfcc.py:27-42: bit 31 of a word = soft reset; mic2mfcc.py:19-30: I2S samples
 * through a FIFO) and the receiver reads columns as they come (software/cepstrum.c:93-159).
 * A session carries exactly the core's cross-frame state on the device between calls: the one
 * pre-emphasis history sample (preemph.py:20-28) and the samples of the frame in progress (the ring
 * buffer of frame.py:65-153, at most nfft - 1 + hop of them).  Any chunking of a stream gives, frame
 * for frame, bit for bit, the result of the one-shot calls above (tests/test_gpu_parity.py).
 * Several sessions may share a handle; like the handle they are not thread-safe.                 */
typedef struct mfcc_hip_stream mfcc_hip_stream;

/* fixed = 0: float contract (out = float), fixed = 1: RTL contract (out = int16_t) */
int  mfcc_hip_stream_create(mfcc_hip_handle *h, int fixed, mfcc_hip_stream **out);
/* frees the session's device buffers; if its handle was already given to mfcc_hip_destroy and this was the
 * handle's last session, the handle is freed here (see the lifetime rule at mfcc_hip_destroy) */
void mfcc_hip_stream_destroy(mfcc_hip_stream *s);
/* `mfcc_softreset` (software/main.c:21-34): drop the pending samples, history back to 0 */
int  mfcc_hip_stream_reset(mfcc_hip_stream *s);
/* samples waiting for their frame to complete (0 <= pending < nfft between calls) */
size_t mfcc_hip_stream_pending(const mfcc_hip_stream *s);
/* upper bound of the frames a push of n samples can complete: (pending + n) / hop + 1 */
size_t mfcc_hip_stream_max_frames(const mfcc_hip_stream *s, size_t n);
/*
 * Feed n samples (host buffer); every frame they complete is computed and written to `out`
 * ([frames][n_cep], float or int16_t by the session's contract; out_capacity in elements).
 * *n_frames_out = frames written (may be 0).  MFCC_HIP_ERROR_BUFFER_SMALL leaves the session
 * untouched.  Synchronous.
 */
int  mfcc_hip_stream_push(mfcc_hip_stream *s, const int16_t *samples, size_t n, void *out,
                          size_t out_capacity, size_t *n_frames_out);
/*
 * End of the stream.  MFCC_HIP_PAD_STREAM: the host driver keeps feeding zeros until the frame
 * holding the last sample is out (main.c:134-144) -- one more, zero-padded frame is written.
 * MFCC_HIP_PAD_NOTEBOOK: the tail samples are dropped (notebook cell 9), nothing is written.
 * Either way the session is back in its reset state afterwards.
 */
int  mfcc_hip_stream_flush(mfcc_hip_stream *s, void *out, size_t out_capacity, size_t *n_frames_out);

/* ---- stream bank: many online sessions advanced by one launch ---------------------------------
 * A bank is n_streams independent sessions (N live lines: a microphone array, telephony) whose state
 * lives on the device in one allocation: per stream the pre-emphasis history sample and the samples of
 * the frame in progress.  One push takes a ragged batch of chunks, one per stream, and advances all of
 * them with one launch of the frame kernels; every stream gets exactly the rows a session of its own
 * would have returned for the same chunks, bit for bit.  The samples may already lie in device memory
 * (mfcc_hip_bank_push_dev).  The number of samples each stream holds back (0 <= pending < nfft) depends
 * on lengths only and is mirrored on the host: planning a push needs no device traffic.
 * Cost of a push: the streams that complete frames run as channels of ONE launch of nfmax frames each,
 * nfmax = the most frames any of them completes.  Equal chunks (lines in lockstep) compute exactly the
 * frames returned and write them straight into `out`; a mixed push computes active x nfmax frames and
 * gathers the ones that count; a straggler pushed alone costs only its own frames.
 * A bank counts as a streaming session of its handle: the lifetime rule at mfcc_hip_destroy and the
 * MFCC_HIP_ERROR_BUSY of the mfcc_hip_set_* calls hold for it, and mfcc_hip_bank_create refuses what
 * mfcc_hip_stream_create refuses (MFCC_HIP_ERROR_UNSUPPORTED: a handle with normalization, deltas or VAD;
 * fixed = 1 where the fixed-point path does not cover the parameters, a log-mel handle included).
 * Banks, sessions and one-shot calls may share a handle; like the handle a bank is not thread-safe.  */
typedef struct mfcc_hip_bank mfcc_hip_bank;

/* fixed as for mfcc_hip_stream_create; n_streams >= 1.  Every stream starts in the reset state. */
int    mfcc_hip_bank_create(mfcc_hip_handle *h, int fixed, size_t n_streams, mfcc_hip_bank **out);
/* frees the bank's device buffers (waits for its work first); frees the handle too if that was already
 * given to mfcc_hip_destroy and this was its last session or bank */
void   mfcc_hip_bank_destroy(mfcc_hip_bank *b);
/* n_streams (0 for NULL) */
size_t mfcc_hip_bank_size(const mfcc_hip_bank *b);
/* pending[n_streams]: the samples every stream holds back for its frame in progress */
int    mfcc_hip_bank_pending(const mfcc_hip_bank *b, size_t *pending);
/*
 * The plan of a push, host only (no GPU, no handle).  Stream u has pending[u] < nfft samples and receives
 * offsets[u + 1] - offsets[u] more; with total = pending + new it completes
 *   nf = total >= nfft ? (total - nfft) / hop + 1 : 0   frames and keeps   total - nf * hop  (< nfft).
 * frame_offsets[n_streams + 1]: running sum of nf, the row range of every stream in the result of the
 * push; pending_after[n_streams] may be NULL.  Decreasing offsets or pending[u] >= nfft:
 * MFCC_HIP_ERROR_INVALID_PARAM (frame_offsets is filled up to that stream).
 */
int    mfcc_hip_bank_plan(const mfcc_hip_params *p, const size_t *pending, const size_t *offsets,
                          size_t n_streams, size_t *frame_offsets, size_t *pending_after);
/* ... for banks of a framed handle (mfcc_hip_create_framed): the frame length L takes nfft's place, pending[u] < L */
int    mfcc_hip_bank_plan_framed(const mfcc_hip_params *p, int frame_length, const size_t *pending, const size_t *offsets,
                                 size_t n_streams, size_t *frame_offsets, size_t *pending_after);
/*
 * Feed every stream a chunk: stream u gets samples[offsets[u] .. offsets[u + 1]) (n_streams + 1 offsets,
 * not decreasing; a range may be empty).  out: [sum frames][n_cep], float or int16_t by the bank's
 * contract, out_capacity in elements; stream u's rows are rows frame_offsets[u] .. frame_offsets[u + 1].
 * MFCC_HIP_ERROR_BUFFER_SMALL and MFCC_HIP_ERROR_INVALID_PARAM (decreasing offsets): frame_offsets is
 * filled where it can be, NOTHING is consumed and the bank is as before.
 * mfcc_hip_bank_push: host buffers, synchronous (one copy in, the device push, one copy out).
 * mfcc_hip_bank_push_dev: device buffers, asynchronous on the handle's stream (mfcc_hip_set_stream); no
 * synchronize and no device-to-host copy anywhere in it, no per-stream copy or launch.  d_samples and
 * d_out must stay valid until the stream has run it; offsets is read before the call returns.
 */
int    mfcc_hip_bank_push(mfcc_hip_bank *b, const int16_t *samples, const size_t *offsets, void *out,
                          size_t out_capacity, size_t *frame_offsets);
int    mfcc_hip_bank_push_dev(mfcc_hip_bank *b, const void *d_samples, const size_t *offsets, void *d_out,
                              size_t out_capacity, size_t *frame_offsets);
/*
 * End of some streams.  streams == NULL: all of them (n is not read); otherwise n distinct indices below
 * the bank's size -- one repeated or out of range is MFCC_HIP_ERROR_INVALID_PARAM and nothing is done.
 * Per listed stream, in the order listed, what mfcc_hip_stream_flush gives, [n_frames][n_cep] to HOST
 * memory: MFCC_HIP_PAD_STREAM one zero-padded tail frame each, MFCC_HIP_PAD_NOTEBOOK nothing.
 * *n_frames_out (may be NULL) = frames written; MFCC_HIP_ERROR_BUFFER_SMALL leaves the bank untouched.
 * The listed streams are in the reset state afterwards, the others are not touched.  Synchronous.
 */
int    mfcc_hip_bank_flush(mfcc_hip_bank *b, const size_t *streams, size_t n, void *out, size_t out_capacity,
                           size_t *n_frames_out);
/* `mfcc_softreset` for the listed streams (as for flush): pending samples dropped, history back to 0.
 * Ordered on the handle's stream behind the pushes before it; does not wait for them. */
int    mfcc_hip_bank_reset(mfcc_hip_bank *b, const size_t *streams, size_t n);

/* ---- online bank: causal CMVN and delta coefficients as state of the bank --------------------------------
 * A float bank on a RAW handle (no normalization, deltas or VAD set on it: MFCC_HIP_ERROR_UNSUPPORTED otherwise, as
 * for a handle that cannot run the float path) with settings of its own, fixed at creation:
 *   normalize         MFCC_HIP_NORMALIZE_MEAN / _MEAN_VAR over the purely causal window of mfcc_hip_set_normalize_window:
 *                     row t of a stream is standardized with rows [max(0, t - normalize_window), t + 1) of that stream.
 *                     In one-shot terms window = normalize_window, min_window = 1, center = 0.
 *                     1 <= normalize_window <= MFCC_HIP_MAX_NORMALIZE_WINDOW, else MFCC_HIP_ERROR_INVALID_PARAM; with
 *                     MFCC_HIP_NORMALIZE_NONE the window is ignored.  NOT offered, because they need the stream's end
 *                     or frames of its future: per-utterance statistics (window 0), the centred window, min_window > 1
 *                     and VAD.
 *   delta_order       0, 1 or 2 with delta_window 1..8 (anything else: MFCC_HIP_ERROR_INVALID_PARAM): the formula of
 *                     mfcc_hip_set_deltas on the normalized rows.  A stream's edges are its own: indices clamp at frame 0
 *                     after create / reset and at the last frame only when the stream is flushed.  Row t is therefore
 *                     returned once row t + lag is known, lag = delta_order * delta_window: every stream holds back up
 *                     to lag finished rows (mfcc_hip_bank_held), which a flush returns.
 * Rows are [s | D | DD], W (1 + delta_order) floats, W = n_cep or n_mel.  Contract: any pushes followed by a flush give,
 * per stream and bit for bit, the rows of the one-shot call on the stream's whole signal by a handle with
 * normalize, normalize_window, min_window 1, center 0, delta_order, delta_window.
 * Device memory besides mfcc_hip_bank_create's: n_streams * (normalize_window + S) * W * 4 bytes of raw rows with
 * normalization (S = normalize_window / 4 clamped to 32..256) and n_streams * 2 * lag * W * 4 bytes of static rows with
 * deltas; MFCC_HIP_ERROR_NO_MEM if that cannot be had.
 * With MFCC_HIP_NORMALIZE_NONE and order 0 the bank is mfcc_hip_bank_create(h, 0, n_streams) bit for bit.
 * It counts as a session of the handle like any bank.  mfcc_hip_bank_push / _push_dev / _reset / _pending / _destroy
 * take it; capacities and MFCC_HIP_ERROR_BUFFER_SMALL count expanded floats, frame_offsets the rows RETURNED; a refused
 * push consumes nothing.  mfcc_hip_bank_push_dev stays asynchronous: held depends on chunk lengths only. */
int    mfcc_hip_bank_create_online(mfcc_hip_handle *h, size_t n_streams, int normalize, int normalize_window,
                                   int delta_order, int delta_window, mfcc_hip_bank **out);
/* The same with PCEN (mfcc_hip_set_pcen) in front of the normalization, as state of the bank: per stream and column
 * the carry C of the tile in progress and its local smoother L, n_streams * 2 * W * 4 bytes; the frame count since
 * create / reset, which the host mirrors, gives the slot of every fresh row.  h must be a RAW handle with
 * MFCC_HIP_OUTPUT_LOGMEL (MFCC_HIP_ERROR_UNSUPPORTED otherwise); a bad block is MFCC_HIP_ERROR_INVALID_PARAM;
 * p = NULL is mfcc_hip_bank_create_online, bit for bit.  The PCEN rows are what enters the normalization's ring and
 * the deltas; with MFCC_HIP_NORMALIZE_NONE and order 0 they go straight to the caller's rows.  A flush's zero-padded
 * tail frame goes through it like any row; reset and flush stay host-only bookkeeping (with a frame count of 0 nothing
 * of C / L is read) and mfcc_hip_bank_push_dev stays asynchronous.  Contract: any pushes followed by a flush give, per
 * stream and bit for bit, the rows of the one-shot call by a handle with the same p (mfcc_hip_set_pcen), normalize,
 * normalize_window, min_window 1, center 0, delta_order, delta_window.                                            */
int    mfcc_hip_bank_create_online_pcen(mfcc_hip_handle *h, size_t n_streams, const mfcc_hip_pcen *p, int normalize,
                                        int normalize_window, int delta_order, int delta_window, mfcc_hip_bank **out);
/* ---- filterbank bank: live lines whose rows are the handle's filterbank rows ----------
 * A float bank whose frame launch is the one of mfcc_hip_fbank_i16_dev: rows of W = n_bands floats, 1 .. 128, of the
 * matrix the handle carries when the bank is created, in that matrix's scale and with its floor (mfcc_hip_set_fbank).
 * Framing, window, pre-emphasis, pad mode and sample format are the handle's.  The handle's own n_mel, output kind,
 * normalization, deltas, PCEN and VAD settings do NOT apply and are not refused, as on every filterbank call.  There is
 * no fixed-point form.
 *   p, normalize, normalize_window, delta_order, delta_window
 *                     exactly those of mfcc_hip_bank_create_online_pcen / mfcc_hip_bank_create_online, with the same
 *                     validation and the same MFCC_HIP_ERROR_INVALID_PARAM cases; p may be NULL.  With p = NULL,
 *                     MFCC_HIP_NORMALIZE_NONE and order 0 it is a plain bank: lockstep pushes write straight into the
 *                     caller's buffer, mixed pushes gather.
 * Contract: any pushes followed by a flush give, per stream and bit for bit, the rows of mfcc_hip_fbank_i16_dev on the
 * stream's whole signal with the handle's pad mode (MFCC_HIP_PAD_STREAM: one zero-padded tail row from the flush;
 * MFCC_HIP_PAD_NOTEBOOK: none), on the generic kernel and on both forms of the fused one -- an element's bits depend on
 * its power row alone.  With online settings: those rows taken column by column through PCEN, the causal sliding
 * normalization (window = normalize_window, min_window 1, center 0) and the delta regression of the direct entries
 * mfcc_hip_pcen_dev, mfcc_hip_normalize_sliding_dev and mfcc_hip_deltas_dev, whose arithmetic is per column and does not
 * depend on the row width (those entries themselves keep their limit of 64 columns).  Rows are [s | D | DD],
 * n_bands (1 + delta_order) floats: mfcc_hip_bank_row_width.
 * Refused before anything is allocated, MFCC_HIP_ERROR_UNSUPPORTED: a handle without a matrix (as the mfcc_hip_fbank_*
 * calls answer); a handle with an input rate (as every bank answers); p on a matrix whose scale is not
 * MFCC_HIP_FBANK_LOG2 (PCEN reads log2 energies).
 * Lifetime: the bank counts as a session of the handle like any bank (MFCC_HIP_ERROR_BUSY of the mfcc_hip_set_* calls,
 * either destroy order).  While at least one filterbank bank of a handle lives, mfcc_hip_set_fbank on that handle answers
 * MFCC_HIP_ERROR_BUSY and leaves the matrix untouched: the bank's width and state are the matrix's.  With only other
 * banks or sessions alive mfcc_hip_set_fbank succeeds as before.
 * mfcc_hip_bank_push / _push_dev / _flush / _flush_ragged / _reset / _pending / _held / _lag / _row_width / _size /
 * _destroy take the bank unchanged; mfcc_hip_bank_push_dev stays asynchronous (no synchronize, no device-to-host copy).
 * Device memory: that of the online banks with W = n_bands. */
int    mfcc_hip_bank_create_filterbank(mfcc_hip_handle *h, size_t n_streams, const mfcc_hip_pcen *p /* may be NULL */,
                                  int normalize, int normalize_window, int delta_order, int delta_window,
                                  mfcc_hip_bank **out);
/* floats per row: W (1 + delta_order); W for a plain bank (int16 elements for a fixed one); 0 for NULL */
size_t mfcc_hip_bank_row_width(const mfcc_hip_bank *b);
/* delta_order * delta_window; 0 for a plain bank or NULL */
int    mfcc_hip_bank_lag(const mfcc_hip_bank *b);
/* held[n_streams]: finished rows every stream has not returned yet (0 <= held <= lag) */
int    mfcc_hip_bank_held(const mfcc_hip_bank *b, size_t *held);
/*
 * mfcc_hip_bank_plan for sessions with a lag, host only (no GPU, no handle).  nf_raw and pending_after as there; then
 *   emitted = max(0, held + nf_raw - lag)   rows are returned and   held_after = held + nf_raw - emitted.
 * frame_offsets[n_streams + 1]: running sum of emitted; pending_after, held_after may be NULL.  With lag = 0 (held all
 * 0) it is mfcc_hip_bank_plan.  lag < 0, held[u] > lag, decreasing offsets or pending[u] >= nfft:
 * MFCC_HIP_ERROR_INVALID_PARAM.
 */
int    mfcc_hip_bank_plan_online(const mfcc_hip_params *p, int lag, const size_t *pending, const size_t *held,
                                 const size_t *offsets, size_t n_streams, size_t *frame_offsets,
                                 size_t *pending_after, size_t *held_after);
/* ... for online banks of a framed handle: the frame length L takes nfft's place, pending[u] < L */
int    mfcc_hip_bank_plan_online_framed(const mfcc_hip_params *p, int frame_length, int lag, const size_t *pending,
                                        const size_t *held, const size_t *offsets, size_t n_streams,
                                        size_t *frame_offsets, size_t *pending_after, size_t *held_after);
/*
 * mfcc_hip_bank_flush with a row count per stream; works on every bank.  streams / n as there.  Per listed stream, in
 * the order listed: with MFCC_HIP_PAD_STREAM the zero-padded tail frame is computed and joins the stream as its last
 * row; then the held rows (and that one) are written with the delta indices clamped at the stream's end, rows
 * frame_offsets[i] .. frame_offsets[i + 1] of out (HOST memory, out_capacity in elements), held + (STREAM ? 1 : 0) of
 * them -- fewer than lag for a short stream.  frame_offsets has n + 1 entries (bank size + 1 with streams == NULL) and
 * is filled also on MFCC_HIP_ERROR_BUFFER_SMALL, which leaves the bank untouched.  The listed streams are in the reset
 * state afterwards.  Synchronous.  mfcc_hip_bank_flush itself answers MFCC_HIP_ERROR_UNSUPPORTED on a bank with
 * lag > 0 (its rows per stream are not uniform) and works on every other.  mfcc_hip_bank_reset also forgets a stream's
 * window, its held rows and its frame count.
 */
int    mfcc_hip_bank_flush_ragged(mfcc_hip_bank *b, const size_t *streams, size_t n, void *out,
                                  size_t out_capacity, size_t *frame_offsets);

/* ---- `.mfcc` -> `.lift` (software/lift.py:28-40): host only, no GPU --------------------------
 * reads raw int16 [frame][n_cep], multiplies column n by 1 + (L/2) sin(pi n / L) in double
 * (lift.py:12-26; L <= 0: unchanged) and writes `astype(np.int16)` of it: truncation toward zero,
 * low 16 bits for values beyond int16 (what NumPy does on x86-64).  *n_frames_out may be NULL. */
int  mfcc_hip_lift_file(const char *mfcc_in, const char *lift_out, int n_cep, double L,
                        size_t *n_frames_out);

/* ---- serial wire format of the FPGA's coefficient stream (host only, no GPU) ---------------
 * mfcc/misc/magic.py:9-41 (MagicInserter: 0xa55a in front of every frame's coefficients),
 * software/serial.c:13-14,89-122 (expect_magic: byte-wise resynchronisation, big endian),
 * software/cepstrum.c:15-71 (cepstrum_get_column: magic, then n_cep big-endian int16).       */

/* bytes mfcc_hip_serial_pack writes for n_frames frames: n_frames * 2 * (n_cep + 1) */
size_t mfcc_hip_serial_packed_size(size_t n_frames, int n_cep);

/* cep [n_frames][n_cep] int16 (what process_fixed_i16 returns) -> the byte stream the FPGA's
 * UART carries: per frame 0xa5 0x5a, then n_cep coefficients high byte first.             */
int  mfcc_hip_serial_pack(const int16_t *cep, size_t n_frames, int n_cep, uint8_t *out, size_t out_capacity);

/* The receiver of cepstrum_get_column, on a buffer instead of a file descriptor: scan for 0xa5
 * followed by 0x5a exactly like expect_magic (a 0xa5 not followed by 0x5a drops both bytes), then
 * take n_cep big-endian int16; repeat.  Stops at max_frames or when the buffer cannot hold another
 * whole column.  *n_frames_out = columns decoded, *consumed_out = bytes of `bytes` used up.   */
int  mfcc_hip_serial_unpack(const uint8_t *bytes, size_t n_bytes, int n_cep, int16_t *cep, size_t max_frames,
                            size_t *n_frames_out, size_t *consumed_out);

/* cepstrum_eval_power (software/cepstrum.c:161-183): `window` is the circular buffer of
 * n_frames x n_cep int16, `head` the element index of its oldest entry (0 for a linear window).
 * Sums the squares of the elements head + i, i = size/3, size/3 + n_cep, ... < 2 size/3 (size =
 * n_frames * n_cep; the first coefficient of the middle third of the frames when size/3 is a
 * multiple of n_cep, as in the reference's 16 x 93 window).  *power_out gets the sum (64-bit; the
 * reference accumulates in a 32-bit int); returns 1 if it reaches the reference's threshold 1e8,
 * 0 if not, negative on bad arguments.                                                       */
int  mfcc_hip_eval_power(const int16_t *window, int n_cep, int n_frames, size_t head, long long *power_out);
/* The same with the reference's own accumulator, a 32-bit `int`: *power_out gets the low 32 bits of the sum read as a
 * signed number, and the return value compares THAT with 1e8.  The C standard leaves signed overflow undefined; this is
 * what the reference's loop gives when built with gcc on x86-64 (two's-complement wrap), and what a receiver built that
 * way decides: two coefficients of -32768 sum to 2^31 and do NOT pass, four of them sum to 0.                    */
int  mfcc_hip_eval_power32(const int16_t *window, int n_cep, int n_frames, size_t head, int32_t *power_out);

/* ---- the power gate and window extraction on fixed-point rows (DESIGN.md sections 4.10, 6c-quater) ---------------------
 * The receiver (software/cepstrum.c:93-183) keeps the last n_frames columns of n_cep int16 coefficients, sums c0^2 over
 * the middle third of that window and lets the window through when the sum reaches POWER_THRESHOLD.  Here: the same
 * decision for EVERY window of int16 rows in HBM, and the extraction of the windows a mask keeps.
 * Rows are int16 [row][n_cep], n_cep 1..64 (what the fixed-point entry points and a fixed bank write).  A segment is one
 * channel or one utterance of T rows.  With n_frames 1..MFCC_HIP_MAX_GATE_WINDOW, stride 1..MFCC_HIP_MAX_GATE_WINDOW and
 * threshold >= 0 (MFCC_HIP_POWER_THRESHOLD is the reference's):
 *     n_win    = T >= n_frames ? (T - n_frames) / stride + 1 : 0      window j = rows [j stride, j stride + n_frames)
 *     size     = n_frames n_cep,  first = size / 3,  last = 2 size / 3
 *     power_j  = sum of x^2 over the elements i = first, first + n_cep, ... < last of window j taken as a linear array
 *                (head = 0): with K = ceil((last - first) / n_cep) (0 when last == first), f0 = first / n_cep and
 *                c0 = first % n_cep this is column c0 of frames f0 .. f0 + K - 1 of the window.  c0 is 0 when size / 3
 *                is a multiple of n_cep (the reference's 16 x 93) and is NOT 0 in general (5 x 4: c0 = 1, f0 = 1, K = 2)
 *     gate_j     = power_j >= threshold                                   power exact in int64: at most 1366 * 2^30
 *     gate_ref_j = (long long)(int32_t)(uint32_t)power_j >= threshold     what the reference's 32-bit `int power` holds on
 *                two's-complement hardware.  The C standard leaves that overflow undefined; this is what gcc on x86-64
 *                produces (mfcc_hip_eval_power32).  On loud speech the two gates differ.
 * Everything is integer arithmetic: every entry point, any tiling, any run gives the same bits.  No atomics.
 * The ABI version and the parameter block are unchanged.                                                         */
#define MFCC_HIP_MAX_GATE_WINDOW 4096
#define MFCC_HIP_POWER_THRESHOLD 100000000LL
/* Host only (no GPU, no handle): win_offsets[n_segs + 1] = running sum of n_win over the segments seg_offsets[k] ..
 * seg_offsets[k + 1] (rows; n_segs + 1 entries, must not decrease) -- the global window index every output below is
 * indexed by.  Window counts depend on lengths only.  Bad ranges, NULL arrays, decreasing offsets:
 * MFCC_HIP_ERROR_INVALID_PARAM.                                                                                */
int  mfcc_hip_gate_count(int n_frames, int stride, const size_t *seg_offsets, size_t n_segs, size_t *win_offsets);
/* The decision.  d_rows int16 [seg_offsets[n_segs]][n_cep] (2-byte aligned; rows before seg_offsets[0] are not read);
 * d_power int64 (8-byte aligned), d_gate and d_gate_ref uint8 0 / 1, one entry per window at the global window index of
 * mfcc_hip_gate_count; entries beyond the last window are untouched.  Any of the three may be NULL, not all of them.
 * Inputs and outputs (or two outputs) that overlap, a parameter outside its range, decreasing offsets:
 * MFCC_HIP_ERROR_INVALID_PARAM.  Asynchronous on the handle's stream; n_segs = 0 or no window at all is a no-op that
 * does not look at the data pointers (all of them may then be NULL). */
int  mfcc_hip_gate_dev(mfcc_hip_handle *h, const void *d_rows, int n_cep, const size_t *seg_offsets, size_t n_segs,
                       int n_frames, int stride, long long threshold, void *d_power, void *d_gate, void *d_gate_ref);
/* The selection: the windows whose d_mask byte (one per window, global window index; the gate bytes, the reference bytes
 * or anything computed from d_power) is not 0, copied whole to d_out, int16 [n_sel][n_frames][n_cep] (2-byte aligned),
 * packed in window order; overlapping windows are each copied in full.  d_starts (may be NULL; 8-byte aligned) int64
 * [n_sel]: the first row of every kept window as an index into d_rows.  out_offsets (HOST, n_segs + 1 entries): the
 * range of every segment in the packed result.  The count depends on the data: the call counts and scans, SYNCHRONIZES
 * the handle's stream and reads the total; if out_capacity_windows is below it, MFCC_HIP_ERROR_BUFFER_SMALL with
 * out_offsets filled and nothing written to d_out or d_starts -- size them from out_offsets[n_segs] and call again (a
 * first call with capacity 0 and d_out NULL is the way to ask).  Otherwise the copy is enqueued; it is asynchronous.
 * What is written must not overlap what is read: MFCC_HIP_ERROR_INVALID_PARAM, nothing written.                 */
int  mfcc_hip_gate_windows_dev(mfcc_hip_handle *h, const void *d_rows, int n_cep, const size_t *seg_offsets, size_t n_segs,
                               int n_frames, int stride, const void *d_mask, void *d_out, void *d_starts,
                               size_t out_capacity_windows, size_t *out_offsets);

/* ---- gate tracker: the receiver's circular window for N live lines ------------------------
 * The batched form of cepstrum_refill_window + cepstrum_eval_power: n_lines independent windows whose state lives on
 * the device, per line a ring of the last D = n_frames + stride - 1 rows (row t of the line in slot t mod D), and on the
 * host the frames every line has seen since create / reset.  A push takes exactly what mfcc_hip_bank_push_dev of a fixed
 * bank leaves behind -- the device rows and the host frame_offsets -- so the two chain on one stream with no synchronize
 * between them.  Window j of a line starts at the line's absolute frame j stride counted from create / reset.  Contract:
 * any chunking of a line's rows gives the same windows with the same bytes, and they are the windows of
 * mfcc_hip_gate_dev / mfcc_hip_gate_windows_dev on the line's whole row sequence as one segment.
 * A tracker counts as a session of its handle (lifetime rule at mfcc_hip_destroy, MFCC_HIP_ERROR_BUSY of the
 * mfcc_hip_set_* calls); like the handle it is not thread-safe.                                                  */
typedef struct mfcc_hip_gate mfcc_hip_gate;
/* n_lines >= 1, the other parameters in the ranges above; every line starts with no frame seen */
int    mfcc_hip_gate_create(mfcc_hip_handle *h, size_t n_lines, int n_cep, int n_frames, int stride, long long threshold,
                            mfcc_hip_gate **out);
/* frees the ring (waits for the tracker's work first); frees the handle too if that was already given to
 * mfcc_hip_destroy and this was its last session */
void   mfcc_hip_gate_destroy(mfcc_hip_gate *g);
/* seen[n_lines]: frames every line has received since create / reset (a host mirror, no device traffic) */
int    mfcc_hip_gate_seen(const mfcc_hip_gate *g, size_t *seen);
/* The plan of a push, host only (no GPU, no handle).  Line u has seen[u] = s frames and receives
 * nf = frame_offsets[u + 1] - frame_offsets[u] more; it completes the windows j with s <= j stride + n_frames - 1 < s + nf.
 * win_offsets[n_lines + 1]: the running sum of their counts; seen_after[n_lines] (may be NULL) = s + nf. */
int    mfcc_hip_gate_plan(int n_frames, int stride, const size_t *seen, const size_t *frame_offsets, size_t n_lines,
                          size_t *win_offsets, size_t *seen_after);
/* Feed every line its new rows: line u gets rows frame_offsets[u] .. frame_offsets[u + 1] of d_rows (int16 [..][n_cep],
 * 2-byte aligned; n_lines + 1 offsets, not decreasing; a range may be empty).  Per completed window, in line order then
 * window order, entries win_offsets[u] .. win_offsets[u + 1] of d_power / d_gate / d_gate_ref as for mfcc_hip_gate_dev
 * (any may be NULL; not all when a window completes).  capacity_windows below the total: MFCC_HIP_ERROR_BUFFER_SMALL;
 * that and MFCC_HIP_ERROR_INVALID_PARAM fill win_offsets where they can and consume NOTHING.  Asynchronous on the
 * handle's stream, no synchronize and no device-to-host copy; d_rows must stay valid until the stream has run it. */
int    mfcc_hip_gate_push_dev(mfcc_hip_gate *g, const void *d_rows, const size_t *frame_offsets, void *d_power, void *d_gate,
                              void *d_gate_ref, size_t capacity_windows, size_t *win_offsets);
/* The listed lines (lines == NULL: all, n is not read; otherwise n distinct indices below n_lines, else
 * MFCC_HIP_ERROR_INVALID_PARAM and nothing is done) start again at frame 0.  Only the frame counts are zeroed: a line
 * that has seen nothing reads nothing of its ring.  Ordered on the stream behind the pushes before it; does not wait. */
int    mfcc_hip_gate_reset(mfcc_hip_gate *g, const size_t *lines, size_t n);
/* For each listed line the rows of its last completed window, d_out int16 [n][n_frames][n_cep] in the order listed.
 * A listed line that has completed no window since create / reset, or a repeated or out-of-range index:
 * MFCC_HIP_ERROR_INVALID_PARAM and nothing is written.  Asynchronous on the handle's stream. */
int    mfcc_hip_gate_window_dev(mfcc_hip_gate *g, const size_t *lines, size_t n, void *d_out);

#ifdef __cplusplus
}
#endif
#endif /* MFCC_HIP_H */
