// libmfcc_hip.so -- C ABI (include/mfcc_hip.h) over the gfx950 MFCC kernels.
//
// Host side: parameter validation, table building (tables.hpp), device buffers, launches.
// There is NO CPU compute path in this library: without a HIP device mfcc_hip_create fails
// with MFCC_HIP_ERROR_NOT_FOUND (the host-only helpers -- frame counts, table dumps, error
// strings -- keep working so the CPU test-suite can check the host logic).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mfcc_hip.h"
#include "bank_plan.hpp"
#include "batch_plan.hpp"
#include "seg_plan.hpp"
#include "kernels_generic.hpp"
#include "kernel_fixed512.hpp"
#include "kernel_fused1024.hpp"
#include "kernel_fused1024_f32.hpp"
#include "kernel_fused1024_w12.hpp"
#include "kernel_fused512.hpp"
#include "kernel_fused512_w12.hpp"
#include "kernel_fused512_h160.hpp"
#include "kernel_fused512_h160_mb.hpp"
#include "kernel_normalize.hpp"
#include "kernel_deltas.hpp"
#include "kernel_normalize_sliding.hpp"
#include "kernel_pcen.hpp"
#include "kernel_vad.hpp"
#include "kernel_stream_bank.hpp"
#include "kernel_stream_bank_online.hpp"
#include "kernel_gate.hpp"
#include "kernel_decode.hpp"
#include "kernel_resample.hpp"
#include "kernel_center.hpp"
#include "kernel_spectrum.hpp"
#include "kernel_fbank.hpp"
#include "post_wide.hpp"
#include "tables.hpp"

namespace {

using namespace mfcc_tables;

struct Resolved {
    int nfft, hop, n_mel, n_cep, sample_rate, pad_mode;
    double power_scale, lifter;
    int device, float_impl;
    int output;                // enum mfcc_hip_output
    int frame_len;             // samples of a frame (hop <= frame_len <= nfft); the window's length.  nfft: a plain handle
    int mel_kind;              // enum mfcc_hip_mel_kind (mfcc_hip_create_banked); NOTEBOOK: the reference's bank
    double mel_lo, mel_hi;     // HTK: the band edges in Hz, mel_hi effective (never 0); NOTEBOOK: both 0
    Front front;               // window function and pre-emphasis pair (mfcc_hip_create_fronted); default: the reference's
};

// width of a row of the handle's own output: n_mel log-mel values or n_cep coefficients
inline size_t row_width(const Resolved &r) { return size_t(r.output == MFCC_HIP_OUTPUT_LOGMEL ? r.n_mel : r.n_cep); }
inline bool is_logmel(const Resolved &r) { return r.output == MFCC_HIP_OUTPUT_LOGMEL; }

// The passes behind the float kernels as a handle is set up for them (mfcc_hip_set_normalize, _normalize_window, _deltas,
// _pcen, _vad); default-constructed: none of them
struct Post {
    int norm = MFCC_HIP_NORMALIZE_NONE;
    int norm_window = 0;       // 0: the per-segment form; else the sliding one, with the minimum window of its causal form
    int norm_min_window = 1;   // and centered / causal
    int norm_center = 1;
    int delta_order = 0;       // 0 (off), 1 or 2
    int delta_window = 2;
    bool pcen_on = false;
    mfcc_pcen::Prm pcen{};     // the parameters as the kernels take them
    int vad_mode = MFCC_HIP_VAD_OFF;
    int vad_column = 0;
    int vad_context = 0;
    float vad_threshold = 5.0f, vad_scale = 0.5f, vad_proportion = 0.6f;
};
const Post kNoPost{};

// What the sample pointer in hand holds: the format, the rate (0: the handle's own) and whether the signal is still to be
// centred (enum mfcc_hip_center).  It travels with the pointer as far as the input stage of its route (dense_input,
// ragged_input); behind that stage every pointer is int16 at the handle's own rate, padded where it had to be
struct Samples {
    int fmt, rate, center;
};

// What a call computes.  Every entry point builds one (call_of) and passes it down; the routes read it, never the handle's
// settings
enum class Kind { kFeatures, kSpectrum, kFbank };     // the handle's own output, power-spectrum rows, filterbank rows
struct Call {
    Kind kind;
    bool fixed;
    size_t width;              // floats (fixed: int16) of a row as the kernel writes it
    size_t out_width;          // ... and as the call returns it: width times 1 + the delta order
    const Post &post;          // the handle's for a float features call, its fb_post for a filterbank call, else kNoPost
};

// The kernel a handle's float calls run; build_tables decides it when the handle is made.
enum class FloatKernel {
    kGeneric,
    kFused512W12,        // twelve waves (kernel_fused512_w12.hpp): the default at 512/170
    kFused512,           // four waves (kernel_fused512.hpp)
    kFused512H160,       // a framed handle at 512 / hop 160 (kernel_fused512_h160.hpp)
    kFused512H160Mb,     // an HTK-bank handle at 512 / hop 160 (kernel_fused512_h160_mb.hpp)
    kFused1024W12Bf,     // twelve waves, bf16-split contraction (kernel_fused1024_w12.hpp): the default at 1024/341
    kFused1024W12F32,    // twelve waves, fp32 contraction
    kFused1024Bf,        // eight waves, bf16-split contraction (kernel_fused1024.hpp)
    kFused1024F32,       // eight waves, fp32 contraction (kernel_fused1024_f32.hpp)
};
// ... and its fixed-point calls; kNone: every fixed entry point answers UNSUPPORTED
enum class FixedKernel { kNone, kGeneric, kFixed512 };

inline bool is_fused512(FloatKernel k) {
    return k == FloatKernel::kFused512W12 || k == FloatKernel::kFused512 || k == FloatKernel::kFused512H160 ||
           k == FloatKernel::kFused512H160Mb;
}

int resolve(const mfcc_hip_params *p, Resolved &r) {
    if (!p) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (p->struct_size != sizeof(mfcc_hip_params)) return MFCC_HIP_ERROR_INVALID_PARAM;
    for (int v : p->reserved)
        if (v != 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    r.nfft = p->nfft;
    r.hop = p->hop == 0 ? p->nfft / 3 : p->hop;
    r.n_mel = p->n_mel;
    r.n_cep = p->n_cep;
    r.sample_rate = p->sample_rate;
    r.pad_mode = p->pad_mode;
    r.power_scale = p->power_scale == 0.0f ? double(p->nfft) : double(p->power_scale);
    r.lifter = double(p->lifter);
    r.device = p->device;
    r.float_impl = p->float_impl;
    r.output = p->output;
    r.frame_len = p->nfft;
    r.mel_kind = MFCC_HIP_MEL_NOTEBOOK;
    r.mel_lo = r.mel_hi = 0.0;
    r.front = Front{};
    if (!is_pow2(r.nfft) || r.nfft < 64 || r.nfft > 1024) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.hop < 1 || r.hop > r.nfft) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.n_mel < 1 || r.n_mel > mfcc_k::kMaxMel) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.n_cep < 1 || r.n_cep > r.n_mel) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.sample_rate < 1) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.pad_mode != MFCC_HIP_PAD_NOTEBOOK && r.pad_mode != MFCC_HIP_PAD_STREAM)
        return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!(r.power_scale > 0.0) || r.lifter < 0.0) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.float_impl < MFCC_HIP_IMPL_AUTO || r.float_impl > MFCC_HIP_IMPL_FUSED512)
        return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.output != MFCC_HIP_OUTPUT_CEPSTRA && r.output != MFCC_HIP_OUTPUT_LOGMEL) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (r.output == MFCC_HIP_OUTPUT_LOGMEL && r.lifter != 0.0) return MFCC_HIP_ERROR_INVALID_PARAM;   // weights cepstra
    return MFCC_HIP_SUCCESS;
}

// ... and a frame length (mfcc_hip_create_framed): 0 and nfft mean the plain handle
int resolve_framed(const mfcc_hip_params *p, int frame_length, Resolved &r) {
    if (frame_length < 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    const int rc = resolve(p, r);
    if (rc) return rc;
    if (frame_length == 0) return MFCC_HIP_SUCCESS;
    if (frame_length < 2 || frame_length > r.nfft || frame_length < r.hop) return MFCC_HIP_ERROR_INVALID_PARAM;
    r.frame_len = frame_length;
    return MFCC_HIP_SUCCESS;
}

inline bool is_framed(const Resolved &r) { return r.frame_len != r.nfft; }

// ... and a mel bank (mfcc_hip_create_banked): NULL and NOTEBOOK without edges mean the handle above
int resolve_banked(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank, Resolved &r) {
    const int rc = resolve_framed(p, frame_length, r);
    if (rc || !bank) return rc;
    if (bank->struct_size != sizeof(mfcc_hip_mel_bank)) return MFCC_HIP_ERROR_INVALID_PARAM;
    for (int v : bank->reserved)
        if (v != 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    const double lo = double(bank->low_hz), hi = double(bank->high_hz);
    if (bank->kind == MFCC_HIP_MEL_NOTEBOOK) return (lo == 0.0 && hi == 0.0) ? MFCC_HIP_SUCCESS : MFCC_HIP_ERROR_INVALID_PARAM;
    if (bank->kind != MFCC_HIP_MEL_HTK) return MFCC_HIP_ERROR_INVALID_PARAM;
    const double nyq = double(r.sample_rate) / 2.0, top = hi == 0.0 ? nyq : hi;
    if (!(lo >= 0.0) || !(lo < top) || !(top <= nyq)) return MFCC_HIP_ERROR_INVALID_PARAM;       // NaN fails every test
    r.mel_kind = MFCC_HIP_MEL_HTK;
    r.mel_lo = lo;
    r.mel_hi = top;
    return MFCC_HIP_SUCCESS;
}

inline bool is_htk(const Resolved &r) { return r.mel_kind == MFCC_HIP_MEL_HTK; }

// ... and a front (mfcc_hip_create_fronted): NULL means the handle above.  The pair is reduced by its gcd, so the default
// front written out in any form IS the default front
int resolve_fronted(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank, const mfcc_hip_front *front,
                    Resolved &r) {
    const int rc = resolve_banked(p, frame_length, bank, r);
    if (rc || !front) return rc;
    if (front->struct_size != sizeof(mfcc_hip_front)) return MFCC_HIP_ERROR_INVALID_PARAM;
    for (int v : front->reserved)
        if (v != 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (front->window < 0 || front->window >= kFrontWindows) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (front->symmetric != 0 && front->symmetric != 1) return MFCC_HIP_ERROR_INVALID_PARAM;
    int num = front->preemph_num, den = front->preemph_den;
    if (!reduce_preemph(num, den)) return MFCC_HIP_ERROR_INVALID_PARAM;
    r.front.window = front->window;
    r.front.symmetric = front->symmetric;
    r.front.num = num;
    r.front.den = den;
    return MFCC_HIP_SUCCESS;
}

inline bool is_fronted(const Resolved &r) { return !front_is_default(r.front); }

// the mel matrix of a handle, [n_mel][nfft / 2 + 1], before the power scale: every float table is built from this
std::vector<double> handle_mel(const Resolved &r) {
    if (is_htk(r)) return mel_dense_htk(r.nfft, r.n_mel, double(r.sample_rate), r.mel_lo, r.mel_hi);
    return mel_dense(r.nfft, r.n_mel, double(r.sample_rate));
}

inline mfcc_batch::Framing framing(const Resolved &r) {
    return {size_t(r.frame_len), size_t(r.hop), r.pad_mode != MFCC_HIP_PAD_NOTEBOOK};
}

size_t count_frames(const Resolved &r, size_t n) { return mfcc_batch::frames_of(framing(r), n); }

// the float window of a handle: its front's window function (periodic Hamming by default) over the frame, zeros up to
// nfft (the frame is zero-padded at the end).  Every float table is built from this vector and the front's pair
std::vector<double> frame_window(const Resolved &r) {
    std::vector<double> w = front_window(r.front, r.frame_len);
    w.resize(size_t(r.nfft), 0.0);
    return w;
}

bool fixed_supported(const Resolved &r) {
    // RTL constraints: FFT sizes are powers of two (mfcc/misc/fft.py:351-353) for both the
    // nfft-point FFT and the (4 * nfilters)-point DCT FFT; hop = nfft // 3 (mfcc/core/mfcc.py:43); the window is the
    // RTL's ROM curve over nfft samples: no frame length below nfft and no other front; its filterbank is the notebook's:
    // no HTK bank
    if (is_framed(r) || is_htk(r) || is_fronted(r)) return false;
    if (!(is_pow2(4 * r.n_mel) && 4 * r.n_mel <= r.nfft && r.n_mel >= 4 && r.hop == r.nfft / 3 && r.nfft >= 64))
        return false;
    // filter points too dense for the streaming filterbank's ramp logic (filterbank.py:22-34, 88-142): the RTL then
    // emits fewer than n_mel values per frame and the frame structure falls apart -- not a configuration to reproduce
    return fx_mel(r.nfft, r.n_mel, double(r.sample_rate)).n_out == r.n_mel;
}

struct SparseRows {
    std::vector<int> start, count, off;
};

template <typename T>
SparseRows pack_rows(const std::vector<T> &dense, int rows, int cols, std::vector<T> &packed) {
    SparseRows s;
    packed.clear();
    for (int r = 0; r < rows; ++r) {
        int lo = cols, hi = -1;
        for (int k = 0; k < cols; ++k)
            if (dense[size_t(r) * cols + k] != T(0)) {
                if (k < lo) lo = k;
                hi = k;
            }
        int cnt = hi >= lo ? hi - lo + 1 : 0;
        s.start.push_back(cnt ? lo : 0);
        s.count.push_back(cnt);
        s.off.push_back(int(packed.size()));
        for (int k = 0; k < cnt; ++k) packed.push_back(dense[size_t(r) * cols + lo + k]);
    }
    return s;
}

}  // namespace

// a device buffer that only grows (ensure)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct mfcc_hip_handle {
    Resolved r;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int last_hip = 0;
    int n_cu = 0;
    // which kernel a call runs: both decided once, at the end of build_tables, and only read afterwards (launch,
    // mfcc_hip_kernel_name, the ragged entry points)
    FloatKernel float_kernel = FloatKernel::kGeneric;
    FixedKernel fixed_kernel = FixedKernel::kNone;
    bool fused_dense = false;     // h->fu holds the all-pairs schedule: the banded MFMA list does not fit this sample rate
    // device tables (one arena)
    void *arena = nullptr;
    mfcc_k::FloatTables ft{};
    mfcc_k::FixedTables xt{};
    mfcc_fused::W4Tables fu{};             // the twelve-wave kernel takes its base
    mfcc_fused160mb::Tables fmb{};
    mfcc_fixed512::Tables x5{};
    // the power-spectrum output (mfcc_hip_spectrum_*): the kernel of every such call (spectrum_plan.hpp: choose) and the
    // tables of the fused one
    mfcc_spec::Kernel spec_kernel = mfcc_spec::Kernel::kGeneric;
    mfcc_spec::FusedTables sf{};
    // the filterbank output (mfcc_hip_set_fbank, mfcc_hip_fbank_*): the kernel of every such call (fbank_plan.hpp:
    // choose; the fused one reads sf too), the matrix's tables in a device allocation of their own (fb_dev; NULL: no
    // matrix) and the scale.  fb_used: a call has read the tables, so a new matrix synchronizes the device first
    mfcc_fbank::Kernel fb_kernel = mfcc_fbank::Kernel::kGeneric;
    void *fb_dev = nullptr;
    mfcc_fbank::Tables fb{};
    int fb_scale = MFCC_HIP_FBANK_ENERGY;
    bool fb_used = false;
    // the passes behind the one-shot filterbank calls (mfcc_hip_set_filterbank_post): the matrix's, so mfcc_hip_set_fbank
    // resets them; never a VAD.  `post` below does not apply to a filterbank call, and this does not apply to any other
    Post fb_post;
    // the 1024 forms: one of the two is bound, the one float_kernel names
    mfcc_fused1024::Tables f1k{};          // bf16-split contraction, set lists for every rate (kernel_fused1024.hpp)
    mfcc_fused1024_f32::Tables f1k_f32{};  // fp32 contraction, one MFMA list per rate (kernel_fused1024_f32.hpp)
    // descriptor tables of the ragged calls live in pinned host memory, two buffers used in turn: the H2D copy of
    // an asynchronous call reads buffer i while the next call fills buffer 1 - i; the call after that waits for the
    // event recorded behind buffer i's copy before it overwrites it
    struct PinnedDesc {
        long long *p = nullptr;
        size_t cap = 0;
        hipEvent_t copied = nullptr;
        bool in_flight = false;
    } desc[2];
    int desc_next = 0;
    // scratch for the host-buffer and ragged entry points.  It is reused by calls that may run on different
    // streams (mfcc_hip_set_stream): scratch_done is recorded behind every use and the next use on ANOTHER stream
    // waits for it on the device (an event outlives the stream it was recorded on)
    DevBuf d_in, d_out;
    hipEvent_t scratch_done = nullptr;
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;
    // host-buffer pipeline (process_host): copy streams of their own, three chunks in flight
    static constexpr int kPipe = 3;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[kPipe] = {}, ev_k[kPipe] = {}, ev_out[kPipe] = {};
    DevBuf p_in[kPipe], p_out[kPipe];
    // streaming sessions opened on this handle that are still alive.  mfcc_hip_destroy with live sessions only marks
    // the handle; the last mfcc_hip_stream_destroy then tears it down (include/mfcc_hip.h: lifetime)
    int n_sessions = 0;
    bool destroy_pending = false;
    // ... and the filterbank banks among them (mfcc_hip_bank_create_filterbank): their width and state are the matrix's,
    // so mfcc_hip_set_fbank answers BUSY while one lives
    int n_fbank_banks = 0;
    // the passes behind the float kernels: their settings, written by the mfcc_hip_set_* functions and nowhere else
    Post post;
    // per-segment normalization: the stats / coefficient / tile-table scratch and, for host-buffer calls whose chunks cut
    // a channel, the whole result on the device (run_host_pipeline)
    DevBuf d_norm, d_full;
    // delta coefficients: the static rows the delta pass reads (d_stat) and its tile table (d_dtab)
    DevBuf d_stat, d_dtab;
    // sliding-window normalization: the raw rows the sliding pass reads (d_slide: it cannot run in place) and its tile
    // table (d_stab)
    DevBuf d_slide, d_stab;
    // energy VAD: the decision's scratch (d_vad: tile partials, thresholds, tile table), the mask (d_voiced), the
    // selection's scratch (d_sel: tile counts, prefixes, segment offsets, tile table) and the final rows of a SELECT call
    // before the gather moves them to the caller (d_final)
    DevBuf d_vad, d_voiced, d_sel, d_final;
    // PCEN: the pass's scratch (d_pcen: tile ends, carries, tile table)
    DevBuf d_pcen;
    // sample format (mfcc_hip_set_sample_format): what every sample pointer holds; the decoded int16 samples of a call
    // (d_dec) and the raw bytes of a session's push on their way to the decode (d_raw)
    int sample_fmt = MFCC_HIP_SAMPLE_S16;
    DevBuf d_dec, d_raw;
    // sample rates (mfcc_hip_resample_dev, mfcc_hip_set_input_rate): the tap table of the last ratio on the device
    // (d_rs_tab; rs_in / rs_out name the ratio, 0: none yet), the rate every sample pointer is read at (0: the handle's
    // own, no pass) and the resampled int16 samples of a call (d_rs)
    int rs_in = 0, rs_out = 0;
    mfcc_rs::Geometry rs_geom;
    DevBuf d_rs_tab, d_rs;
    int input_rate = 0;
    // centring (mfcc_hip_set_center): the mode every one-shot float call frames by, and the padded int16 samples of a call
    // (d_ctr; behind them the records of a ragged one)
    int center = MFCC_HIP_CENTER_OFF;
    DevBuf d_ctr;
};

namespace {

#define HIP_TRY(h, expr)                         \
    do {                                         \
        hipError_t e__ = (expr);                 \
        if (e__ != hipSuccess) {                 \
            (h)->last_hip = int(e__);            \
            return e__ == hipErrorOutOfMemory ? MFCC_HIP_ERROR_NO_MEM : MFCC_HIP_ERROR_OTHER; \
        }                                        \
    } while (0)

// Makes h's device current for the scope and puts the caller's device back afterwards (a process that drives
// several GPUs -- torch included -- must not find its current device changed by a library call).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// order a new use of the handle's scratch buffers behind the previous one when the stream has changed
int scratch_acquire(mfcc_hip_handle *h) {
    if (h->scratch_used && h->scratch_stream != h->stream)
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->scratch_done, 0));
    return MFCC_HIP_SUCCESS;
}

int scratch_release(mfcc_hip_handle *h) {
    HIP_TRY(h, hipEventRecord(h->scratch_done, h->stream));
    h->scratch_stream = h->stream;
    h->scratch_used = true;
    return MFCC_HIP_SUCCESS;
}

// a pinned descriptor buffer of at least n entries that no copy in flight still reads
int desc_acquire(mfcc_hip_handle *h, size_t n, mfcc_hip_handle::PinnedDesc **out) {
    mfcc_hip_handle::PinnedDesc &d = h->desc[h->desc_next];
    h->desc_next ^= 1;
    if (d.in_flight) {
        HIP_TRY(h, hipEventSynchronize(d.copied));
        d.in_flight = false;
    }
    if (d.cap < n) {
        if (d.p) HIP_TRY(h, hipHostFree(d.p));
        d.p = nullptr;
        d.cap = 0;
        const size_t want = n + n / 2 + 64;
        HIP_TRY(h, hipHostMalloc(reinterpret_cast<void **>(&d.p), want * sizeof(long long), hipHostMallocDefault));
        d.cap = want;
    }
    if (!d.copied) HIP_TRY(h, hipEventCreateWithFlags(&d.copied, hipEventDisableTiming));
    *out = &d;
    return MFCC_HIP_SUCCESS;
}

// n_ll descriptors of pd on their way to d_dst, on the handle's stream; the pinned buffer is free again once the event
// recorded behind the copy has passed
int desc_upload(mfcc_hip_handle *h, mfcc_hip_handle::PinnedDesc *pd, size_t n_ll, void *d_dst) {
    HIP_TRY(h, hipMemcpyAsync(d_dst, pd->p, n_ll * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(pd->copied, h->stream));
    pd->in_flight = true;
    return MFCC_HIP_SUCCESS;
}

int ensure(mfcc_hip_handle *h, DevBuf &b, size_t want) {
    if (b.bytes >= want && b.p) return MFCC_HIP_SUCCESS;
    if (b.p) {
        HIP_TRY(h, hipFree(b.p));
        b = DevBuf{};
    }
    const size_t sz = want + want / 4 + 4096;
    HIP_TRY(h, hipMalloc(&b.p, sz));
    b.bytes = sz;
    return MFCC_HIP_SUCCESS;
}

// The scratch buffer b of the handle grown to `want` bytes (0: left as it is) and taken (scratch_acquire), the
// descriptors of pd (none without one) on their way to byte `at` of it
int desc_stage(mfcc_hip_handle *h, DevBuf &b, size_t want, mfcc_hip_handle::PinnedDesc *pd, size_t n_ll, size_t at = 0) {
    int rc;
    if (want && (rc = ensure(h, b, want))) return rc;
    if ((rc = scratch_acquire(h))) return rc;
    return pd ? desc_upload(h, pd, n_ll, static_cast<char *>(b.p) + at) : MFCC_HIP_SUCCESS;
}

// ---- sample formats (kernel_decode.hpp): one streaming pass in front of the kernels turns the
// samples of a call into int16 in h->d_dec, and the call goes on from there as it does on int16 input
inline bool decodes(int fmt) { return fmt != MFCC_HIP_SAMPLE_S16; }
inline size_t sample_bytes(int fmt) { return mfcc_decode::sample_size(fmt); }
inline bool sample_aligned(int fmt, const void *p) { return (reinterpret_cast<uintptr_t>(p) & (sample_bytes(fmt) - 1)) == 0; }
// sample i behind p
inline const void *sample_at(int fmt, const void *p, size_t i) { return static_cast<const char *>(p) + i * sample_bytes(fmt); }

// rows of n samples in format fmt (row r at sample r * in_stride of d_in) -> int16 rows of out_stride samples at d_out,
// on the handle's stream.  More than one row: out_stride is a multiple of 8, or the rows lie back to back
int decode_rows(mfcc_hip_handle *h, int fmt, const void *d_in, size_t n, size_t rows, size_t in_stride, int16_t *d_out,
                size_t out_stride) {
    if (!n || !rows) return MFCC_HIP_SUCCESS;
    if (rows > 1 && in_stride == n && out_stride == n) {         // back to back on both sides: one row
        n *= rows;
        rows = 1;
    }
    if (!mfcc_decode::launch(fmt, d_in, d_out, n, rows, in_stride, out_stride, h->n_cu, h->stream))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

// ... into the handle's scratch area, grown and taken (the caller releases it behind the kernels that read it): rows
// back to back where the input's are, else every row rounded up to 8 samples
int decode_to_scratch(mfcc_hip_handle *h, int fmt, const void *d_in, size_t n, size_t rows, size_t in_stride,
                      const int16_t **out, size_t *out_stride) {
    const size_t stride = rows <= 1 || in_stride == n ? n : (n + 7) & ~size_t(7);
    int rc = ensure(h, h->d_dec, rows * stride * sizeof(int16_t) + 64);
    if (rc || (rc = scratch_acquire(h))) return rc;
    *out = static_cast<const int16_t *>(h->d_dec.p);
    *out_stride = stride;
    return decode_rows(h, fmt, d_in, n, rows, rows <= 1 ? n : in_stride, static_cast<int16_t *>(h->d_dec.p), stride);
}

// ---- sample rates (include/mfcc_hip.h: "sample rates"; resample_plan.hpp, kernel_resample.hpp)
int rs_geometry(int in_rate, int out_rate, mfcc_rs::Geometry &g) {
    const int bad = mfcc_rs::geometry(in_rate, out_rate, g);
    return bad == 1 ? MFCC_HIP_ERROR_INVALID_PARAM : bad ? MFCC_HIP_ERROR_UNSUPPORTED : MFCC_HIP_SUCCESS;
}

int rs_table(int in_rate, int out_rate, mfcc_rs::Geometry &g, std::vector<int16_t> &t) {
    const int rc = rs_geometry(in_rate, out_rate, g);
    if (rc) return rc;
    return mfcc_rs::build_taps(g, t) ? MFCC_HIP_SUCCESS : MFCC_HIP_ERROR_UNSUPPORTED;
}

// the ratio's table on the handle's device.  Another ratio than the last one's: the stream drains first, since
// kernels in flight may still read the old table
int rs_bind(mfcc_hip_handle *h, int in_rate, int out_rate, mfcc_rs::Taps &a) {
    if (h->rs_in != in_rate || h->rs_out != out_rate) {
        mfcc_rs::Geometry g;
        std::vector<int16_t> t;
        int rc = rs_table(in_rate, out_rate, g, t);
        if (rc) return rc;
        if (h->rs_in) HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->rs_in = h->rs_out = 0;
        if ((rc = ensure(h, h->d_rs_tab, t.size() * sizeof(int16_t)))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_rs_tab.p, t.data(), t.size() * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));          // t goes out of scope
        h->rs_geom = g;
        h->rs_in = in_rate;
        h->rs_out = out_rate;
    }
    a = mfcc_rs::Taps{static_cast<const int16_t *>(h->d_rs_tab.p), h->rs_geom.L, h->rs_geom.M, h->rs_geom.H, h->rs_geom.K};
    return MFCC_HIP_SUCCESS;
}

// a handle with an input rate (mfcc_hip_set_input_rate): every sample pointer is resampled to the handle's own rate
// behind the decode and in front of the route
inline bool rated(const mfcc_hip_handle *h) { return h && h->input_rate != 0; }

// n of a call's samples, at the handle's own rate (the WAV readers size their buffers by it)
inline size_t own_rate_len(const mfcc_hip_handle *h, size_t n) {
    mfcc_rs::Geometry g;
    if (!rated(h) || mfcc_rs::geometry(h->input_rate, h->r.sample_rate, g)) return n;
    return size_t(mfcc_rs::count(n, g.L, g.M));
}

// what a sample pointer handed to an entry point holds: the handle's format, at its input rate
inline Samples samples_of(const mfcc_hip_handle *h) { return Samples{h->sample_fmt, h->input_rate, h->center}; }

// ---- centring (include/mfcc_hip.h: "centring"; center_plan.hpp, kernel_center.hpp)
inline bool centred(Samples in) { return in.center != MFCC_HIP_CENTER_OFF; }
inline mfcc_center::Geom center_geom(const Resolved &r, int mode) {
    return mfcc_center::geometry(r.nfft, r.frame_len, r.hop, mode);
}
// n of a call's samples at the handle's own rate -> the samples the kernels frame: N'(n) of a centred call
inline size_t framed_len(const mfcc_hip_handle *h, Samples in, size_t n) {
    return centred(in) ? mfcc_center::padded(center_geom(h->r, in.center), n) : n;
}

// The descriptor of a call on h.  The handle's own passes behind the kernels belong to its own float output: a spectrum
// and a fixed-point call run none, whatever the handle is set up for, and a filterbank call runs the matrix's
// (h->fb_post, mfcc_hip_set_filterbank_post).  A filterbank bank's frame launch gets kNoPost through this too: a bank
// cannot exist together with those settings (bank_create_checked, mfcc_hip_set_filterbank_post)
inline Call call_of(const mfcc_hip_handle *h, Kind kind, bool fixed) {
    const Post &post = kind == Kind::kFeatures && !fixed ? h->post : kind == Kind::kFbank ? h->fb_post : kNoPost;
    const size_t w = kind == Kind::kFbank      ? size_t(h->fb.n_bands)
                     : kind == Kind::kSpectrum ? size_t(mfcc_spec::bins(h->r.nfft))
                                               : row_width(h->r);
    return Call{kind, fixed, w, w * size_t(1 + post.delta_order), post};
}

struct Arena {
    std::vector<char> host;
    template <typename T>
    size_t put(const std::vector<T> &v) {
        size_t off = (host.size() + 255) & ~size_t(255);
        host.resize(off + v.size() * sizeof(T));
        if (!v.empty()) std::memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
        return off;
    }
};

int build_tables(mfcc_hip_handle *h) {
    const Resolved &r = h->r;
    Arena a;
    // ---- float
    // the window in double; the kernels' tables carry it over den (they form the integer den x[i] - num x[i-1]): one
    // rounding of w / den to fp32
    const std::vector<double> wfull = frame_window(r);
    const int pe_num = r.front.num, pe_den = r.front.den;
    std::vector<double> wd(wfull.size());
    for (size_t i = 0; i < wd.size(); ++i) wd[i] = wfull[i] / double(pe_den);
    std::vector<float> win(wd.begin(), wd.end());
    const int M = r.nfft / 2;
    std::vector<float2> twf(M), tws(M + 1);
    for (int m = 0; m < M; ++m) {
        double ang = -2.0 * kPi * double(m) / double(M);
        twf[m] = make_float2(float(std::cos(ang)), float(std::sin(ang)));
    }
    for (int k = 0; k <= M; ++k) {
        double ang = -2.0 * kPi * double(k) / double(r.nfft);
        tws[k] = make_float2(float(std::cos(ang)), float(std::sin(ang)));
    }
    std::vector<double> md = handle_mel(r);
    const double inv_s2 = 1.0 / (r.power_scale * r.power_scale);
    std::vector<float> mdf(md.size());
    for (size_t i = 0; i < md.size(); ++i) mdf[i] = float(md[i] * inv_s2);
    std::vector<float> melw;
    SparseRows ms = pack_rows(mdf, r.n_mel, M + 1, melw);
    if (melw.empty()) melw.push_back(0.0f);
    std::vector<double> dd = dct_rows(r.n_cep, r.n_mel, r.lifter);
    std::vector<float> dct(dd.begin(), dd.end());

    bool dc_exact = false;                     // some filter has weight on the real-valued DC bin: that bin in double
    for (int f = 0; f < r.n_mel; ++f) dc_exact = dc_exact || md[size_t(f) * (M + 1)] != 0.0;
    size_t o_wd = dc_exact ? a.put(wd) : 0;
    size_t o_win = a.put(win), o_twf = a.put(twf), o_tws = a.put(tws);
    size_t o_ms = a.put(ms.start), o_mc = a.put(ms.count), o_mo = a.put(ms.off);
    size_t o_mw = a.put(melw), o_dct = a.put(dct);

    // ---- fixed
    size_t o_cv = 0, o_xt = 0, o_xd = 0, o_xs = 0, o_xc = 0, o_xo = 0, o_xw = 0;
    int x5_w_total = 0, x5_chunk = 0, x5_span = 0;
    bool x5_lanes_ok = false;
    std::vector<int> x5_lanes;
    std::vector<uint32_t> x5_wl;
    FxMel fm;
    const bool have_fixed = fixed_supported(r) && !is_logmel(r);     // log-mel output is float only: every fixed entry point refuses
    if (have_fixed) {
        std::vector<int> cv = fx_window_curve(r.nfft);
        std::vector<int> re, im;
        fx_twiddles(r.nfft, re, im);
        // twiddles as dot2 operand pairs: A = (twr, -twi), B = (twi, twr) (kernels_generic.hpp: fx_bfly)
        auto pack = [](int tre, int tim) {
            return make_uint2((uint32_t(tre) & 0xffffu) | (uint32_t(-tim) << 16), (uint32_t(tim) & 0xffffu) | (uint32_t(tre) << 16));
        };
        std::vector<uint2> t1(re.size());
        for (size_t i = 0; i < re.size(); ++i) t1[i] = pack(re[i], im[i]);
        fx_twiddles(4 * r.n_mel, re, im);
        std::vector<uint2> t2(re.size());
        for (size_t i = 0; i < re.size(); ++i) t2[i] = pack(re[i], im[i]);
        fm = fx_mel(r.nfft, r.n_mel, double(r.sample_rate));
        std::vector<uint32_t> xw;
        SparseRows xs = pack_rows(fm.dense, r.n_mel, r.nfft / 2, xw);
        if (xw.empty()) xw.push_back(0u);
        o_cv = a.put(cv); o_xt = a.put(t1); o_xd = a.put(t2);
        o_xs = a.put(xs.start); o_xc = a.put(xs.count); o_xo = a.put(xs.off); o_xw = a.put(xw);
        x5_w_total = (int)xw.size();
        x5_lanes_ok = mfcc_fixed512::build_mel_lanes(xs.start, xs.count, xs.off, xw, x5_lanes, x5_wl, x5_chunk, x5_span);
    }
    // ---- fused fixed-point kernel (the RTL's own configuration)
    std::vector<char> x5_blob;
    uint32_t x5_tw[4] = {0, 0, 0, 0};
    const bool have_fixed512 = have_fixed && mfcc_fixed512::supported(r.nfft, r.n_mel, r.n_cep) && x5_lanes_ok &&
                               mfcc_fixed512::build_tables(r.n_mel, x5_blob, x5_tw);
    size_t o_x5 = 0, o_x5l = 0, o_x5w = 0;
    if (have_fixed512) {
        o_x5 = a.put(x5_blob);
        o_x5l = a.put(x5_lanes);
        o_x5w = a.put(x5_wl);
    }

    // ---- fused 512/170/32 kernel tables
    std::vector<char> fused_blob;
    bool have_fused = false;
    h->fused_dense = false;
    bool fused_dcx = false;
    // a framed handle (frame_len < nfft) runs none of the fused forms below: their windows span nfft samples
    // ... and an HTK-bank handle runs the matrix-driven hop-160 form or the generic kernel, nothing else: the band
    // schedules and DC paths of the other forms are built around the notebook bank
    // ... and another front than the reference's runs the four-wave 512 forms (pair up to num + den = 127) or the generic
    // kernel: the twelve-wave 512 kernel's DC path folds 31/32 and a window symmetric about sample 256 into its digits, and
    // the 1024 forms keep the pair at compile time.  The choice refuses; it never mis-computes
    const bool framed = is_framed(r), htk = is_htk(r), fronted = is_fronted(r), pair_fused = front_fused(r.front);
    std::vector<char> fmb_blob;
    uint32_t fmb_mask = 0;
    const bool have_h160mb = htk && pair_fused &&
                             mfcc_fused160mb::supported(r.nfft, r.hop, r.frame_len, r.n_mel, r.n_cep, is_logmel(r)) &&
                             mfcc_fused160mb::build_tables(md, r.n_mel, r.n_cep, wfull, pe_den, r.power_scale, r.lifter, fmb_blob,
                                                           fmb_mask);
    const size_t o_fmb = have_h160mb ? a.put(fmb_blob) : 0;
    bool have_h160 = false;
    // the window the hop-170 tables are built with: the front's over all 512 samples (a framed handle's goes in behind)
    const std::vector<double> w512 = r.nfft == mfcc_fused::kNfft ? front_window(r.front, mfcc_fused::kNfft) : std::vector<double>();
    auto fused_tables = [&](bool dense) {
        return dense ? mfcc_fused::build_tables<true>(r.sample_rate, r.power_scale, r.lifter, r.n_cep, r.n_mel, w512, pe_num,
                                                      pe_den, fused_blob)
                     : mfcc_fused::build_tables<false>(r.sample_rate, r.power_scale, r.lifter, r.n_cep, r.n_mel, w512, pe_num,
                                                       pe_den, fused_blob);
    };
    if (!htk && framed && pair_fused && mfcc_fused160::supported(r.nfft, r.hop, r.frame_len, r.n_mel, r.n_cep)) {
        // the tables of the hop-170 form (none of them depends on the hop) with the frame's window in place of theirs
        fused_dcx = mfcc_fused::needs_dc_exact(r.sample_rate, r.n_mel);
        have_h160 = !fused_dcx && fused_tables(false);
        if (!have_h160) {
            h->fused_dense = true;
            have_h160 = fused_tables(true);
        }
        if (have_h160) mfcc_fused160::set_window(fused_blob, h->fused_dense, wfull, pe_den);
    }
    // a fronted handle has the four-wave form here, which has no log-mel tail: its log-mel rows come from the generic kernel
    if (!htk && !framed && pair_fused && !(fronted && is_logmel(r)) && mfcc_fused::supported(r.nfft, r.hop, r.n_mel, r.n_cep)) {
        fused_dcx = mfcc_fused::needs_dc_exact(r.sample_rate, r.n_mel);    // only the dense instantiation has the DC path
        have_fused = !fused_dcx && fused_tables(false);
        if (!have_fused) {
            h->fused_dense = true;
            have_fused = fused_tables(true);
        }
    }
    size_t o_fu = 0;
    if (have_fused || have_h160) o_fu = a.put(fused_blob);
    std::vector<char> f1k_blob;
    int f1k_var = 0;
    bool f1k_fp32 = false, f1k_twelve = false;
    bool have_1k = !htk && !framed && !fronted && mfcc_fused1024::supported(r.nfft, r.hop, r.n_mel, r.n_cep);
    if (have_1k) {
        // Default: the twelve-wave staging with the bf16-split contraction (kernel_fused1024_w12.hpp), every rate.
        // MFCC_HIP_FUSED1024 is a diagnostic override for A/B runs -- f32 / bf16: the eight-wave lockstep staging of
        // either contraction; w12 / w12bf: the twelve-wave staging of either (fp32: the five rates it has lists for)
        // a log-mel handle ignores it: only the default form has a log-mel tail
        const char *e = is_logmel(r) ? nullptr : std::getenv("MFCC_HIP_FUSED1024");
        auto is = [&](const char *v) { return e && !std::strcmp(e, v); };
        const bool no_f32 = !(is("f32") || is("w12")), no_bf16 = is("f32") || is("w12");
        f1k_twelve = !(is("f32") || is("bf16"));
        f1k_fp32 = !no_f32 && mfcc_fused1024_f32::build_tables(r.sample_rate, r.power_scale, r.lifter, r.n_cep, f1k_blob, f1k_var);
        if (!f1k_fp32)
            have_1k = !no_bf16 && mfcc_fused1024::build_tables(r.sample_rate, r.power_scale, r.lifter, r.n_cep, f1k_blob, f1k_var);
    }
    size_t o_f1k = 0;
    if (have_1k) o_f1k = a.put(f1k_blob);
    // ---- the power-spectrum kernels: the generic one reads the float tables above; the fused one has a blob of its own
    const bool power_generic = r.float_impl == MFCC_HIP_IMPL_GENERIC || !pair_fused;   // the power tile parks with preemph8
    h->spec_kernel = mfcc_spec::choose(r.nfft, r.hop, r.frame_len, power_generic);
    h->fb_kernel = mfcc_fbank::choose(r.nfft, r.hop, r.frame_len, power_generic);
    std::vector<char> spec_blob;
    size_t o_spec = 0;
    if (h->spec_kernel == mfcc_spec::Kernel::kFused512) {
        mfcc_spec::build_tables(wfull, spec_blob, pe_den);
        o_spec = a.put(spec_blob);
    }

    HIP_TRY(h, hipMalloc(&h->arena, a.host.size() + 256));
    HIP_TRY(h, hipMemcpy(h->arena, a.host.data(), a.host.size(), hipMemcpyHostToDevice));
    char *b = static_cast<char *>(h->arena);
    h->ft.window = reinterpret_cast<const float *>(b + o_win);
    h->ft.tw_fft = reinterpret_cast<const float2 *>(b + o_twf);
    h->ft.tw_split = reinterpret_cast<const float2 *>(b + o_tws);
    h->ft.mel_start = reinterpret_cast<const int *>(b + o_ms);
    h->ft.mel_count = reinterpret_cast<const int *>(b + o_mc);
    h->ft.mel_off = reinterpret_cast<const int *>(b + o_mo);
    h->ft.mel_w = reinterpret_cast<const float *>(b + o_mw);
    h->ft.mel_w_total = (int)melw.size();
    h->ft.dct = reinterpret_cast<const float *>(b + o_dct);
    h->ft.window_d = dc_exact ? reinterpret_cast<const double *>(b + o_wd) : nullptr;
    h->ft.n_mel = r.n_mel;
    h->ft.n_cep = r.n_cep;
    h->ft.pe_num = float(pe_num);
    h->ft.pe_den = float(pe_den);
    h->ft.pe_num_i = pe_num;
    h->ft.pe_den_i = pe_den;
    const int pair = packed_preemph(pe_num, pe_den);
    if (have_fixed) {
        h->xt.curve = reinterpret_cast<const int *>(b + o_cv);
        h->xt.tw_fft = reinterpret_cast<const uint2 *>(b + o_xt);
        h->xt.tw_dct = reinterpret_cast<const uint2 *>(b + o_xd);
        h->xt.mel_start = reinterpret_cast<const int *>(b + o_xs);
        h->xt.mel_count = reinterpret_cast<const int *>(b + o_xc);
        h->xt.mel_off = reinterpret_cast<const int *>(b + o_xo);
        h->xt.mel_w = reinterpret_cast<const uint32_t *>(b + o_xw);
        h->xt.mel_w_total = x5_w_total;
        h->xt.mel_shift = fm.shift;
        h->xt.log2_mel = ilog2(r.n_mel);
        h->xt.nfft = r.nfft;
        h->xt.log2_nfft = ilog2(r.nfft);
        h->xt.n_mel = r.n_mel;
        h->xt.log2_dct = ilog2(4 * r.n_mel);
        h->xt.n_cep = r.n_cep;
    }
    if (have_fused || have_h160) {
        mfcc_fused::bind_tables(b + o_fu, r.n_cep, r.n_mel, h->fused_dense, fused_dcx, h->fu);
        h->fu.preemph = pair;
    }
    if (have_h160mb) mfcc_fused160mb::bind_tables(b + o_fmb, r.n_cep, r.n_mel, fmb_mask, h->fmb, pair);
    if (have_1k) {
        if (f1k_fp32) mfcc_fused1024_f32::bind_tables(b + o_f1k, r.n_cep, f1k_var, h->f1k_f32);
        else mfcc_fused1024::bind_tables(b + o_f1k, r.n_cep, f1k_var, h->f1k);
    }
    if (h->spec_kernel == mfcc_spec::Kernel::kFused512) mfcc_spec::bind_tables(b + o_spec, r.power_scale, h->sf, pair);
    if (have_fixed512) {
        mfcc_fixed512::bind_tables(b + o_x5, h->x5);
        h->x5.tw64a = x5_tw[0]; h->x5.tw64b = x5_tw[1]; h->x5.tw192a = x5_tw[2]; h->x5.tw192b = x5_tw[3];
        h->x5.mel_lane = reinterpret_cast<const int4 *>(b + o_x5l);
        h->x5.mel_chunk = x5_chunk;
        h->x5.mel_span = x5_span;
        h->x5.mel_wl = reinterpret_cast<const uint32_t *>(b + o_x5w);
        h->x5.mel_shift = fm.shift;
        h->x5.n_cep = r.n_cep;
        h->x5.n_mel = r.n_mel;
    }

    // ---- the kernel of every later call, from what was built above and the handle's float_impl
    h->fixed_kernel = have_fixed512 ? FixedKernel::kFixed512 : have_fixed ? FixedKernel::kGeneric : FixedKernel::kNone;
    // diagnostic override for A/B runs: MFCC_HIP_FUSED512=w4 keeps the four-wave form (not on a log-mel handle: the
    // four-wave form has no log-mel tail)
    const char *e512 = is_logmel(r) ? nullptr : std::getenv("MFCC_HIP_FUSED512");
    const bool w4 = fronted || (e512 && std::strcmp(e512, "w4") == 0);
    h->float_kernel = FloatKernel::kGeneric;
    if (r.float_impl == MFCC_HIP_IMPL_GENERIC) {
        // the tables above stay allocated and unused
    } else if (have_h160mb) {
        h->float_kernel = FloatKernel::kFused512H160Mb;
    } else if (have_h160) {
        h->float_kernel = FloatKernel::kFused512H160;
    } else if (have_fused) {
        h->float_kernel = w4 ? FloatKernel::kFused512 : FloatKernel::kFused512W12;
    } else if (have_1k && r.float_impl == MFCC_HIP_IMPL_AUTO) {
        h->float_kernel = f1k_twelve ? (f1k_fp32 ? FloatKernel::kFused1024W12F32 : FloatKernel::kFused1024W12Bf)
                                     : (f1k_fp32 ? FloatKernel::kFused1024F32 : FloatKernel::kFused1024Bf);
    }
    return MFCC_HIP_SUCCESS;
}

// the generic float kernel for every nfft; LOGMEL: its log-mel form
template <bool LOGMEL>
int launch_generic(mfcc_hip_handle *h, const mfcc_k::StreamDesc &s, unsigned blocks, float *o) {
    switch (h->r.nfft) {
#define MFCC_GEN_CASE(N)                                                                                           \
    case N:                                                                                                        \
        hipLaunchKernelGGL((mfcc_k::mfcc_float_generic_kernel<N, LOGMEL>), dim3(blocks), dim3(mfcc_k::kBlock), 0,  \
                           h->stream, s, h->ft, o);                                                                \
        break;
        MFCC_GEN_CASE(64)
        MFCC_GEN_CASE(128)
        MFCC_GEN_CASE(256)
        MFCC_GEN_CASE(512)
        MFCC_GEN_CASE(1024)
#undef MFCC_GEN_CASE
        default:
            return MFCC_HIP_ERROR_UNSUPPORTED;
    }
    return MFCC_HIP_SUCCESS;
}

// what the generic spectrum and filterbank kernels read of the handle's float tables
mfcc_k::PowerTables power_tables(const mfcc_hip_handle *h) {
    return {h->ft.window, h->ft.tw_fft, h->ft.tw_split, float(1.0 / (h->r.power_scale * h->r.power_scale)), h->ft.pe_num,
            h->ft.pe_den};
}

// The kernel of a call over int16 samples: the spectrum's, the filterbank's or the handle's own, as c says
int launch(mfcc_hip_handle *h, const Call &c, const void *d_pcm, size_t n, size_t stride, size_t nch,
           int halo, void *d_out, size_t *n_frames, size_t force_frames = 0) {
    const bool fixed = c.fixed;
    if ((!d_pcm && n * nch) || halo < 0 || halo > 1) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (fixed && h->fixed_kernel == FixedKernel::kNone) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (!fixed && h->r.float_impl == MFCC_HIP_IMPL_FUSED512 && !is_fused512(h->float_kernel))
        return MFCC_HIP_ERROR_UNSUPPORTED;
    // force_frames: the packed stream of the ragged entry points -- every hop position is a frame
    const size_t nf = force_frames ? force_frames : count_frames(h->r, n);
    if (n_frames) *n_frames = nf;
    if (nf == 0 || nch == 0) return MFCC_HIP_SUCCESS;
    if (!d_out) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (nch > 1 && stride < n + size_t(halo)) return MFCC_HIP_ERROR_INVALID_PARAM;

    mfcc_k::StreamDesc s;
    s.pcm = static_cast<const int16_t *>(d_pcm) + halo;
    s.ch_stride = (long long)stride;
    s.n_samples = (long long)n;
    s.halo = halo;
    s.frames_per_ch = (long long)nf;
    s.total_frames = (long long)(nf * nch);
    s.hop = h->r.hop;

    DeviceGuard guard(h->device);
    const long long total = s.total_frames;
    const bool logmel = is_logmel(h->r);
    if (c.kind == Kind::kFbank) {
        // the fused kernel, or the generic one where the problem does not fit its tiles
        float *o = static_cast<float *>(d_out);
        if (reinterpret_cast<uintptr_t>(o) & 3) return MFCC_HIP_ERROR_INVALID_PARAM;
        const bool log = h->fb_scale != MFCC_HIP_FBANK_ENERGY;
        if (h->fb_kernel != mfcc_fbank::Kernel::kFused512 || !mfcc_fbank::launch_fused(s, h->sf, h->fb, log, o, h->n_cu, h->stream)) {
            if (!mfcc_fbank::launch_generic(s, power_tables(h), h->fb, log, h->r.nfft, o, h->n_cu, h->stream)) return MFCC_HIP_ERROR_UNSUPPORTED;
        }
        h->fb_used = true;
    } else if (c.kind == Kind::kSpectrum) {
        float *o = static_cast<float *>(d_out);
        if (reinterpret_cast<uintptr_t>(o) & 3) return MFCC_HIP_ERROR_INVALID_PARAM;
        if (h->spec_kernel != mfcc_spec::Kernel::kFused512 || !mfcc_spec::launch_fused(s, h->sf, o, h->n_cu, h->stream)) {
            if (!mfcc_spec::launch_generic(s, power_tables(h), h->r.nfft, o, h->n_cu, h->stream)) return MFCC_HIP_ERROR_UNSUPPORTED;
        }
    } else if (fixed && h->fixed_kernel == FixedKernel::kFixed512) {
        mfcc_fixed512::launch(s, h->x5, static_cast<int16_t *>(d_out), h->n_cu, h->stream);
    } else if (fixed) {
        long long blocks = (total + mfcc_k::kWavesPerBlock - 1) / mfcc_k::kWavesPerBlock;
        long long cap = (long long)h->n_cu * 32;     // a deep queue of workgroups, not a merely full grid (kernel_fixed512.hpp: launch)
        if (blocks > cap) blocks = cap;
        size_t lds = size_t(mfcc_k::kWavesPerBlock) *
                         (size_t(h->r.nfft + h->r.nfft / 32) * sizeof(uint32_t) + size_t(h->r.nfft / 2) * 4 + mfcc_k::kMaxMel * 4) +
                     size_t((h->xt.mel_w_total + 1) & ~1) * sizeof(uint32_t) +            // filterbank weights,
                     (size_t(h->r.nfft / 2) + size_t(2 * h->r.n_mel)) * sizeof(uint2);     // both twiddle ROMs
        int16_t *o = static_cast<int16_t *>(d_out);
        switch (h->r.nfft) {
#define MFCC_FX_CASE(N)                                                                                            \
    case N:                                                                                                        \
        hipLaunchKernelGGL(mfcc_k::mfcc_fixed_kernel<N>, dim3((unsigned)blocks), dim3(mfcc_k::kBlock), lds, h->stream, \
                           s, h->xt, o);                                                                           \
        break;
            MFCC_FX_CASE(64)
            MFCC_FX_CASE(128)
            MFCC_FX_CASE(256)
            MFCC_FX_CASE(512)
            MFCC_FX_CASE(1024)
#undef MFCC_FX_CASE
            default:
                return MFCC_HIP_ERROR_UNSUPPORTED;
        }
    } else {
        float *o = static_cast<float *>(d_out);
        hipStream_t st = h->stream;
        const int n_cu = h->n_cu;
        bool generic = false;
        // A kernel's launch answers false where the problem does not fit its 32-bit tile arithmetic.  A twelve-wave
        // form then falls through to the four- / eight-wave form of the same tables, and a 1024 form from there to
        // the generic kernel; a 512 form and a log-mel handle answer UNSUPPORTED.
        switch (h->float_kernel) {
        case FloatKernel::kFused512H160Mb:
            if (!(logmel ? mfcc_fused160mb::launch<true>(s, h->fmb, o, n_cu, st) : mfcc_fused160mb::launch<false>(s, h->fmb, o, n_cu, st)))
                return MFCC_HIP_ERROR_UNSUPPORTED;
            break;
        case FloatKernel::kFused512H160:
            if (!(logmel ? mfcc_fused160::launch<true>(s, h->fu, h->fused_dense, o, n_cu, st)
                         : mfcc_fused160::launch<false>(s, h->fu, h->fused_dense, o, n_cu, st)))
                return MFCC_HIP_ERROR_UNSUPPORTED;
            break;
        case FloatKernel::kFused512W12:
            if (logmel ? mfcc_fused12::launch<true>(s, h->fu, h->fused_dense, o, n_cu, st)
                       : mfcc_fused12::launch<false>(s, h->fu, h->fused_dense, o, n_cu, st))
                break;
            if (logmel) return MFCC_HIP_ERROR_UNSUPPORTED;       // the four-wave form has no log-mel tail
            [[fallthrough]];     // does not fit: the four-wave form
        case FloatKernel::kFused512:
            if (!mfcc_fused::launch(s, h->fu, h->fused_dense, o, n_cu, st)) return MFCC_HIP_ERROR_UNSUPPORTED;
            break;
        case FloatKernel::kFused1024W12Bf:
            if (logmel ? mfcc_fused1024_w12bf::launch<true>(s, h->f1k, o, n_cu, st)
                       : mfcc_fused1024_w12bf::launch<false>(s, h->f1k, o, n_cu, st))
                break;
            if (logmel) return MFCC_HIP_ERROR_UNSUPPORTED;       // the eight-wave form has no log-mel tail
            [[fallthrough]];     // does not fit: the eight-wave form
        case FloatKernel::kFused1024Bf:
            generic = !mfcc_fused1024::launch(s, h->f1k, o, n_cu, st);       // does not fit: the generic kernel
            break;
        case FloatKernel::kFused1024W12F32:
            if (mfcc_fused1024_w12::launch(s, h->f1k_f32, o, n_cu, st)) break;
            [[fallthrough]];     // does not fit: the eight-wave form
        case FloatKernel::kFused1024F32:
            generic = !mfcc_fused1024_f32::launch(s, h->f1k_f32, o, n_cu, st);   // does not fit: the generic kernel
            break;
        case FloatKernel::kGeneric:
            generic = true;
            break;
        }
        if (generic) {
            const unsigned blocks = mfcc_k::generic_grid(s, n_cu);
            const int rc = logmel ? launch_generic<true>(h, s, blocks, o) : launch_generic<false>(h, s, blocks, o);
            if (rc) return rc;
        }
    }
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

// ---- the tiles and the scratch of a segment pass (seg_plan.hpp).  Normalization, PCEN, deltas,
// sliding normalization, the VAD, the selection and the gate all stage here; each brings its own tile size, its own
// buffer, the areas it wants in front of the table, and its kernels.
using namespace mfcc_seg;

struct Staged {
    mfcc_norm::Segs s;                      // the table form points at the device copy
    const long long *extra;                 // the extra column there (nullptr: none, or the uniform form)
    char *area[kMaxAreas];
};

// The tiles of tile_rows units of a span that is not empty, with `areas` in buf: count, pinned buffer and fill (table
// form only), buf grown (a pass that needs no byte allocates nothing) and taken, the table on its way behind the areas
int seg_stage(mfcc_hip_handle *h, const SegSpan &sp, int width, int tile_rows, const Column *extra, DevBuf &buf,
              const Area *areas, int n_areas, Staged &st) {
    Plan pl;
    int rc = plan_count(sp, width, tile_rows, extra, pl);
    if (rc) return rc;
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    if (pl.table_ll) {
        if ((rc = desc_acquire(h, pl.table_ll, &pd))) return rc;
        plan_fill(sp, extra, pl, pd->p);
    }
    const Scratch lay = lay_out(areas, n_areas, pl);
    if ((rc = desc_stage(h, buf, n_areas || pd ? lay.total : 0, pd, pl.table_ll, lay.table_off))) return rc;
    char *base = static_cast<char *>(buf.p);
    st.extra = plan_bind(pl, reinterpret_cast<const long long *>(base + lay.table_off));
    st.s = pl.s;
    for (int i = 0; i < n_areas; ++i) st.area[i] = base + lay.off[i];
    return MFCC_HIP_SUCCESS;
}

inline unsigned tile_grid(long long n) { return unsigned(std::min<long long>(n, 1 << 20)); }

// ---- per-segment mean / variance normalization (kernel_normalize.hpp): in place.
// Scratch (h->d_norm): [tile partials: n_blocks * W * 24 B][coefficients: n_segs * W * 8 B][tile table]
// Rows of more than 64 floats (a filterbank call's; the direct entry refuses them) go to the wide kernels of post_wide.hip:
// the same tiles, the same scratch
int normalize_pass(mfcc_hip_handle *h, float *d_rows, int width, const SegSpan &sp, int mode) {
    if (span_empty(sp) || mode == MFCC_HIP_NORMALIZE_NONE) return MFCC_HIP_SUCCESS;
    static_assert(mfcc_norm::kTileFloats == mfcc_post::kNormTileFloats && mfcc_norm::kMaxWidth == mfcc_post::kNarrowWidth, "post_plan.hpp");
    const size_t W = size_t(width);
    const Area areas[] = {{W * sizeof(mfcc_norm::Part), 0, 0}, {0, W * sizeof(float2), 0}};
    Staged st;
    const int rc = seg_stage(h, sp, width, mfcc_norm::tile_rows(width), nullptr, h->d_norm, areas, 2, st);
    if (rc) return rc;
    if (mfcc_post::wide_rows(width)) {
        mfcc_post_wide::launch_normalize(d_rows, st.s, st.area[0], st.area[1], mode, h->n_cu, h->stream);
        HIP_TRY(h, hipGetLastError());
        return scratch_release(h);
    }
    auto *part = reinterpret_cast<mfcc_norm::Part *>(st.area[0]);
    auto *coef = reinterpret_cast<float2 *>(st.area[1]);
    const mfcc_norm::Segs &s = st.s;
    const unsigned grid = tile_grid(s.n_blocks), grid_f = tile_grid(s.n_segs);
    hipLaunchKernelGGL(mfcc_norm::normalize_stats_kernel, dim3(grid), dim3(mfcc_norm::kThreads), 0, h->stream,
                       static_cast<const float *>(d_rows), s, part);
    hipLaunchKernelGGL(mfcc_norm::normalize_finalize_kernel, dim3(grid_f), dim3(mfcc_norm::kThreads), 0, h->stream, s,
                       static_cast<const mfcc_norm::Part *>(part), coef, mode);
    hipLaunchKernelGGL(mfcc_norm::normalize_apply_kernel, dim3(grid), dim3(mfcc_norm::kThreads), 0, h->stream, d_rows, s,
                       static_cast<const float2 *>(coef));
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

// ---- PCEN (kernel_pcen.hpp): in place on the raw log-mel rows.
// Scratch (h->d_pcen): [tile ends: n_blocks * W floats][carries: n_blocks * W floats][tile table]
bool pcen_ok(const mfcc_hip_pcen *p) {
    if (!p || p->struct_size != sizeof(mfcc_hip_pcen) || p->reserved[0] || p->reserved[1] || p->reserved[2]) return false;
    if (!std::isfinite(p->s) || !std::isfinite(p->alpha) || !std::isfinite(p->delta) || !std::isfinite(p->r) ||
        !std::isfinite(p->eps))
        return false;
    return p->s > 0.0f && p->s <= 1.0f && p->alpha >= 0.0f && p->alpha <= 1.0f && p->delta >= 0.0f && p->r > 0.0f &&
           p->r <= 1.0f && p->eps > 0.0f;
}

// what mfcc_hip_set_normalize, _set_normalize_window and _set_deltas take, and mfcc_hip_set_filterbank_post with them
inline bool normalize_mode_ok(int mode) { return mode >= MFCC_HIP_NORMALIZE_NONE && mode <= MFCC_HIP_NORMALIZE_MEAN_VAR; }
inline bool normalize_window_ok(int window, int min_window, int center) {
    if (center < 0 || center > 1 || window < 0 || window > MFCC_HIP_MAX_NORMALIZE_WINDOW) return false;
    return !window || (min_window >= 1 && min_window <= window);
}
inline bool deltas_ok(int order, int window) { return order >= 0 && order <= 2 && window >= 1 && window <= MFCC_HIP_MAX_DELTA_WINDOW; }

// the constants of the tile form: float64 on the host, rounded once
mfcc_pcen::Prm pcen_prm(const mfcc_hip_pcen &p) {
    mfcc_pcen::Prm q{};
    const double d = 1.0 - double(p.s);
    q.s = p.s;
    q.a = float(d);
    q.alpha = p.alpha;
    q.r = p.r;
    q.eps = p.eps;
    q.delta = p.delta;
    q.delta_r = float(std::pow(double(p.delta), double(p.r)));
    for (int k = 0; k < mfcc_pcen::kTile; ++k) q.decay[k] = float(std::pow(d, double(k + 1)));
    return q;
}

int pcen_pass(mfcc_hip_handle *h, float *d_rows, int width, const SegSpan &sp, const mfcc_pcen::Prm &prm) {
    if (span_empty(sp)) return MFCC_HIP_SUCCESS;
    const Area areas[] = {{size_t(width) * sizeof(float), 0, 0}, {size_t(width) * sizeof(float), 0, 0}};
    Staged st;
    const int rc = seg_stage(h, sp, width, mfcc_pcen::kTile, nullptr, h->d_pcen, areas, 2, st);
    if (rc) return rc;
    float *lend = reinterpret_cast<float *>(st.area[0]), *carry = reinterpret_cast<float *>(st.area[1]);
    const mfcc_norm::Segs &s = st.s;
    const long long G = mfcc_pcen::tiles_per_group(s.width);
    const unsigned grid = tile_grid((s.n_blocks + G - 1) / G);
    const unsigned grid_c = tile_grid((s.n_segs * s.width + mfcc_pcen::kThreads - 1) / mfcc_pcen::kThreads);
    hipLaunchKernelGGL(mfcc_pcen::pcen_tile_end_kernel, dim3(grid), dim3(mfcc_pcen::kThreads), 0, h->stream,
                       static_cast<const float *>(d_rows), s, prm, lend);
    hipLaunchKernelGGL(mfcc_pcen::pcen_carry_kernel, dim3(grid_c), dim3(mfcc_pcen::kThreads), 0, h->stream,
                       static_cast<const float *>(d_rows), s, prm, static_cast<const float *>(lend), carry);
    hipLaunchKernelGGL(mfcc_pcen::pcen_apply_kernel, dim3(grid), dim3(mfcc_pcen::kThreads), 0, h->stream, d_rows, s, prm,
                       static_cast<const float *>(carry));
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

// ---- delta coefficients (kernel_deltas.hpp): out of place, the last step of post_chain.  The
// tile table of a ragged call goes to h->d_dtab.  Rows of more than 64 floats (a filterbank call's; the direct entry refuses
// them) go to the wide kernel of post_wide.hip, on its larger tiles
int deltas_pass(mfcc_hip_handle *h, const float *d_in, float *d_out, int width, const SegSpan &sp, int order, int window) {
    if (span_empty(sp)) return MFCC_HIP_SUCCESS;
    static_assert(mfcc_delta::kLdsFloats == mfcc_post::kDeltaLdsFloats && mfcc_delta::kMaxWidth == mfcc_post::kNarrowWidth, "post_plan.hpp");
    const bool wide = mfcc_post::wide_rows(width);
    const int tile = wide ? mfcc_post::delta_wide_tile_rows(width, order, window) : mfcc_delta::tile_rows(width, order, window);
    Staged st;
    const int rc = seg_stage(h, sp, width, tile, nullptr, h->d_dtab, nullptr, 0, st);
    if (rc) return rc;
    if (wide) {
        if (!mfcc_post_wide::launch_deltas(d_in, d_out, st.s, order, window, h->n_cu, h->stream)) return MFCC_HIP_ERROR_INVALID_PARAM;
        HIP_TRY(h, hipGetLastError());
        return scratch_release(h);
    }
    const mfcc_delta::DeltasKernel kernel = mfcc_delta::deltas_kernel_of(order, window);
    if (!kernel) return MFCC_HIP_ERROR_INVALID_PARAM;
    hipLaunchKernelGGL(kernel, dim3(tile_grid(st.s.n_blocks)), dim3(mfcc_delta::kThreads), 0, h->stream, d_in, d_out, st.s,
                       mfcc_delta::delta_scale(window));
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

// ---- sliding-window normalization (kernel_normalize_sliding.hpp): out of place, raw -> stat
// of post_route.  The tile table of a ragged call goes to h->d_stab
struct SlideArgs {
    int mode, window, min_window, center;
};

inline bool sliding(const Post &p) { return p.norm != MFCC_HIP_NORMALIZE_NONE && p.norm_window > 0; }
inline SlideArgs slide_args(const Post &p) { return SlideArgs{p.norm, p.norm_window, p.norm_min_window, p.norm_center}; }

int sliding_pass(mfcc_hip_handle *h, const float *d_in, float *d_out, int width, const SegSpan &sp, SlideArgs a) {
    if (span_empty(sp)) return MFCC_HIP_SUCCESS;
    Staged st;
    const int rc = seg_stage(h, sp, width, mfcc_slide::tile_rows(width, a.window), nullptr, h->d_stab, nullptr, 0, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mfcc_slide::normalize_sliding_kernel, dim3(tile_grid(st.s.n_blocks)), dim3(mfcc_slide::kThreads), 0,
                       h->stream, d_in, d_out, st.s, mfcc_slide::run_rows(a.window), a.window, a.min_window, a.center, a.mode);
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

// ---- energy VAD and voiced-row selection (kernel_vad.hpp).  The decision reads one column of
// the raw rows and writes a byte per row; the selection packs the rows whose byte is set.  Both work on tiles of the
// SAME plan when a handle with MFCC_HIP_VAD_SELECT runs them (the decision's tile counts feed the selection's prefix sum);
// the direct entries each make their own.
struct VadArgs {
    int column;
    float threshold, scale;
    int context;
    float proportion;
};

inline VadArgs vad_args(const Post &p) {
    return VadArgs{p.vad_column, p.vad_threshold, p.vad_scale, p.vad_context, p.vad_proportion};
}

inline bool vad_args_ok(int width, int column, float threshold, float scale, int context, float proportion) {
    return column >= 0 && column < width && std::isfinite(threshold) && std::isfinite(scale) && scale >= 0.0f &&
           context >= 0 && context <= MFCC_HIP_MAX_VAD_CONTEXT && proportion > 0.0f && proportion < 1.0f;
}

// the tiles of a selection and its scratch in h->d_sel: [tile counts][tile prefixes (n_blocks + 1)][segment offsets
// (n_segs + 1)][tile table]
struct SelPlan {
    mfcc_norm::Segs s;
    unsigned *counts;
    long long *tile_off, *seg_off;
};

inline SelPlan sel_plan_of(const Staged &st) {
    return SelPlan{st.s, reinterpret_cast<unsigned *>(st.area[0]), reinterpret_cast<long long *>(st.area[1]),
                   reinterpret_cast<long long *>(st.area[2])};
}

int select_plan(mfcc_hip_handle *h, const SegSpan &span, int tile_width, SelPlan &pl) {
    Staged st;
    const int rc = seg_stage(h, span, tile_width, mfcc_vad::select_tile_rows(tile_width), nullptr, h->d_sel,
                             kSelectAreas, 3, st);
    if (!rc) pl = sel_plan_of(st);
    return rc;
}

// the decision on column a.column of rows [..][W], on the tiles of pl (whose counts it fills).  Scratch (h->d_vad):
// [tile partials of the mean][theta per segment][tile table of the mean]
int vad_decide(mfcc_hip_handle *h, const float *d_rows, int W, const SegSpan &sp, VadArgs a, unsigned char *d_voiced,
               const SelPlan &pl) {
    const double *theta = nullptr;
    int rc;
    if (a.scale != 0.0f) {
        const Area areas[] = {{sizeof(mfcc_vad::MeanPart), 0, 0}, {0, sizeof(double), 0}};
        Staged mp;
        if ((rc = seg_stage(h, sp, W, mfcc_vad::kMeanTileRows, nullptr, h->d_vad, areas, 2, mp))) return rc;
        const mfcc_norm::Segs &sm = mp.s;
        auto *part = reinterpret_cast<mfcc_vad::MeanPart *>(mp.area[0]);
        double *th = reinterpret_cast<double *>(mp.area[1]);
        hipLaunchKernelGGL(mfcc_vad::vad_mean_kernel, dim3(tile_grid(sm.n_blocks)),
                           dim3(mfcc_vad::kThreads), 0, h->stream, d_rows, sm, a.column, part);
        hipLaunchKernelGGL(mfcc_vad::vad_theta_kernel, dim3(tile_grid(sm.n_segs)),
                           dim3(mfcc_vad::kThreads), 0, h->stream, sm, static_cast<const mfcc_vad::MeanPart *>(part),
                           double(a.threshold), double(a.scale), th);
        theta = th;
    }
    mfcc_norm::Segs sd = pl.s;
    sd.width = W;
    hipLaunchKernelGGL(mfcc_vad::vad_decide_kernel, dim3(tile_grid(sd.n_blocks)),
                       dim3(mfcc_vad::kThreads), 0, h->stream, d_rows, sd, a.column, theta, double(a.threshold), a.context,
                       a.proportion, d_voiced, pl.counts);
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

// the selection on the tiles of pl (made for rows of Wp floats): [count,] scan, gather, then the segment offsets to the
// host -- which is why this synchronizes the stream
int select_run(mfcc_hip_handle *h, const float *d_in, int Wp, const unsigned char *d_voiced, const SelPlan &pl, bool counted,
               float *d_out, size_t *out_offsets) {
    mfcc_norm::Segs s = pl.s;
    s.width = Wp;
    const unsigned grid = tile_grid(s.n_blocks);
    if (!counted)
        hipLaunchKernelGGL(mfcc_vad::vad_count_kernel, dim3(grid), dim3(mfcc_vad::kThreads), 0, h->stream, d_voiced, s,
                           pl.counts);
    hipLaunchKernelGGL(mfcc_vad::vad_scan_kernel, dim3(1), dim3(mfcc_vad::kScanThreads), 0, h->stream, s,
                       static_cast<const unsigned *>(pl.counts), pl.tile_off, pl.seg_off);
    hipLaunchKernelGGL(mfcc_vad::vad_gather_kernel, dim3(grid), dim3(mfcc_vad::kThreads), 0, h->stream, d_in, d_voiced, s,
                       static_cast<const long long *>(pl.tile_off), d_out);
    HIP_TRY(h, hipGetLastError());
    static_assert(sizeof(size_t) == sizeof(long long), "segment offsets are copied as they are");
    HIP_TRY(h, hipMemcpyAsync(out_offsets, pl.seg_off, size_t(s.n_segs + 1) * sizeof(long long), hipMemcpyDeviceToHost,
                              h->stream));
    const int rc = scratch_release(h);
    if (rc) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MFCC_HIP_SUCCESS;
}

// the decision alone, on tiles of its own
int vad_segments(mfcc_hip_handle *h, const float *d_rows, int W, const SegSpan &sp, VadArgs a, unsigned char *d_voiced) {
    if (span_empty(sp)) return MFCC_HIP_SUCCESS;
    SelPlan pl;
    int rc = select_plan(h, sp, 1, pl);                    // tiles of kMaxTileRows rows
    if (rc || (rc = vad_decide(h, d_rows, W, sp, a, d_voiced, pl))) return rc;
    return scratch_release(h);
}

// the selection alone: counts the mask's bytes itself
int select_segments(mfcc_hip_handle *h, const float *d_in, int Wp, const unsigned char *d_voiced, const SegSpan &sp,
                    float *d_out, size_t *out_offsets) {
    if (span_empty(sp)) {
        for (size_t k = 0; k <= sp.n_segs && out_offsets; ++k) out_offsets[k] = 0;
        return MFCC_HIP_SUCCESS;
    }
    SelPlan pl;
    const int rc = select_plan(h, sp, Wp, pl);
    if (rc) return rc;
    return select_run(h, d_in, Wp, d_voiced, pl, false, d_out, out_offsets);
}

// ---- the passes behind the float kernels.  Every float entry point of a handle runs them in
// ONE order, enqueued by post_chain and nowhere else: the VAD decision on the raw rows, PCEN, the normalization (sliding or
// per segment), deltas; the voiced-row selection (select_run) follows where the handle selects.
// A handle with any of them is refused (UNSUPPORTED) by every fixed-point entry point and by the entry points that see
// part of a stream: there is no fixed-point normalization, PCEN, delta or frame selection, and the float ones are
// whole-segment passes.
inline bool has_post(const Post &p) { return p.norm != MFCC_HIP_NORMALIZE_NONE || p.pcen_on || p.delta_order || p.vad_mode; }

// Where the rows of a call go.  The kernels write `raw`; PCEN works on it in place; the sliding normalization moves it to
// `stat`, the per-segment one works on `stat` (= raw) in place; deltas expand `stat` into `out`.  So `stat` is h->d_stat
// iff the call has a delta order (else out), and `raw` is h->d_slide iff its normalization slides (else stat).
struct PostRoute {
    float *raw, *stat, *out;
    unsigned char *voiced;      // the decision's byte per row (selection only)
    bool staged;                // some of them lie in the handle's scratch, acquired before the kernels: the caller
                                // releases it behind the chain (a selection: select_run does)
};

// the rule, at `at` floats into h->d_stat / h->d_slide (already grown)
inline PostRoute route_to(const mfcc_hip_handle *h, const Post &p, float *out, size_t at = 0) {
    PostRoute rt{};
    rt.out = out;
    rt.stat = p.delta_order ? static_cast<float *>(h->d_stat.p) + at : out;
    rt.raw = sliding(p) ? static_cast<float *>(h->d_slide.p) + at : rt.stat;
    rt.staged = p.delta_order || sliding(p);
    return rt;
}

// grows h->d_stat / h->d_slide for `rows` static rows where the rule needs them
int stage_rows(mfcc_hip_handle *h, const Call &c, size_t rows) {
    const size_t bytes = rows * c.width * sizeof(float) + 64;
    int rc = c.post.delta_order ? ensure(h, h->d_stat, bytes) : MFCC_HIP_SUCCESS;
    if (!rc && sliding(c.post)) rc = ensure(h, h->d_slide, bytes);
    return rc;
}

// the route of a device call of `rows` frames into d_out; select: every frame goes to h->d_final first and its byte to
// h->d_voiced, select_run then moves the voiced rows to d_out
int post_route(mfcc_hip_handle *h, const Call &c, size_t rows, float *d_out, bool select, PostRoute &rt) {
    int rc = MFCC_HIP_SUCCESS;
    if (select) {
        rc = ensure(h, h->d_final, rows * c.out_width * sizeof(float) + 64);
        if (!rc) rc = ensure(h, h->d_voiced, rows + 64);
    }
    if (rc || (rc = stage_rows(h, c, rows))) return rc;
    rt = route_to(h, c.post, select ? static_cast<float *>(h->d_final.p) : d_out);
    rt.voiced = select ? static_cast<unsigned char *>(h->d_voiced.p) : nullptr;
    rt.staged = rt.staged || select;
    return rt.staged ? scratch_acquire(h) : MFCC_HIP_SUCCESS;
}

// the chain over the segments of sp; sel: the tiles of the selection that follows, whose counts the decision fills
int post_chain(mfcc_hip_handle *h, const Call &c, const SegSpan &sp, const PostRoute &rt, const SelPlan *sel) {
    const Post &p = c.post;
    const int W = int(c.width);
    int rc;
    if (sel && (rc = vad_decide(h, rt.raw, W, sp, vad_args(p), rt.voiced, *sel))) return rc;
    if (p.pcen_on && (rc = pcen_pass(h, rt.raw, W, sp, p.pcen))) return rc;
    if ((rc = sliding(p) ? sliding_pass(h, rt.raw, rt.stat, W, sp, slide_args(p))
                         : normalize_pass(h, rt.stat, W, sp, p.norm)))
        return rc;
    if (p.delta_order && (rc = deltas_pass(h, rt.stat, rt.out, W, sp, p.delta_order, p.delta_window))) return rc;
    return MFCC_HIP_SUCCESS;
}

// the dense float device path: the launch, then the chain with one segment per channel
int launch_float_dev(mfcc_hip_handle *h, const Call &c, const void *d_pcm, size_t n, size_t stride, size_t nch, int halo,
                     void *d_out, size_t *n_frames) {
    // nothing behind the kernels (the headline of bench.py): the launch and nothing else
    if (!has_post(c.post)) return launch(h, c, d_pcm, n, stride, nch, halo, d_out, n_frames);
    if (halo) return MFCC_HIP_ERROR_UNSUPPORTED;                                 // a shard of a longer stream
    const size_t nf = count_frames(h->r, n);
    if (nf == 0 || nch == 0 || !d_out) return launch(h, c, d_pcm, n, stride, nch, 0, d_out, n_frames);
    DeviceGuard guard(h->device);
    PostRoute rt;
    int rc = post_route(h, c, nf * nch, static_cast<float *>(d_out), false, rt);
    if (rc || (rc = launch(h, c, d_pcm, n, stride, nch, 0, rt.raw, n_frames))) return rc;
    if ((rc = post_chain(h, c, span_uniform(0, nch, nf), rt, nullptr)) || !rt.staged) return rc;
    return scratch_release(h);
}

// ---- the input stage of a dense call (DESIGN.md sections 4.15, 4.17, 4.21): nch rows of n samples as `in` describes them
// (n + halo are read; a rate and centring take no halo) -> int16 rows at the handle's own rate: decoded into h->d_dec, then
// resampled into h->d_rs by the taps of a (rs_bind) to n2 samples a row, then centred into h->d_ctr to n3 samples a row.
// The centring kernel decodes while it pads, so a centred call without a rate runs no decode pass of its own.  p / stride:
// where the rows now lie; the scratch area is taken, the caller releases it behind the kernels that read them
struct DenseIn {
    const int16_t *p;
    size_t stride;
};
// the stride of `rows` resampled rows of n samples: rounded up to 8 samples where there is more than one
inline size_t rs_stride(size_t n, size_t rows) { return rows <= 1 ? n : (n + 7) & ~size_t(7); }

int dense_input(mfcc_hip_handle *h, Samples in, const void *d_pcm, size_t n, size_t stride, size_t nch, int halo,
                const mfcc_rs::Taps &a, size_t n2, size_t n3, DenseIn &o) {
    o = DenseIn{static_cast<const int16_t *>(d_pcm), nch <= 1 ? n : stride};
    int rc, fmt = in.fmt;                   // fmt: the format of the rows at o.p
    if (decodes(fmt) && (in.rate || !centred(in))) {
        if ((rc = decode_to_scratch(h, fmt, d_pcm, n + size_t(halo), nch, stride, &o.p, &o.stride))) return rc;
        fmt = MFCC_HIP_SAMPLE_S16;
    }
    if (in.rate) {
        const size_t stride2 = rs_stride(n2, nch);
        if ((rc = ensure(h, h->d_rs, nch * stride2 * sizeof(int16_t) + 64)) || (rc = scratch_acquire(h))) return rc;
        mfcc_rs::launch(a, o.p, (long long)n, static_cast<int16_t *>(h->d_rs.p), (long long)n2, (long long)nch, (long long)o.stride,
                        (long long)stride2, nullptr, 0, h->n_cu, h->stream);
        HIP_TRY(h, hipGetLastError());
        o = DenseIn{static_cast<const int16_t *>(h->d_rs.p), stride2};
    }
    if (!centred(in)) return MFCC_HIP_SUCCESS;
    const size_t stride3 = mfcc_center::dense_stride(n3, nch);
    if ((rc = ensure(h, h->d_ctr, nch * stride3 * sizeof(int16_t) + 64)) || (rc = scratch_acquire(h))) return rc;
    if (!mfcc_center::launch_dense(fmt, o.p, static_cast<int16_t *>(h->d_ctr.p), n2, n3, nch, o.stride, stride3,
                                   center_geom(h->r, in.center), h->n_cu, h->stream))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    HIP_TRY(h, hipGetLastError());
    o = DenseIn{static_cast<const int16_t *>(h->d_ctr.p), stride3};
    return MFCC_HIP_SUCCESS;
}

// The dense device entries: int16 at the handle's own rate goes straight to the kernels; anything else through the input
// stage first, and from there on as int16 at the handle's own rate
int dense_dev(mfcc_hip_handle *h, const Call &c, Samples in, const void *d_pcm, size_t n, size_t stride, size_t nch, int halo,
              void *d_out, size_t *n_frames) {
    auto route = [&](const void *p, size_t len, size_t st) {
        return c.fixed ? launch(h, c, p, len, st, nch, halo, d_out, n_frames)
                       : launch_float_dev(h, c, p, len, st, nch, halo, d_out, n_frames);
    };
    if (!decodes(in.fmt) && !in.rate && !centred(in)) return route(d_pcm, n, stride);
    // centring: the fixed-point framing is the RTL's, and a shard of a longer stream has no edges
    if (centred(in) && (c.fixed || halo == 1)) return MFCC_HIP_ERROR_UNSUPPORTED;
    // what launch() refuses, before anything is read
    if ((!d_pcm && n * nch) || halo < 0 || halo > 1 || !sample_aligned(in.fmt, d_pcm)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (nch > 1 && stride < n + size_t(halo)) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    mfcc_rs::Taps a{};
    size_t n2 = n;
    int rc;
    if (in.rate) {
        if (halo) return MFCC_HIP_ERROR_UNSUPPORTED;              // a shard's edge would need the neighbour's samples
        if (n >= mfcc_rs::kMaxLen) return MFCC_HIP_ERROR_INVALID_PARAM;
        if ((rc = rs_bind(h, in.rate, h->r.sample_rate, a))) return rc;
        n2 = size_t(mfcc_rs::count(n, a.L, a.M));
    }
    const size_t n3 = framed_len(h, in, n2);                     // the samples of a channel as the kernels frame them
    if (count_frames(h->r, n3) == 0 || nch == 0 || !d_out)       // no sample is read
        return route(d_pcm, n3, centred(in) ? mfcc_center::dense_stride(n3, nch) : in.rate ? rs_stride(n2, nch) : stride);
    DenseIn src;
    if ((rc = dense_input(h, in, d_pcm, n, stride, nch, halo, a, n2, n3, src)) || (rc = route(src.p, n3, src.stride))) return rc;
    return scratch_release(h);
}

// ---- host buffers in, host buffers out: the shape of the reference's own caller (software/main.c:100-177: file in,
// file out).  The input crosses PCIe at 340 B per frame, which is 25 times what the kernel needs per frame in time, so this
// path is a COPY pipeline: the batch is cut into chunks of ~64 MB (whole channels, or frame ranges of a long channel with
// a one-sample history halo), three chunks in flight -- H2D of chunk k + 1 on one copy stream, the kernel of chunk k on
// the handle's stream, D2H of chunk k - 1 on another.  An asynchronous copy from pageable memory blocks the calling thread
// until it is done (measured: hipMemcpyAsync of 154 MB returned after 8.6 ms); pinned in place with hipHostRegister (13 us
// per MB, done for chunk k + 1 while chunk k is on the wire) it returns in 20 us.  Round 2 ran copy, kernel, copy in series.
// Measured on 8 channels x 10 min (154 MB in, 23 MB out; tools/hostio_sweep.sh, median of 15): one chunk unpinned 3.42 ms,
// 64 MB chunks pinned 3.20 ms (0.141 G frames/s = 48 GB/s of input against 53 GB/s for the bare H2D copy), 32 MB 3.68,
// 16 MB 3.94 -- every chunk costs ~60 us of calls and a kernel launch that cannot fill the chip.  A batch that fits one
// chunk takes the plain blocking copies (pinning it first only adds its 13 us per MB in front).
using mfcc_batch::HostChunk;      // one chunk of a dense call (batch_plan.hpp: cut_dense)

// A caller's buffer pinned block by block for the duration of a call: page-aligned blocks of 16 MB, registered when a
// copy first touches them and released when every chunk that could touch them is done.  A copy must stay inside ONE
// registration (the runtime resolves a host pointer to the allocation it lies in and rejects a size that runs past it),
// so copies are split at block boundaries.
struct PinnedSpan {
    static constexpr size_t kBlock = size_t(16) << 20;
    char *base = nullptr;
    size_t nblocks = 0, total = 0;
    std::vector<char> state;      // 0: untouched, 1: pinned by us, 2: tried, not ours (already pinned or not pinnable)
    void init(const void *p, size_t bytes) {
        const uintptr_t page = 4096, a = reinterpret_cast<uintptr_t>(p) & ~(page - 1);
        const uintptr_t b = (reinterpret_cast<uintptr_t>(p) + bytes + page - 1) & ~(page - 1);
        base = reinterpret_cast<char *>(a);
        total = size_t(b - a);
        nblocks = (total + kBlock - 1) / kBlock;
        state.assign(nblocks, 0);
    }
    size_t block_bytes(size_t k) const { return std::min(kBlock, total - k * kBlock); }
    void ensure(const void *p, size_t bytes) {
        if (!bytes) return;
        const size_t k0 = size_t(static_cast<const char *>(p) - base) / kBlock;
        const size_t k1 = size_t(static_cast<const char *>(p) + bytes - 1 - base) / kBlock;
        for (size_t k = k0; k <= k1 && k < nblocks; ++k)
            if (!state[k]) {
                state[k] = hipHostRegister(base + k * kBlock, block_bytes(k), hipHostRegisterDefault) == hipSuccess ? 1 : 2;
                if (state[k] == 2) (void)hipGetLastError();
            }
    }
    // blocks that end at or below p are no longer needed
    void release_below(const void *p) {
        for (size_t k = 0; k < nblocks && base + k * kBlock + block_bytes(k) <= static_cast<const char *>(p); ++k)
            if (state[k] == 1) {
                (void)hipHostUnregister(base + k * kBlock);
                state[k] = 2;
            }
    }
    void release_all() {
        for (size_t k = 0; k < nblocks; ++k)
            if (state[k] == 1) {
                (void)hipHostUnregister(base + k * kBlock);
                state[k] = 2;
            }
    }
    // hipMemcpyAsync in pieces that do not cross a block boundary
    hipError_t copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st) const {
        const char *host = static_cast<const char *>(kind == hipMemcpyHostToDevice ? src : dst);
        size_t done = 0;
        while (done < bytes) {
            const size_t k = size_t(host + done - base) / kBlock;
            const size_t room = size_t(base + k * kBlock + block_bytes(k) - (host + done));
            const size_t len = std::min(bytes - done, room);
            const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + done, static_cast<const char *>(src) + done, len, kind, st);
            if (e != hipSuccess) return e;
            done += len;
        }
        return hipSuccess;
    }
};

// one chunk of a host-buffer call as the pipeline sees it: bytes in, bytes out
struct PipeChunk {
    const void *in;
    size_t in_bytes;
    void *out;
    size_t out_bytes;
};

// the pipeline itself: H2D of chunk i + 1 | enqueue(i, d_in, d_out) on the handle's stream | D2H of chunk i - 1.  The
// chunks must ascend in both host buffers ([in_lo, in_lo + in_total) and [out_lo, out_lo + out_total) are what gets pinned).
template <typename Enqueue>
int run_host_pipeline(mfcc_hip_handle *h, const std::vector<PipeChunk> &chunks, const void *in_lo, size_t in_total,
                      void *out_lo, size_t out_total, Enqueue &&enqueue) {
    constexpr int kPipe = mfcc_hip_handle::kPipe;
    const size_t nchunks = chunks.size();
    if (!nchunks) return MFCC_HIP_SUCCESS;
    bool no_pin = false;
    if (const char *e = std::getenv("MFCC_HIP_HOST_NOPIN")) no_pin = e[0] == '1';                  // diagnostic
    if (!h->s_in) HIP_TRY(h, hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
    if (!h->s_out) HIP_TRY(h, hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    size_t max_in = 0, max_out = 0;
    for (const PipeChunk &c : chunks) {
        max_in = std::max(max_in, c.in_bytes);
        max_out = std::max(max_out, c.out_bytes);
    }
    const int nbuf = int(std::min<size_t>(kPipe, nchunks));
    for (int i = 0; i < nbuf; ++i) {
        if (!h->ev_in[i]) {
            HIP_TRY(h, hipEventCreateWithFlags(&h->ev_in[i], hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(&h->ev_k[i], hipEventDisableTiming));
            HIP_TRY(h, hipEventCreateWithFlags(&h->ev_out[i], hipEventDisableTiming));
        }
        int rc = ensure(h, h->p_in[i], max_in + 64);
        if (rc) return rc;
        if ((rc = ensure(h, h->p_out[i], max_out + 64))) return rc;
    }
    // the copy streams start behind whatever is queued on the handle's stream
    HIP_TRY(h, hipEventRecord(h->ev_k[0], h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->s_in, h->ev_k[0], 0));

    // a batch that fits one chunk takes the plain blocking copies: pinning it first only adds its cost in front
    const bool pin_it = !no_pin && nchunks > 1;
    PinnedSpan pin_in, pin_out;
    pin_in.init(in_lo, in_total);
    pin_out.init(out_lo, out_total);
    if (!pin_it) {
        pin_in.state.assign(pin_in.nblocks, 2);
        pin_out.state.assign(pin_out.nblocks, 2);
    }
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(h->s_in);
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->s_out);
        pin_in.release_all();
        pin_out.release_all();
        return code;
    };
    // what lies below the next unfinished chunk is released as the pipeline moves on, what lies ahead is pinned one chunk
    // early (on the CPU, while the wire is busy)
    auto pin = [&](size_t i) {
        pin_in.ensure(chunks[i].in, chunks[i].in_bytes);
        pin_out.ensure(chunks[i].out, chunks[i].out_bytes);
    };
    pin(0);
#define PIPE_TRY(expr)                                   \
    do {                                                 \
        const hipError_t e__ = (expr);                   \
        if (e__ != hipSuccess) {                         \
            h->last_hip = int(e__);                      \
            return fail(MFCC_HIP_ERROR_OTHER);           \
        }                                                \
    } while (0)
    for (size_t i = 0; i < nchunks; ++i) {
        const PipeChunk &c = chunks[i];
        const int slot = int(i % kPipe);
        if (i + 1 < nchunks) pin(i + 1);
        if (i >= size_t(kPipe)) {
            // slot reuse: chunk i - kPipe's kernel has read p_in[slot] / its rows have left p_out[slot]
            PIPE_TRY(hipStreamWaitEvent(h->s_in, h->ev_k[slot], 0));
            PIPE_TRY(hipStreamWaitEvent(h->stream, h->ev_out[slot], 0));
            PIPE_TRY(hipEventSynchronize(h->ev_out[slot]));
            // chunks 0 .. i - kPipe are done (copies, kernel, rows): nothing touches what lies below the next one
            pin_in.release_below(chunks[i - kPipe + 1].in);
            pin_out.release_below(chunks[i - kPipe + 1].out);
        }
        if (c.in_bytes) PIPE_TRY(pin_in.copy(h->p_in[slot].p, c.in, c.in_bytes, hipMemcpyHostToDevice, h->s_in));
        PIPE_TRY(hipEventRecord(h->ev_in[slot], h->s_in));
        PIPE_TRY(hipStreamWaitEvent(h->stream, h->ev_in[slot], 0));
        const int rc = enqueue(i, h->p_in[slot].p, h->p_out[slot].p);
        if (rc) return fail(rc);
        PIPE_TRY(hipEventRecord(h->ev_k[slot], h->stream));
        PIPE_TRY(hipStreamWaitEvent(h->s_out, h->ev_k[slot], 0));
        if (c.out_bytes) PIPE_TRY(pin_out.copy(c.out, h->p_out[slot].p, c.out_bytes, hipMemcpyDeviceToHost, h->s_out));
        PIPE_TRY(hipEventRecord(h->ev_out[slot], h->s_out));
    }
    PIPE_TRY(hipStreamSynchronize(h->s_out));
#undef PIPE_TRY
    // the handle's stream continues behind the last rows
    (void)hipStreamWaitEvent(h->stream, h->ev_out[int((nchunks - 1) % kPipe)], 0);
    pin_in.release_all();
    pin_out.release_all();
    return MFCC_HIP_SUCCESS;
}

inline size_t host_chunk_bytes() {
    size_t b = size_t(64) << 20;
    if (const char *e = std::getenv("MFCC_HIP_HOST_CHUNK_MB")) b = size_t(std::atoi(e) > 0 ? std::atoi(e) : 64) << 20;   // diagnostic
    return b;
}

template <typename OutT>
int process_host(mfcc_hip_handle *h, const Call &c, Samples in, const void *pcm, size_t n, size_t nch, OutT *out,
                 size_t cap, size_t *n_frames) {
    const bool fixed = c.fixed;
    if (!pcm && n * nch) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (fixed && (h->fixed_kernel == FixedKernel::kNone || centred(in))) return MFCC_HIP_ERROR_UNSUPPORTED;
    size_t n2 = n;                              // samples of a channel at the handle's own rate
    if (in.rate) {
        mfcc_rs::Geometry g;
        const int rc = rs_geometry(in.rate, h->r.sample_rate, g);
        if (rc) return rc;
        if (n >= mfcc_rs::kMaxLen) return MFCC_HIP_ERROR_INVALID_PARAM;
        n2 = size_t(mfcc_rs::count(n, g.L, g.M));
    }
    const size_t nf = count_frames(h->r, framed_len(h, in, n2));
    if (n_frames) *n_frames = nf;
    if (nf == 0 || nch == 0) return MFCC_HIP_SUCCESS;
    const size_t ncep = c.out_width;            // elements per row
    const size_t n_out = nf * nch * ncep;
    if (!out || cap < n_out) return MFCC_HIP_ERROR_BUFFER_SMALL;
    DeviceGuard guard(h->device);
    const size_t ssz = sample_bytes(in.fmt);
    if (in.rate || centred(in)) {
        // an input rate, centring: the unchunked route -- one copy in, the device route, one copy back
        int rc;
        if ((rc = ensure(h, h->d_raw, n * nch * ssz + 64)) || (rc = ensure(h, h->d_full, n_out * sizeof(OutT) + 64)) ||
            (rc = scratch_acquire(h)))
            return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_raw.p, pcm, n * nch * ssz, hipMemcpyHostToDevice, h->stream));
        if ((rc = dense_dev(h, c, in, h->d_raw.p, n, n, nch, 0, h->d_full.p, nullptr))) return rc;
        HIP_TRY(h, hipMemcpyAsync(out, h->d_full.p, n_out * sizeof(OutT), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MFCC_HIP_SUCCESS;
    }
    const size_t kChunkBytes = host_chunk_bytes();
    // deltas: the static rows are 1 + K times narrower than the output rows
    const int K = c.post.delta_order;
    // a sample format: the chunks are cut by sample count exactly as for int16, their raw bytes cross the wire and every
    // chunk is decoded on the device in front of its kernel
    const bool dec = decodes(in.fmt);

    const std::vector<HostChunk> chunks = mfcc_batch::cut_dense(n, nch, nf, ncep, framing(h->r), kChunkBytes);
    // The chain (post_chain) works on whole channels: no row may leave the device before its channel's statistics exist,
    // deltas need the neighbouring frames and PCEN is recursive along the channel -- a chunk edge is not a channel edge.
    // Chunks of whole channels run the chain on their own rows before the copy back; frame-range chunks of long channels
    // write into one device buffer of the whole result (and its staging), which goes through the chain and is copied
    // back after the pipeline
    const bool post = has_post(c.post);
    const bool whole = post && mfcc_batch::dense_cuts_channels(n, kChunkBytes);
    OutT *d_full = nullptr;
    if (whole) {
        const int rc = ensure(h, h->d_full, n_out * sizeof(OutT) + 64);
        if (rc) return rc;
        d_full = static_cast<OutT *>(h->d_full.p);
    }
    // the staging of the chain (route_to's rule) holds the rows of one chunk, or of the whole result
    const bool staged = post && (K || sliding(c.post));
    if (staged) {
        int rc = stage_rows(h, c, whole ? nch * nf : mfcc_batch::max_chunk_rows(chunks));
        if (rc || (rc = scratch_acquire(h))) return rc;
    }
    std::vector<PipeChunk> pc;
    pc.reserve(chunks.size());
    for (const HostChunk &k : chunks)
        pc.push_back({sample_at(in.fmt, pcm, k.in_off), k.in_samples * ssz, out + k.out_off,
                      whole ? 0 : k.out_elems * sizeof(OutT)});
    int rc = run_host_pipeline(h, pc, pcm, nch * n * ssz, out, whole ? 0 : n_out * sizeof(OutT), [&](size_t i, void *d_raw, void *d_out) {
        const HostChunk &k = chunks[i];
        DenseIn src{static_cast<const int16_t *>(d_raw), k.stride};
        int crc;
        if (dec && (crc = dense_input(h, in, d_raw, k.n, k.stride, k.nch, k.halo, mfcc_rs::Taps{}, k.n, k.n, src))) return crc;
        void *rows = whole ? static_cast<void *>(d_full + k.out_off) : d_out;
        PostRoute rt{};
        if (post) {
            // a frame-range chunk writes its rows of the whole result, W wide where they are statics
            rt = route_to(h, c.post, static_cast<float *>(rows), whole ? k.out_off / size_t(1 + K) : 0);
            rows = rt.raw;
        }
        crc = launch(h, c, src.p, k.n, src.stride, k.nch, k.halo, rows, nullptr, k.halo || k.frames != nf ? k.frames : 0);
        if (crc || whole || !post) return crc;
        return post_chain(h, c, span_uniform(0, k.nch, nf), rt, nullptr);
    });
    if (rc || !whole) return rc ? rc : (staged || dec ? scratch_release(h) : MFCC_HIP_SUCCESS);
    if ((rc = post_chain(h, c, span_uniform(0, nch, nf), route_to(h, c.post, reinterpret_cast<float *>(d_full)), nullptr))) return rc;
    if ((staged || dec) && (rc = scratch_release(h))) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, d_full, n_out * sizeof(OutT), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MFCC_HIP_SUCCESS;
}

// ---- ragged batch: many utterances of different lengths, one launch.
// The utterances are packed into ONE stream at offsets that are multiples of the hop, separated by
// zeros: at least one zero in front (pre-emphasis history 0, like after the driver's soft reset,
// main.c:21-34) and zeros behind up to the end of the last frame (the zero-padded tail of main.c:134-144).
// Frame k of utterance u is then frame start_u / hop + k of the packed stream -- the same samples, the
// same arithmetic, bit for bit -- and the frames that fall into the gaps are simply not copied out.
template <typename OutT>
__global__ void gather_rows_kernel(const OutT *__restrict__ src, OutT *__restrict__ dst,
                                   const long long *__restrict__ desc, long long n_utt, int row) {
    for (long long u = blockIdx.x; u < n_utt; u += gridDim.x) {
        const long long s0 = desc[3 * u] * row, d0 = desc[3 * u + 1] * row, n = desc[3 * u + 2] * row;
        for (long long i = threadIdx.x; i < n; i += blockDim.x) dst[d0 + i] = src[s0 + i];
    }
}

// device-resident input: copy every utterance to its place in the packed stream and zero what lies between it and
// the next one (no memset of the whole stream: every sample of it is written exactly once).  16 bytes per lane:
// the destination is brought to 16-byte alignment first, the source is read as it lies (2-byte aligned; global
// memory takes unaligned vector loads)
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(2))) Unaligned16 {
    u32x4_t v;
};

__global__ void pack_utterances_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst,
                                       const long long *__restrict__ desc, long long n_utt) {
    // desc: (source offset, destination offset, samples, end of this utterance's part of the stream) per utterance
    for (long long u = blockIdx.x; u < n_utt; u += gridDim.x) {
        const long long n = desc[4 * u + 2], span = desc[4 * u + 3] - desc[4 * u + 1];
        if (span <= 0) continue;
        const int16_t *s0 = src + desc[4 * u];
        int16_t *d0 = dst + desc[4 * u + 1];
        long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(d0) & 15)) & 15) >> 1);
        if (head > n) head = n;
        for (long long i = threadIdx.x; i < head; i += blockDim.x) d0[i] = s0[i];
        const long long nvec = (n - head) >> 3;
        u32x4_t *dv = reinterpret_cast<u32x4_t *>(d0 + head);
        const Unaligned16 *sv = reinterpret_cast<const Unaligned16 *>(s0 + head);
        for (long long v = threadIdx.x; v < nvec; v += blockDim.x) dv[v] = sv[v].v;
        for (long long i = head + 8 * nvec + threadIdx.x; i < span; i += blockDim.x) d0[i] = i < n ? s0[i] : int16_t(0);
    }
}

// The fused 512 kernel's tiles, for the scan and the tile records (batch_plan.hpp does not include a kernel header)
constexpr mfcc_batch::TileGeom kRaggedTiles = {mfcc_fused::kTile, mfcc_fused::kTileHop, mfcc_fused::kSUsed};

inline mfcc_batch::Scan ragged_scan(const mfcc_hip_handle *h, const size_t *offsets, size_t n_utt, size_t *frame_offsets) {
    return mfcc_batch::scan(offsets, n_utt, framing(h->r), size_t(kRaggedTiles.tile), frame_offsets);
}

// The launch of a scanned corpus with at least one frame, d_out large enough: route -> fill -> desc_stage -> launch
// (batch_plan.hpp).  d_pcm is int16; fo: the scan's frame offsets
template <typename OutT>
int ragged_launch(mfcc_hip_handle *h, const Call &c, const int16_t *d_pcm, const size_t *offsets, size_t n_utt, OutT *d_out,
                  const size_t *fo, const mfcc_batch::Scan &sc) {
    using mfcc_batch::Records;
    using mfcc_batch::Route;
    const bool fixed = c.fixed;
    Records kernel = Records::kNone;        // what the kernel of this call reads utterances from
    if (!fixed && c.kind == Kind::kFeatures && h->float_kernel == FloatKernel::kFused512W12 && std::is_same<OutT, float>::value)
        kernel = Records::kTiles;                 // (a spectrum or filterbank call packs: its kernels take no tile records)
    if (fixed && h->fixed_kernel == FixedKernel::kFixed512 && std::is_same<OutT, int16_t>::value) kernel = Records::kFrames;
    const Route route = mfcc_batch::route(kernel, fixed, sc, n_utt);
    // Checked first: this is the per-step host work of a sharded corpus (BASELINE config 5: 10 000 x 10 s; bench.py
    // `enqueue_us_per_step`) -- no packing copy, no row gather, no descriptors, the same bits (every channel of the
    // plain call starts from reset, its frames are the utterance's frames and the rows come out dense)
    if (route == Route::kUniform) return launch(h, c, d_pcm + offsets[0], sc.len0, sc.len0, n_utt, 0, d_out, nullptr);
    // the table in pinned memory: its H2D copy is asynchronous
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    int rc = desc_acquire(h, mfcc_batch::table_ll(route, n_utt), &pd);
    if (rc) return rc;
    if (route == Route::kTileRecords) {
        // no packed copy at all: the kernel reads every utterance where it lies and writes its rows where they belong
        // (kernel_fused512_w12.hpp)
        const mfcc_batch::TilePlan p =
            mfcc_batch::fill_chans(offsets, fo, n_utt, kRaggedTiles, reinterpret_cast<mfcc_fused12::RaggedChan *>(pd->p));
        if ((rc = desc_stage(h, h->d_in, p.bytes, pd, p.chan_ll))) return rc;
        auto *d_chans = static_cast<const mfcc_fused12::RaggedChan *>(h->d_in.p);
        auto *d_map = reinterpret_cast<mfcc_fused12::RaggedTile *>(static_cast<char *>(h->d_in.p) + p.map_off);
        const bool launched =
            is_logmel(h->r) ? mfcc_fused12::launch_ragged<true>(d_pcm, d_chans, (int)n_utt, d_map, (int)p.n_tiles, h->fu,
                                                                h->fused_dense, reinterpret_cast<float *>(d_out), h->n_cu, h->stream)
                            : mfcc_fused12::launch_ragged(d_pcm, d_chans, (int)n_utt, d_map, (int)p.n_tiles, h->fu,
                                                          h->fused_dense, reinterpret_cast<float *>(d_out), h->n_cu, h->stream);
        if (!launched) return MFCC_HIP_ERROR_OTHER;               // cannot happen with at least one tile
    } else if (route == Route::kFrameRecords) {
        // the same: the kernel's waves walk consecutive frames and step from one utterance into the next
        // (kernel_fixed512.hpp)
        const mfcc_batch::RecPlan p =
            mfcc_batch::fill_recs(offsets, fo, n_utt, reinterpret_cast<mfcc_fixed512::RaggedRec *>(pd->p));
        if ((rc = desc_stage(h, h->d_in, p.bytes, pd, p.rec_ll))) return rc;
        mfcc_fixed512::launch_ragged(d_pcm, static_cast<const mfcc_fixed512::RaggedRec *>(h->d_in.p), (int)p.n_recs,
                                     (long long)sc.total, h->r.hop, h->x5, reinterpret_cast<int16_t *>(d_out), h->n_cu, h->stream);
    } else {
        const size_t ncep = c.width;
        const mfcc_batch::PackPlan p = mfcc_batch::fill_pack(offsets, fo, n_utt, framing(h->r), ncep * sizeof(OutT), pd->p);
        if ((rc = ensure(h, h->d_in, p.in_bytes))) return rc;
        if ((rc = desc_stage(h, h->d_out, p.out_bytes, pd, p.desc_ll, p.desc_off))) return rc;
        OutT *d_all = static_cast<OutT *>(h->d_out.p);
        long long *d_desc = reinterpret_cast<long long *>(static_cast<char *>(h->d_out.p) + p.desc_off);
        const unsigned blocks = (unsigned)std::min<size_t>(n_utt, size_t(h->n_cu) * 8);
        hipLaunchKernelGGL(pack_utterances_kernel, dim3(blocks), dim3(256), 0, h->stream, d_pcm,
                           static_cast<int16_t *>(h->d_in.p), d_desc, (long long)n_utt);
        if ((rc = launch(h, c, h->d_in.p, p.len, p.len, 1, 0, d_all, nullptr, p.F))) return rc;
        hipLaunchKernelGGL(gather_rows_kernel<OutT>, dim3(blocks), dim3(256), 0, h->stream, d_all, d_out,
                           d_desc + p.gather_ll, (long long)n_utt, (int)ncep);
    }
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

// the offsets of the resampled utterances, back to back from 0.  false: decreasing offsets or a length over the limit
bool rated_offsets(const mfcc_rs::Geometry &g, const size_t *offsets, size_t n_utt, std::vector<size_t> &off2) {
    off2.assign(n_utt + 1, 0);
    for (size_t u = 0; u < n_utt; ++u) {
        if (offsets[u + 1] < offsets[u] || offsets[u + 1] - offsets[u] >= mfcc_rs::kMaxLen) return false;
        off2[u + 1] = off2[u] + size_t(mfcc_rs::count(offsets[u + 1] - offsets[u], g.L, g.M));
    }
    return true;
}

// the offsets of the centred utterances (center_plan.hpp: fill_table): they abut from 0, F = 0 takes no room.  false:
// decreasing offsets
bool centred_offsets(const mfcc_hip_handle *h, int mode, const size_t *own, size_t n_utt, std::vector<size_t> &off3) {
    off3.assign(n_utt + 1, 0);
    for (size_t u = 0; u < n_utt; ++u)
        if (own[u + 1] < own[u]) return false;
    mfcc_center::fill_table(center_geom(h->r, mode), own, n_utt, 0, off3.data(), nullptr);
    return true;
}

// ---- the input stage of a ragged call (DESIGN.md sections 4.15, 4.17, 4.21): the utterances at `offsets` of d_pcm, as `in`
// describes them -> int16 utterances at the handle's own rate.  The span offsets[0] .. offsets[n_utt] is decoded into
// h->d_dec; every utterance is then resampled on its own (zeros outside it) by one launch over a tile list into h->d_rs, at
// `own` (rated_offsets); every utterance is then centred on its own by one launch over a record list into h->d_ctr, at
// `ctr` (centred_offsets; NULL where the call is not centred).  The centring kernel decodes while it pads, so a centred
// call without a rate runs no decode pass.  p / offsets: where the utterances now lie.  scratch: the area is taken, the
// caller releases it behind the kernels that read them (plain int16 at the handle's own rate: nothing is done or taken)
struct RaggedIn {
    const int16_t *p;
    const size_t *offsets;
    bool scratch;
    std::vector<size_t> loc;                // the offsets of a decoded span, from its start
};

// the centring of a ragged call: the utterances at src_off of d_src, in format fmt -> h->d_ctr at ctr, one launch.  d_ctr:
// the samples, then the records
int ragged_center(mfcc_hip_handle *h, int mode, int fmt, const void *d_src, const size_t *src_off, const size_t *ctr,
                  size_t n_utt) {
    const mfcc_center::Geom g = center_geom(h->r, mode);
    const size_t rec_off = (ctr[n_utt] * sizeof(int16_t) + 255) & ~size_t(255), rec_ll = n_utt * mfcc_center::kRecLL;
    int rc;
    if ((rc = ensure(h, h->d_ctr, rec_off + rec_ll * sizeof(long long) + 64))) return rc;
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    if ((rc = desc_acquire(h, rec_ll, &pd))) return rc;
    std::vector<size_t> off3(n_utt + 1);
    const mfcc_center::Table t = mfcc_center::fill_table(g, src_off, n_utt, 0, off3.data(), pd->p);
    if ((rc = desc_stage(h, h->d_ctr, 0, pd, rec_ll, rec_off))) return rc;
    if (!t.total) return MFCC_HIP_SUCCESS;
    if (!mfcc_center::launch_ragged(fmt, d_src, static_cast<int16_t *>(h->d_ctr.p),
                                    reinterpret_cast<const long long *>(static_cast<const char *>(h->d_ctr.p) + rec_off), n_utt,
                                    t.max_padded, g, h->n_cu, h->stream))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

int ragged_input(mfcc_hip_handle *h, Samples in, const void *d_pcm, const size_t *offsets, const size_t *own, const size_t *ctr,
                 size_t n_utt, RaggedIn &o) {
    o.p = static_cast<const int16_t *>(d_pcm);
    o.offsets = offsets;
    o.scratch = decodes(in.fmt) || in.rate || centred(in);
    if (!o.scratch) return MFCC_HIP_SUCCESS;
    int rc;
    if (centred(in) && !in.rate) {
        // one pass: the kernel reads the caller's samples where they lie and decodes them while it pads
        if ((rc = ragged_center(h, in.center, in.fmt, d_pcm, offsets, ctr, n_utt))) return rc;
        o.p = static_cast<const int16_t *>(h->d_ctr.p);
        o.offsets = ctr;
        return MFCC_HIP_SUCCESS;
    }
    mfcc_rs::Taps a;
    if (in.rate && (rc = rs_bind(h, in.rate, h->r.sample_rate, a))) return rc;
    const int16_t *src = o.p + offsets[0];
    if (decodes(in.fmt)) {
        size_t st = 0;
        const size_t span = offsets[n_utt] - offsets[0];
        if ((rc = decode_to_scratch(h, in.fmt, sample_at(in.fmt, d_pcm, offsets[0]), span, 1, span, &src, &st))) return rc;
    }
    if (!in.rate) {
        o.loc.resize(n_utt + 1);
        for (size_t u = 0; u <= n_utt; ++u) o.loc[u] = offsets[u] - offsets[0];
        o.p = src;
        o.offsets = o.loc.data();
        return MFCC_HIP_SUCCESS;
    }
    // d_rs: the samples, then the records (their count does not depend on where the samples lie: 7 slots of lead at most)
    size_t max_tiles = 0;
    for (size_t u = 0; u < n_utt; ++u) max_tiles += mfcc_rs::max_tiles(own[u + 1] - own[u], false);
    const size_t rec_off = (own[n_utt] * sizeof(int16_t) + 255) & ~size_t(255);
    const size_t rec_cap_ll = n_utt * mfcc_rs::kSegLL + max_tiles * mfcc_rs::kTileLL;
    if ((rc = ensure(h, h->d_rs, rec_off + rec_cap_ll * sizeof(long long) + 64))) return rc;
    int16_t *d_rs = static_cast<int16_t *>(h->d_rs.p);
    std::vector<mfcc_rs::SegIn> segs(n_utt);
    for (size_t u = 0; u < n_utt; ++u)
        segs[u] = mfcc_rs::one_shot(h->rs_geom, reinterpret_cast<uintptr_t>(src + (offsets[u] - offsets[0])),
                                    offsets[u + 1] - offsets[u], reinterpret_cast<uintptr_t>(d_rs + own[u]));
    mfcc_rs::CallPlan pl;
    if (!mfcc_rs::plan_call(segs.data(), n_utt, pl) || pl.total_ll > rec_cap_ll) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    if ((rc = desc_acquire(h, pl.total_ll, &pd))) return rc;
    mfcc_rs::fill_call(segs.data(), n_utt, pl, pd->p);
    if ((rc = desc_stage(h, h->d_rs, 0, pd, pl.total_ll, rec_off))) return rc;
    if (pl.n_tiles) {
        mfcc_rs::launch(a, nullptr, 0, nullptr, 0, (long long)n_utt, 0, 0,
                        reinterpret_cast<const long long *>(reinterpret_cast<const char *>(d_rs) + rec_off), (long long)pl.n_tiles,
                        h->n_cu, h->stream);
        HIP_TRY(h, hipGetLastError());
    }
    o.p = d_rs;
    o.offsets = own;
    if (!centred(in)) return MFCC_HIP_SUCCESS;
    if ((rc = ragged_center(h, in.center, MFCC_HIP_SAMPLE_S16, d_rs, own, ctr, n_utt))) return rc;
    o.p = static_cast<const int16_t *>(h->d_ctr.p);
    o.offsets = ctr;
    return MFCC_HIP_SUCCESS;
}

// A scanned corpus on the device, as `in` describes it (own: the offsets at the handle's own rate -- `offsets` itself
// without an input rate; ctr: those of the centred utterances, NULL where the call is not centred; sc has scanned the last
// of the three that exists): what is left to refuse, the input stage, the launch, and the chain over the
// result, one segment per utterance.  A call that stages (deltas, a normalization window, MFCC_HIP_VAD_SELECT) has its
// kernels write into the staging.  With MFCC_HIP_VAD_SELECT every frame goes through the chain into h->d_final, then only
// the voiced rows to d_out; frame_offsets describes those, and the call synchronizes (select_run)
template <typename OutT>
int ragged_scanned(mfcc_hip_handle *h, const Call &c, Samples in, const void *d_pcm, const size_t *offsets, const size_t *own,
                   const size_t *ctr, size_t n_utt, OutT *d_out, size_t cap, size_t *frame_offsets, const mfcc_batch::Scan &sc) {
    if (c.fixed && h->fixed_kernel == FixedKernel::kNone) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (sc.max_len && !d_pcm) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (sc.total == 0) return MFCC_HIP_SUCCESS;
    const bool post = has_post(c.post), sel = c.post.vad_mode != MFCC_HIP_VAD_OFF;
    const size_t WO = c.out_width;
    if (!d_out || cap < sc.total * WO) return MFCC_HIP_ERROR_BUFFER_SMALL;    // frame_offsets: the counts, to size d_out by
    DeviceGuard guard(h->device);
    RaggedIn src;
    int rc = ragged_input(h, in, d_pcm, offsets, own, ctr, n_utt, src);
    if (rc) return rc;
    if (!post) {
        rc = ragged_launch<OutT>(h, c, src.p, src.offsets, n_utt, d_out, frame_offsets, sc);
    } else {
        PostRoute rt;
        if ((rc = post_route(h, c, sc.total, reinterpret_cast<float *>(d_out), sel, rt)) ||
            (rc = ragged_launch<float>(h, c, src.p, src.offsets, n_utt, rt.raw, frame_offsets, sc)))
            return rc;
        const SegSpan sp = span_offsets(frame_offsets, n_utt);
        SelPlan pl;
        if (sel && (rc = select_plan(h, sp, int(WO), pl))) return rc;
        if ((rc = post_chain(h, c, sp, rt, sel ? &pl : nullptr))) return rc;
        if (sel) rc = select_run(h, rt.out, int(WO), rt.voiced, pl, true, reinterpret_cast<float *>(d_out), frame_offsets);
        else if (rt.staged) rc = scratch_release(h);
    }
    return rc || !src.scratch ? rc : scratch_release(h);
}

// the device entry: the one scan of the call, then the above.  The order of the refusals is the entry's own: a sample format
// looks at the offsets and the pointer before the fixed-point kernel, an input rate after it
template <typename OutT>
int process_ragged_dev(mfcc_hip_handle *h, const Call &c, Samples in, const void *d_pcm, const size_t *offsets, size_t n_utt,
                       OutT *d_out, size_t cap, size_t *frame_offsets) {
    if (!offsets || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (centred(in) && c.fixed) return MFCC_HIP_ERROR_UNSUPPORTED;          // the fixed-point framing is the RTL's
    const bool dec = decodes(in.fmt) && n_utt;
    if ((!dec || in.rate) && c.fixed && h->fixed_kernel == FixedKernel::kNone) return MFCC_HIP_ERROR_UNSUPPORTED;
    std::vector<size_t> off2, off3;
    if (in.rate) {
        mfcc_rs::Geometry g;
        const int rc = rs_geometry(in.rate, h->r.sample_rate, g);
        if (rc) return rc;
        if (!rated_offsets(g, offsets, n_utt, off2) || !sample_aligned(in.fmt, d_pcm)) return MFCC_HIP_ERROR_INVALID_PARAM;
    }
    const size_t *own = in.rate ? off2.data() : offsets;
    if (centred(in) && !centred_offsets(h, in.center, own, n_utt, off3)) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t *ctr = centred(in) ? off3.data() : nullptr;
    const mfcc_batch::Scan sc = ragged_scan(h, ctr ? ctr : own, n_utt, frame_offsets);
    if (sc.rc || (dec && !sample_aligned(in.fmt, d_pcm))) return MFCC_HIP_ERROR_INVALID_PARAM;
    return ragged_scanned<OutT>(h, c, in, d_pcm, offsets, own, ctr, n_utt, d_out, cap, frame_offsets, sc);
}

// Host buffers: the corpus goes to the device in ONE copy (the span offsets[0] .. offsets[n_utt] as it lies), runs through
// the device-resident path above -- no copy at all for equal lengths, per-tile / per-utterance records for the fused
// kernels, pack and gather for the rest -- and its rows come back in one copy.  (Round 1 copied utterance by
// utterance into a zeroed packed stream: n_utt memcpy calls, 50 ms of call overhead for 10 000 utterances.)
template <typename OutT>
int process_ragged(mfcc_hip_handle *h, const Call &c, Samples in, const void *pcm, const size_t *offsets, size_t n_utt,
                   OutT *out, size_t cap, size_t *frame_offsets) {
    const bool fixed = c.fixed;
    if (!offsets || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (fixed && (h->fixed_kernel == FixedKernel::kNone || centred(in))) return MFCC_HIP_ERROR_UNSUPPORTED;
    const size_t ncep = c.out_width;                                     // elements per row
    std::vector<size_t> off2, off3;                                      // an input rate: the offsets at the handle's own;
                                                                         // centring: those of the padded utterances
    if (in.rate) {
        mfcc_rs::Geometry g;
        const int rc = rs_geometry(in.rate, h->r.sample_rate, g);
        if (rc) return rc;
        if (!rated_offsets(g, offsets, n_utt, off2)) return MFCC_HIP_ERROR_INVALID_PARAM;
    }
    if (centred(in) && !centred_offsets(h, in.center, in.rate ? off2.data() : offsets, n_utt, off3))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    const mfcc_batch::Scan sc = ragged_scan(h, centred(in) ? off3.data() : in.rate ? off2.data() : offsets, n_utt, frame_offsets);
    if (sc.rc || (sc.max_len && !pcm)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (sc.total == 0) return MFCC_HIP_SUCCESS;                          // frame_offsets: all zero
    if (!out || cap < sc.total * ncep) return MFCC_HIP_ERROR_BUFFER_SMALL;      // the counts, so that the caller can size `out`
    DeviceGuard guard(h->device);
    const size_t ssz = sample_bytes(in.fmt);
    std::vector<size_t> loc, fo;
    if (in.rate || centred(in)) {
        // an input rate, centring: the unchunked route -- one copy in, the device route, one copy back
        loc.resize(n_utt + 1);
        for (size_t u = 0; u <= n_utt; ++u) loc[u] = offsets[u] - offsets[0];
        const size_t in_bytes = loc[n_utt] * ssz, n_out = sc.total * ncep;
        int rc;
        if ((rc = ensure(h, h->d_raw, in_bytes + 64)) || (rc = ensure(h, h->d_full, n_out * sizeof(OutT) + 64)) ||
            (rc = scratch_acquire(h)))
            return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_raw.p, sample_at(in.fmt, pcm, offsets[0]), in_bytes, hipMemcpyHostToDevice, h->stream));
        if ((rc = ragged_scanned<OutT>(h, c, in, h->d_raw.p, loc.data(), in.rate ? off2.data() : loc.data(),
                                       centred(in) ? off3.data() : nullptr, n_utt, static_cast<OutT *>(h->d_full.p), n_out,
                                       frame_offsets, sc)))
            return rc;
        // MFCC_HIP_VAD_SELECT: frame_offsets now counts the voiced rows (the call above has synchronized)
        HIP_TRY(h, hipMemcpyAsync(out, h->d_full.p, frame_offsets[n_utt] * ncep * sizeof(OutT), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MFCC_HIP_SUCCESS;
    }
    // the same copy pipeline as process_host: chunks of whole utterances, ~64 MB each; every chunk is one call of the
    // device-resident ragged path on its own offsets, its rows land behind those of the chunk before it.  A sample format:
    // the chunks are cut by sample count as for int16, their raw bytes cross the wire and the ragged path decodes them
    const std::vector<mfcc_batch::UttRange> ranges =
        mfcc_batch::cut_ragged(offsets, frame_offsets, n_utt, host_chunk_bytes());
    std::vector<PipeChunk> pc;
    pc.reserve(ranges.size());
    for (const mfcc_batch::UttRange &r : ranges)
        pc.push_back({sample_at(in.fmt, pcm, offsets[r.u0]), (offsets[r.u1] - offsets[r.u0]) * ssz, out + r.rows0 * ncep,
                      (r.rows1 - r.rows0) * ncep * sizeof(OutT)});
    // the frame counts of the scan, chunk by chunk (a chunk's call does not count them again)
    const std::vector<size_t> counts(frame_offsets, frame_offsets + n_utt + 1);
    // MFCC_HIP_VAD_SELECT: every chunk returns its voiced rows only (the call below synchronizes and reports them), so its
    // copy back shrinks and lands behind the voiced rows of the chunks before it
    const bool sel_mode = c.post.vad_mode;
    size_t sel_rows = 0;
    return run_host_pipeline(h, pc, sample_at(in.fmt, pcm, offsets[0]), (offsets[n_utt] - offsets[0]) * ssz, out,
                             sc.total * ncep * sizeof(OutT), [&](size_t i, void *d_in, void *d_out) {
        const mfcc_batch::UttRange &r = ranges[i];
        const size_t k = r.u1 - r.u0;
        loc.assign(k + 1, 0);
        fo.assign(k + 1, 0);
        for (size_t j = 0; j <= k; ++j) loc[j] = offsets[r.u0 + j] - offsets[r.u0];
        const mfcc_batch::Scan csc =
            mfcc_batch::scan_with(loc.data(), k, size_t(kRaggedTiles.tile),
                                  [&](size_t u, size_t) { return counts[r.u0 + u + 1] - counts[r.u0 + u]; }, fo.data());
        const int rc = ragged_scanned<OutT>(h, c, in, d_in, loc.data(), loc.data(), nullptr, k, static_cast<OutT *>(d_out),
                                            pc[i].out_bytes / sizeof(OutT), fo.data(), csc);
        const size_t rows0 = sel_mode ? sel_rows : r.rows0;
        for (size_t j = 1; j <= k; ++j) frame_offsets[r.u0 + j] = rows0 + fo[j];
        if (sel_mode && !rc) {
            pc[i].out = out + rows0 * ncep;
            pc[i].out_bytes = fo[k] * ncep * sizeof(OutT);
            sel_rows += fo[k];
        }
        return rc;
    });
}

// ---- minimal RIFF/WAVE reader (the reference uses the un-vendored libwav, main.c:58-98)
int read_wav_i16(const char *path, int want_rate, std::vector<int16_t> &pcm) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return MFCC_HIP_ERROR_IO;
    std::vector<unsigned char> d;
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    std::fclose(f);
    auto u32 = [&](size_t o) { return uint32_t(d[o]) | uint32_t(d[o + 1]) << 8 | uint32_t(d[o + 2]) << 16 | uint32_t(d[o + 3]) << 24; };
    auto u16 = [&](size_t o) { return uint16_t(d[o] | d[o + 1] << 8); };
    if (d.size() < 12 || std::memcmp(d.data(), "RIFF", 4) || std::memcmp(d.data() + 8, "WAVE", 4))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    size_t o = 12;
    int fmt = 0, ch = 0, bits = 0;
    uint32_t rate = 0;
    bool have_fmt = false;
    while (o + 8 <= d.size()) {
        uint32_t sz = u32(o + 4);
        size_t body = o + 8;
        if (!std::memcmp(d.data() + o, "fmt ", 4) && body + 16 <= d.size()) {
            fmt = u16(body); ch = u16(body + 2); rate = u32(body + 4); bits = u16(body + 14);
            have_fmt = true;
        } else if (!std::memcmp(d.data() + o, "data", 4)) {
            // same checks as mfcc_wav_open (software/main.c:72-92): PCM, 16 bit, expected rate
            if (!have_fmt || fmt != 1 || bits != 16 || ch != 1 || int(rate) != want_rate)
                return MFCC_HIP_ERROR_UNSUPPORTED;
            size_t avail = d.size() - body;
            size_t n = (sz < avail ? sz : avail) / 2;
            pcm.resize(n);
            for (size_t i = 0; i < n; ++i) pcm[i] = int16_t(u16(body + 2 * i));
            return MFCC_HIP_SUCCESS;
        }
        o = body + sz + (sz & 1);
    }
    return MFCC_HIP_ERROR_INVALID_PARAM;
}

}  // namespace

// ================================================================================ C ABI

extern "C" {

int mfcc_hip_abi_version(void) { return MFCC_HIP_ABI_VERSION; }

int mfcc_hip_default_params(mfcc_hip_params *p) {
    if (!p) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::memset(p, 0, sizeof *p);
    p->struct_size = sizeof *p;
    p->nfft = 512;             // NFFT        software/main.c:11
    p->hop = 170;              // STEPSIZE    software/main.c:12
    p->n_mel = 32;             // nfilters    mfcc/targets/wav2mfcc.py:19
    p->n_cep = 13;             // BASELINE.json metric (reference tops keep 16/32)
    p->sample_rate = 16000;    // SAMPLERATE  software/main.c:14
    p->pad_mode = MFCC_HIP_PAD_NOTEBOOK;
    p->power_scale = 512.0f;   // MFCC.ipynb cell 22
    p->lifter = 0.0f;
    p->device = -1;
    p->float_impl = MFCC_HIP_IMPL_AUTO;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_num_frames(const mfcc_hip_params *p, size_t n_samples, size_t *n_frames) {
    return mfcc_hip_num_frames_framed(p, 0, n_samples, n_frames);
}

int mfcc_hip_num_frames_framed(const mfcc_hip_params *p, int frame_length, size_t n_samples, size_t *n_frames) {
    Resolved r;
    int rc = resolve_framed(p, frame_length, r);
    if (rc) return rc;
    if (!n_frames) return MFCC_HIP_ERROR_INVALID_PARAM;
    *n_frames = count_frames(r, n_samples);
    return MFCC_HIP_SUCCESS;
}

const char *mfcc_hip_strerror(int err) {
    switch (err) {
        case MFCC_HIP_SUCCESS: return "success";
        case MFCC_HIP_ERROR_INVALID_PARAM: return "invalid parameter";
        case MFCC_HIP_ERROR_NOT_FOUND: return "no usable HIP device (this library has no CPU path)";
        case MFCC_HIP_ERROR_NO_MEM: return "out of memory";
        case MFCC_HIP_ERROR_BUSY: return "busy";
        case MFCC_HIP_ERROR_UNSUPPORTED: return "parameter combination not supported by any kernel";
        case MFCC_HIP_ERROR_BUFFER_SMALL: return "output buffer too small";
        case MFCC_HIP_ERROR_IO: return "file i/o error";
        case MFCC_HIP_ERROR_OTHER: return "HIP runtime error (see mfcc_hip_last_hip_error)";
        default: return "unknown error";
    }
}

static thread_local int g_create_hip_error = 0;
int mfcc_hip_last_hip_error(const mfcc_hip_handle *h) { return h ? h->last_hip : g_create_hip_error; }

int mfcc_hip_get_table(const mfcc_hip_params *p, int which, void *buf, size_t cap, size_t *n_bytes) {
    return mfcc_hip_get_table_framed(p, 0, which, buf, cap, n_bytes);
}

int mfcc_hip_get_table_framed(const mfcc_hip_params *p, int frame_length, int which, void *buf, size_t cap,
                              size_t *n_bytes) {
    return mfcc_hip_get_table_banked(p, frame_length, nullptr, which, buf, cap, n_bytes);
}

int mfcc_hip_get_table_banked(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank, int which,
                              void *buf, size_t cap, size_t *n_bytes) {
    return mfcc_hip_get_table_fronted(p, frame_length, bank, nullptr, which, buf, cap, n_bytes);
}

int mfcc_hip_get_table_fronted(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank,
                               const mfcc_hip_front *front, int which, void *buf, size_t cap, size_t *n_bytes) {
    Resolved r;
    int rc = resolve_fronted(p, frame_length, bank, front, r);
    if (rc) return rc;
    std::vector<char> blob;
    auto put = [&](const void *d, size_t n) { blob.assign((const char *)d, (const char *)d + n); };
    switch (which) {
        case MFCC_HIP_TABLE_WINDOW_F32: {
            std::vector<double> w = frame_window(r);
            std::vector<float> f(w.begin(), w.end());
            put(f.data(), f.size() * 4);
            break;
        }
        case MFCC_HIP_TABLE_MEL_POINTS_I32: {
            if (is_htk(r)) return MFCC_HIP_ERROR_UNSUPPORTED;         // the bank has no integer filter points
            std::vector<int> v = mel_points(r.nfft, r.n_mel, double(r.sample_rate));
            put(v.data(), v.size() * 4);
            break;
        }
        case MFCC_HIP_TABLE_MEL_DENSE_F32: {
            std::vector<double> w = handle_mel(r);
            std::vector<float> f(w.begin(), w.end());
            put(f.data(), f.size() * 4);
            break;
        }
        case MFCC_HIP_TABLE_DCT_F32: {
            std::vector<double> w = dct_rows(r.n_cep, r.n_mel, r.lifter);
            std::vector<float> f(w.begin(), w.end());
            put(f.data(), f.size() * 4);
            break;
        }
        case MFCC_HIP_TABLE_FX_CURVE_I32: {
            std::vector<int> v = fx_window_curve(r.nfft);
            put(v.data(), v.size() * 4);
            break;
        }
        case MFCC_HIP_TABLE_FX_TWIDDLE_I32: {
            std::vector<int> re, im, v;
            fx_twiddles(r.nfft, re, im);
            for (size_t i = 0; i < re.size(); ++i) { v.push_back(re[i]); v.push_back(im[i]); }
            put(v.data(), v.size() * 4);
            break;
        }
        case MFCC_HIP_TABLE_FX_MEL_DENSE_U32: {
            if (!fixed_supported(r)) return MFCC_HIP_ERROR_UNSUPPORTED;
            FxMel m = fx_mel(r.nfft, r.n_mel, double(r.sample_rate));
            // first word: the shift; then the dense table
            std::vector<uint32_t> v;
            v.push_back(uint32_t(m.shift));
            v.insert(v.end(), m.dense.begin(), m.dense.end());
            put(v.data(), v.size() * 4);
            break;
        }
        default:
            return MFCC_HIP_ERROR_INVALID_PARAM;
    }
    if (n_bytes) *n_bytes = blob.size();
    if (buf) {
        if (cap < blob.size()) return MFCC_HIP_ERROR_BUFFER_SMALL;
        std::memcpy(buf, blob.data(), blob.size());
    }
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_create(const mfcc_hip_params *p, mfcc_hip_handle **out) { return mfcc_hip_create_framed(p, 0, out); }

int mfcc_hip_frame_length(const mfcc_hip_handle *h) { return h ? h->r.frame_len : 0; }

int mfcc_hip_create_framed(const mfcc_hip_params *p, int frame_length, mfcc_hip_handle **out) {
    return mfcc_hip_create_banked(p, frame_length, nullptr, out);
}

int mfcc_hip_mel_bank_of(const mfcc_hip_handle *h, mfcc_hip_mel_bank *out) {
    if (!h || !out) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out;
    out->kind = h->r.mel_kind;
    out->low_hz = float(h->r.mel_lo);
    out->high_hz = float(h->r.mel_hi);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_create_banked(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank,
                           mfcc_hip_handle **out) {
    return mfcc_hip_create_fronted(p, frame_length, bank, nullptr, out);
}

int mfcc_hip_front_of(const mfcc_hip_handle *h, mfcc_hip_front *out) {
    if (!h || !out) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::memset(out, 0, sizeof *out);
    out->struct_size = sizeof *out;
    out->window = h->r.front.window;
    out->symmetric = h->r.front.symmetric;
    out->preemph_num = h->r.front.num;
    out->preemph_den = h->r.front.den;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_create_fronted(const mfcc_hip_params *p, int frame_length, const mfcc_hip_mel_bank *bank,
                            const mfcc_hip_front *front, mfcc_hip_handle **out) {
    if (!out) return MFCC_HIP_ERROR_INVALID_PARAM;
    *out = nullptr;
    Resolved r;
    int rc = resolve_fronted(p, frame_length, bank, front, r);
    if (rc) return rc;
    int ndev = 0;
    g_create_hip_error = int(hipGetDeviceCount(&ndev));
    if (g_create_hip_error != int(hipSuccess) || ndev <= 0) return MFCC_HIP_ERROR_NOT_FOUND;
    int dev = r.device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return MFCC_HIP_ERROR_NOT_FOUND;
    }
    if (dev >= ndev) return MFCC_HIP_ERROR_NOT_FOUND;
    mfcc_hip_handle *h = new (std::nothrow) mfcc_hip_handle();
    if (!h) return MFCC_HIP_ERROR_NO_MEM;
    h->r = r;
    h->device = dev;
    auto fail = [&](int code) {
        mfcc_hip_destroy(h);
        return code;
    };
    DeviceGuard guard(dev);
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != dev) return fail(MFCC_HIP_ERROR_NOT_FOUND);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(MFCC_HIP_ERROR_OTHER);
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
        return fail(MFCC_HIP_ERROR_OTHER);
    h->stream = h->own_stream;
    if (hipEventCreateWithFlags(&h->scratch_done, hipEventDisableTiming) != hipSuccess)
        return fail(MFCC_HIP_ERROR_OTHER);
    rc = build_tables(h);
    if (rc) return fail(rc);
    if (r.float_impl == MFCC_HIP_IMPL_FUSED512 && !is_fused512(h->float_kernel)) return fail(MFCC_HIP_ERROR_UNSUPPORTED);
    *out = h;
    return MFCC_HIP_SUCCESS;
}

void mfcc_hip_destroy(mfcc_hip_handle *h) {
    if (!h) return;
    if (h->n_sessions > 0) {           // sessions still use the handle's stream and tables: the last one frees it
        h->destroy_pending = true;
        return;
    }
    DeviceGuard guard(h->device);
    if (h->scratch_used) (void)hipEventSynchronize(h->scratch_done);     // scratch may be in use on a caller's stream
    if (h->own_stream) {
        (void)hipStreamSynchronize(h->own_stream);
        (void)hipStreamDestroy(h->own_stream);
    }
    if (h->scratch_done) (void)hipEventDestroy(h->scratch_done);
    for (auto &d : h->desc) {
        if (d.copied) {
            if (d.in_flight) (void)hipEventSynchronize(d.copied);
            (void)hipEventDestroy(d.copied);
        }
        if (d.p) (void)hipHostFree(d.p);
    }
    for (int i = 0; i < mfcc_hip_handle::kPipe; ++i) {
        if (h->ev_in[i]) (void)hipEventDestroy(h->ev_in[i]);
        if (h->ev_k[i]) (void)hipEventDestroy(h->ev_k[i]);
        if (h->ev_out[i]) (void)hipEventDestroy(h->ev_out[i]);
        if (h->p_in[i].p) (void)hipFree(h->p_in[i].p);
        if (h->p_out[i].p) (void)hipFree(h->p_out[i].p);
    }
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    if (h->arena) (void)hipFree(h->arena);
    if (h->fb_dev) (void)hipFree(h->fb_dev);
    for (DevBuf *b : {&h->d_in, &h->d_out, &h->d_norm, &h->d_pcen, &h->d_full, &h->d_stat, &h->d_dtab, &h->d_slide, &h->d_stab,
                      &h->d_vad, &h->d_voiced, &h->d_sel, &h->d_final, &h->d_dec, &h->d_raw, &h->d_rs_tab, &h->d_rs, &h->d_ctr})
        if (b->p) (void)hipFree(b->p);
    delete h;
}

int mfcc_hip_set_stream(mfcc_hip_handle *h, void *hip_stream) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    h->stream = static_cast<hipStream_t>(hip_stream);      // NULL = the HIP null stream
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_use_own_stream(mfcc_hip_handle *h) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    h->stream = h->own_stream;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_synchronize(mfcc_hip_handle *h) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_process_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n, size_t nch, float *out,
                         size_t cap, size_t *n_frames) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->post.vad_mode) return MFCC_HIP_ERROR_UNSUPPORTED;   // a dense result cannot hold rows of different counts
    return process_host<float>(h, call_of(h, Kind::kFeatures, false), samples_of(h), pcm, n, nch, out, cap, n_frames);
}

int mfcc_hip_process_fixed_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n, size_t nch,
                               int16_t *out, size_t cap, size_t *n_frames) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;
    return process_host<int16_t>(h, call_of(h, Kind::kFeatures, true), samples_of(h), pcm, n, nch, out, cap, n_frames);
}

int mfcc_hip_process_ragged_i16(mfcc_hip_handle *h, const int16_t *pcm, const size_t *offsets, size_t n_utt,
                                float *out, size_t cap, size_t *frame_offsets) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    return process_ragged<float>(h, call_of(h, Kind::kFeatures, false), samples_of(h), pcm, offsets, n_utt, out, cap, frame_offsets);
}

int mfcc_hip_process_ragged_fixed_i16(mfcc_hip_handle *h, const int16_t *pcm, const size_t *offsets, size_t n_utt,
                                      int16_t *out, size_t cap, size_t *frame_offsets) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;
    return process_ragged<int16_t>(h, call_of(h, Kind::kFeatures, true), samples_of(h), pcm, offsets, n_utt, out, cap, frame_offsets);
}

int mfcc_hip_process_ragged_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets, size_t n_utt,
                                    void *d_out, size_t cap, size_t *frame_offsets) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    return process_ragged_dev<float>(h, call_of(h, Kind::kFeatures, false), samples_of(h), d_pcm, offsets, n_utt,
                                     static_cast<float *>(d_out), cap, frame_offsets);
}

int mfcc_hip_process_ragged_fixed_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets, size_t n_utt,
                                          void *d_out, size_t cap, size_t *frame_offsets) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;
    return process_ragged_dev<int16_t>(h, call_of(h, Kind::kFeatures, true), samples_of(h), d_pcm, offsets, n_utt,
                                       static_cast<int16_t *>(d_out), cap, frame_offsets);
}

int mfcc_hip_process_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n, size_t stride, size_t nch,
                             int halo, void *d_out, size_t *n_frames) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->post.vad_mode) return MFCC_HIP_ERROR_UNSUPPORTED;   // a dense result cannot hold rows of different counts
    return dense_dev(h, call_of(h, Kind::kFeatures, false), samples_of(h), d_pcm, n, stride, nch, halo, d_out, n_frames);
}

int mfcc_hip_process_fixed_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n, size_t stride,
                                   size_t nch, int halo, void *d_out, size_t *n_frames) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;
    return dense_dev(h, call_of(h, Kind::kFeatures, true), samples_of(h), d_pcm, n, stride, nch, halo, d_out, n_frames);
}

int mfcc_hip_time_dev(mfcc_hip_handle *h, int fixed, const void *d_pcm, size_t n, size_t stride,
                      size_t nch, void *d_out, int warmup, int iters, float *avg_ms) {
    if (!h || iters < 1 || warmup < 0 || !avg_ms) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (fixed && has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (h->post.vad_mode) return MFCC_HIP_ERROR_UNSUPPORTED;   // a dense result cannot hold rows of different counts
    DeviceGuard guard(h->device);
    // what process_*_dev enqueues: with a sample format the decode, with normalization or deltas on the passes behind
    // the float launch
    const Call c = call_of(h, Kind::kFeatures, fixed != 0);
    auto once = [&]() { return dense_dev(h, c, samples_of(h), d_pcm, n, stride, nch, 0, d_out, nullptr); };
    for (int i = 0; i < warmup; ++i) {
        int rc = once();
        if (rc) return rc;
    }
    struct Events {                                // destroyed on every return path
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    HIP_TRY(h, hipEventCreate(&ev.e0));
    HIP_TRY(h, hipEventCreate(&ev.e1));
    HIP_TRY(h, hipEventRecord(ev.e0, h->stream));
    for (int i = 0; i < iters; ++i) {
        int rc = once();
        if (rc) return rc;
    }
    HIP_TRY(h, hipEventRecord(ev.e1, h->stream));
    HIP_TRY(h, hipEventSynchronize(ev.e1));
    float ms = 0.0f;
    HIP_TRY(h, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *avg_ms = ms / float(iters);
    return MFCC_HIP_SUCCESS;
}

// ---- the power-spectrum output (include/mfcc_hip.h: "power spectrum"; kernel_spectrum.hpp, spectrum_plan.hpp; DESIGN.md
// section 4.18): the float entry points' own routes on a Kind::kSpectrum call
int mfcc_hip_spectrum_bins(const mfcc_hip_params *p, size_t *bins) {
    Resolved r;
    const int rc = resolve(p, r);
    if (rc || !bins) return rc ? rc : MFCC_HIP_ERROR_INVALID_PARAM;
    *bins = size_t(mfcc_spec::bins(r.nfft));
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_spectrum_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n, size_t stride, size_t nch, int halo,
                              void *d_out, size_t *n_frames) {
    if (!h || !mfcc_spec::call_fits(n, nch, size_t(mfcc_spec::bins(h->r.nfft)))) return MFCC_HIP_ERROR_INVALID_PARAM;
    return dense_dev(h, call_of(h, Kind::kSpectrum, false), samples_of(h), d_pcm, n, stride, nch, halo, d_out, n_frames);
}

int mfcc_hip_spectrum_ragged_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets, size_t n_utt, void *d_out,
                                     size_t cap, size_t *frame_offsets) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    // the row count times the bins must fit (decreasing offsets are the route's to refuse)
    if (offsets && n_utt && offsets[n_utt] >= offsets[0] &&
        !mfcc_spec::ragged_fits(offsets[n_utt] - offsets[0], n_utt, size_t(mfcc_spec::bins(h->r.nfft))))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    return process_ragged_dev<float>(h, call_of(h, Kind::kSpectrum, false), samples_of(h), d_pcm, offsets, n_utt,
                                     static_cast<float *>(d_out), cap, frame_offsets);
}

int mfcc_hip_spectrum_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n, size_t nch, float *out, size_t cap,
                          size_t *n_frames) {
    if (!h || !mfcc_spec::call_fits(n, nch, size_t(mfcc_spec::bins(h->r.nfft)))) return MFCC_HIP_ERROR_INVALID_PARAM;
    return process_host<float>(h, call_of(h, Kind::kSpectrum, false), samples_of(h), pcm, n, nch, out, cap, n_frames);
}

const char *mfcc_hip_spectrum_kernel_name(const mfcc_hip_handle *h) { return h ? mfcc_spec::name_of(h->spec_kernel) : ""; }

// ---- the filterbank output (include/mfcc_hip.h: "filterbank"; kernel_fbank.hpp, fbank_plan.hpp; DESIGN.md section
// 4.19): the spectrum entries' routes on a Kind::kFbank call
int mfcc_hip_set_fbank(mfcc_hip_handle *h, const mfcc_hip_fbank *p, const float *weights) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_fbank_banks > 0) return MFCC_HIP_ERROR_BUSY;      // a filterbank bank's width and state are this matrix's
    const int bins = mfcc_spec::bins(h->r.nfft);
    mfcc_fbank::Table t;
    mfcc_fbank::Sets sets;
    bool mfma = false;           // the fused kernel's MFMA form: the packed weights do not fit its LDS (fbank_plan.hpp)
    if (p) {
        if (p->struct_size != sizeof(mfcc_hip_fbank) || !weights) return MFCC_HIP_ERROR_INVALID_PARAM;
        for (int v : p->reserved)
            if (v != 0) return MFCC_HIP_ERROR_INVALID_PARAM;
        if (!mfcc_fbank::valid_bands(p->n_bands) || !mfcc_fbank::valid_scale(p->scale) || !mfcc_fbank::valid_floor(p->floor))
            return MFCC_HIP_ERROR_INVALID_PARAM;
        if (mfcc_fbank::first_bad_weight(weights, p->n_bands, bins) >= 0) return MFCC_HIP_ERROR_INVALID_PARAM;
        t = mfcc_fbank::build_table(weights, p->n_bands, bins);
        mfma = h->fb_kernel == mfcc_fbank::Kernel::kFused512 && !mfcc_fbank::weights_in_lds(t.packed.size());
        if (mfma && !mfcc_fbank::build_sets(weights, p->n_bands, bins, sets)) return MFCC_HIP_ERROR_OTHER;
    }
    DeviceGuard guard(h->device);
    void *dev = nullptr;
    if (p) {
        const std::vector<char> blob = mfma ? mfcc_fbank::build_blob(t, sets) : mfcc_fbank::build_blob(t);
        HIP_TRY(h, hipMalloc(&dev, blob.size()));
        const hipError_t e = hipMemcpy(dev, blob.data(), blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            HIP_TRY(h, e);
        }
    }
    // calls enqueued earlier, on whichever streams the handle had then, still read the old tables: the device is
    // synchronized before they are freed (include/mfcc_hip.h says so).  The new tables are a fresh allocation, so no
    // kernel in flight sees them
    if (h->fb_dev) {
        if (h->fb_used) {
            const hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) {
                if (dev) (void)hipFree(dev);
                HIP_TRY(h, e);
            }
        }
        (void)hipFree(h->fb_dev);
    }
    h->fb_dev = dev;
    h->fb = mfcc_fbank::Tables{};
    h->fb_used = false;
    h->fb_post = Post{};        // the settings were the old matrix's: checked against its scale, sized by its width
    if (p) {
        const char *b = static_cast<const char *>(dev);
        h->fb.w = reinterpret_cast<const float *>(b);
        h->fb.band = reinterpret_cast<const int4 *>(b + mfcc_fbank::blob_bands(t.packed.size()));
        h->fb.n_bands = p->n_bands;
        h->fb.w_total = int(t.packed.size());
        h->fb.c = mfcc_fbank::scale_factor(p->scale);
        h->fb.floor = p->floor == 0.0f ? 0.0f : p->floor;          // -0.0 -> +0.0
        h->fb_scale = p->scale;
        if (mfma) {
            h->fb.a_bf = reinterpret_cast<const uint4 *>(b + mfcc_fbank::blob_bytes(t.packed.size(), p->n_bands));
            for (int i = 0; i < mfcc_fbank::kMaxBlocks; ++i) h->fb.mask[i] = sets.mask[i], h->fb.set_first[i] = sets.first[i];
        }
    }
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_fbank_bands(const mfcc_hip_handle *h, size_t *n_bands) {
    if (!h || !n_bands) return MFCC_HIP_ERROR_INVALID_PARAM;
    *n_bands = size_t(h->fb.n_bands);
    return MFCC_HIP_SUCCESS;
}

// ---- the filterbank post-passes (include/mfcc_hip.h: "filterbank post-passes"): a Post of the
// matrix's own, which call_of hands to every Kind::kFbank call; the routes and the chain are the MFCC calls'
int mfcc_hip_set_filterbank_post(mfcc_hip_handle *h, const mfcc_hip_filterbank_post *p) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    Post q{};
    if (p) {
        if (p->struct_size != sizeof(mfcc_hip_filterbank_post)) return MFCC_HIP_ERROR_INVALID_PARAM;
        for (int v : p->reserved)
            if (v != 0) return MFCC_HIP_ERROR_INVALID_PARAM;
        if (!normalize_mode_ok(p->normalize) || !normalize_window_ok(p->normalize_window, p->normalize_min_window, p->normalize_center) ||
            !deltas_ok(p->delta_order, p->delta_window) || p->pcen_on < 0 || p->pcen_on > 1 || (p->pcen_on && !pcen_ok(&p->pcen)))
            return MFCC_HIP_ERROR_INVALID_PARAM;
        q.norm = p->normalize;
        q.norm_window = p->normalize_window;
        q.norm_min_window = p->normalize_window ? p->normalize_min_window : 1;
        q.norm_center = p->normalize_center;
        q.delta_order = p->delta_order;
        q.delta_window = p->delta_window;
        q.pcen_on = p->pcen_on != 0;
        if (q.pcen_on) q.pcen = pcen_prm(p->pcen);
    }
    if (!h->fb_dev) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (q.pcen_on && h->fb_scale != MFCC_HIP_FBANK_LOG2) return MFCC_HIP_ERROR_UNSUPPORTED;      // PCEN reads log2 energies
    if (h->n_fbank_banks > 0) return MFCC_HIP_ERROR_BUSY;      // a bank's frame launch is the raw kernel of this handle
    h->fb_post = q;
    return MFCC_HIP_SUCCESS;
}

size_t mfcc_hip_filterbank_row_width(const mfcc_hip_handle *h) {
    return h ? size_t(h->fb.n_bands) * size_t(1 + h->fb_post.delta_order) : 0;
}

int mfcc_hip_fbank_i16_dev(mfcc_hip_handle *h, const void *d_pcm, size_t n, size_t stride, size_t nch, int halo, void *d_out,
                           size_t *n_frames) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!h->fb_dev) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (!mfcc_fbank::call_fits(n, nch, mfcc_hip_filterbank_row_width(h))) return MFCC_HIP_ERROR_INVALID_PARAM;
    return dense_dev(h, call_of(h, Kind::kFbank, false), samples_of(h), d_pcm, n, stride, nch, halo, d_out, n_frames);
}

int mfcc_hip_fbank_ragged_i16_dev(mfcc_hip_handle *h, const void *d_pcm, const size_t *offsets, size_t n_utt, void *d_out,
                                  size_t cap, size_t *frame_offsets) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!h->fb_dev) return MFCC_HIP_ERROR_UNSUPPORTED;
    // the row count times the bands must fit (decreasing offsets are the route's to refuse)
    if (offsets && n_utt && offsets[n_utt] >= offsets[0] &&
        !mfcc_fbank::ragged_fits(offsets[n_utt] - offsets[0], n_utt, mfcc_hip_filterbank_row_width(h)))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    return process_ragged_dev<float>(h, call_of(h, Kind::kFbank, false), samples_of(h), d_pcm, offsets, n_utt,
                                     static_cast<float *>(d_out), cap, frame_offsets);
}

int mfcc_hip_fbank_i16(mfcc_hip_handle *h, const int16_t *pcm, size_t n, size_t nch, float *out, size_t cap, size_t *n_frames) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!h->fb_dev) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (!mfcc_fbank::call_fits(n, nch, mfcc_hip_filterbank_row_width(h))) return MFCC_HIP_ERROR_INVALID_PARAM;
    return process_host<float>(h, call_of(h, Kind::kFbank, false), samples_of(h), pcm, n, nch, out, cap, n_frames);
}

const char *mfcc_hip_fbank_kernel_name(const mfcc_hip_handle *h) {
    return h && h->fb_dev ? mfcc_fbank::name_of(h->fb_kernel) : "";
}

int mfcc_hip_htk_weights(int nfft, int sample_rate, int n_bands, float low_hz, float high_hz, float *out, size_t cap_floats,
                         size_t *n_floats) {
    if (!is_pow2(nfft) || nfft < 64 || nfft > 1024 || sample_rate <= 0 || !mfcc_fbank::valid_bands(n_bands))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    // the band edges as resolve_banked takes them
    const double lo = double(low_hz), hi = double(high_hz), nyq = double(sample_rate) / 2.0, top = hi == 0.0 ? nyq : hi;
    if (!(lo >= 0.0) || !(lo < top) || !(top <= nyq)) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t n = size_t(n_bands) * size_t(mfcc_spec::bins(nfft));
    if (n_floats) *n_floats = n;
    if (out) {
        if (cap_floats < n) return MFCC_HIP_ERROR_BUFFER_SMALL;
        const std::vector<double> w = mel_dense_htk(nfft, n_bands, double(sample_rate), lo, top);
        for (size_t i = 0; i < n; ++i) out[i] = float(w[i]);
    }
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_set_normalize(mfcc_hip_handle *h, int mode) {
    if (!h || !normalize_mode_ok(mode)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    h->post.norm = mode;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_normalize_dev(mfcc_hip_handle *h, void *d_rows, int row_width, const size_t *seg_offsets, size_t n_segs,
                           int mode) {
    if (!h || mode < MFCC_HIP_NORMALIZE_NONE || mode > MFCC_HIP_NORMALIZE_MEAN_VAR) return MFCC_HIP_ERROR_INVALID_PARAM;
    const RowPtr ptr[] = {{d_rows, 4, size_t(row_width) * sizeof(float), kWrite, false}};
    const int rc = check_rows(RowCall{row_width, mfcc_norm::kMaxWidth, seg_offsets, n_segs, nullptr, ptr, 1});
    if (rc != kProceed || mode == MFCC_HIP_NORMALIZE_NONE) return rc < 0 ? rc : MFCC_HIP_SUCCESS;
    DeviceGuard guard(h->device);
    return normalize_pass(h, static_cast<float *>(d_rows), row_width, span_offsets(seg_offsets, n_segs), mode);
}

int mfcc_hip_pcen_defaults(mfcc_hip_pcen *p) {
    if (!p) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::memset(p, 0, sizeof *p);
    p->struct_size = sizeof(mfcc_hip_pcen);
    p->s = 0.025f;
    p->alpha = 0.98f;
    p->delta = 2.0f;
    p->r = 0.5f;
    p->eps = 1e-6f;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_pcen_constants(const mfcc_hip_pcen *p, float *decay, float *a, float *delta_r) {
    if (!pcen_ok(p)) return MFCC_HIP_ERROR_INVALID_PARAM;
    const mfcc_pcen::Prm q = pcen_prm(*p);
    if (decay) std::memcpy(decay, q.decay, sizeof q.decay);
    if (a) *a = q.a;
    if (delta_r) *delta_r = q.delta_r;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_set_pcen(mfcc_hip_handle *h, const mfcc_hip_pcen *p) {
    if (!h || (p && !pcen_ok(p))) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (p && !is_logmel(h->r)) return MFCC_HIP_ERROR_UNSUPPORTED;      // PCEN reads log2 band energies
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    h->post.pcen_on = p != nullptr;
    if (p) h->post.pcen = pcen_prm(*p);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_pcen_dev(mfcc_hip_handle *h, void *d_rows, int row_width, const size_t *seg_offsets, size_t n_segs,
                      const mfcc_hip_pcen *p) {
    if (!h || !pcen_ok(p)) return MFCC_HIP_ERROR_INVALID_PARAM;
    const RowPtr ptr[] = {{d_rows, 4, size_t(row_width) * sizeof(float), kWrite, false}};
    const int rc = check_rows(RowCall{row_width, mfcc_pcen::kMaxWidth, seg_offsets, n_segs, nullptr, ptr, 1});
    if (rc != kProceed) return rc < 0 ? rc : MFCC_HIP_SUCCESS;
    DeviceGuard guard(h->device);
    return pcen_pass(h, static_cast<float *>(d_rows), row_width, span_offsets(seg_offsets, n_segs), pcen_prm(*p));
}

int mfcc_hip_set_normalize_window(mfcc_hip_handle *h, int window, int min_window, int center) {
    if (!h || !normalize_window_ok(window, min_window, center)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    h->post.norm_window = window;
    h->post.norm_min_window = window ? min_window : 1;
    h->post.norm_center = center;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_normalize_sliding_dev(mfcc_hip_handle *h, const void *d_in, int row_width, void *d_out,
                                   const size_t *seg_offsets, size_t n_segs, int mode, int window, int min_window,
                                   int center) {
    static_assert(MFCC_HIP_MAX_NORMALIZE_WINDOW == mfcc_slide::kMaxWindow, "window limit");
    if (!h || mode < MFCC_HIP_NORMALIZE_NONE || mode > MFCC_HIP_NORMALIZE_MEAN_VAR) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (window < 1 || window > MFCC_HIP_MAX_NORMALIZE_WINDOW || min_window < 1 || min_window > window || center < 0 ||
        center > 1)
        return MFCC_HIP_ERROR_INVALID_PARAM;
    // the byte ranges the pass reads and writes must not overlap: a window reaches into rows already written.  Mode NONE
    // touches neither pointer: none is looked at
    const size_t row_bytes = size_t(row_width) * sizeof(float);
    const RowPtr ptr[] = {{d_in, 4, row_bytes, kRead, false}, {d_out, 4, row_bytes, kWrite, false}};
    const bool none = mode == MFCC_HIP_NORMALIZE_NONE;
    const int rc = check_rows(RowCall{row_width, mfcc_slide::kMaxWidth, seg_offsets, n_segs, nullptr, ptr, none ? 0 : 2});
    if (rc != kProceed || none) return rc < 0 ? rc : MFCC_HIP_SUCCESS;
    DeviceGuard guard(h->device);
    return sliding_pass(h, static_cast<const float *>(d_in), static_cast<float *>(d_out), row_width,
                        span_offsets(seg_offsets, n_segs), SlideArgs{mode, window, min_window, center});
}

int mfcc_hip_set_deltas(mfcc_hip_handle *h, int order, int window) {
    if (!h || !deltas_ok(order, window)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    h->post.delta_order = order;
    h->post.delta_window = window;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_deltas_dev(mfcc_hip_handle *h, const void *d_in, int width, void *d_out, const size_t *seg_offsets,
                        size_t n_segs, int order, int window) {
    if (!h || order < 1 || order > 2 || window < 1 || window > MFCC_HIP_MAX_DELTA_WINDOW) return MFCC_HIP_ERROR_INVALID_PARAM;
    // the byte ranges the pass reads and writes must not overlap
    const size_t in_bytes = size_t(width) * sizeof(float);
    const RowPtr ptr[] = {{d_in, 4, in_bytes, kRead, false},
                          {d_out, 4, in_bytes * size_t(1 + order), kWrite, false}};
    const int rc = check_rows(RowCall{width, mfcc_delta::kMaxWidth, seg_offsets, n_segs, nullptr, ptr, 2});
    if (rc != kProceed) return rc < 0 ? rc : MFCC_HIP_SUCCESS;
    DeviceGuard guard(h->device);
    return deltas_pass(h, static_cast<const float *>(d_in), static_cast<float *>(d_out), width,
                       span_offsets(seg_offsets, n_segs), order, window);
}

int mfcc_hip_set_vad(mfcc_hip_handle *h, int mode, int column, float energy_threshold, float energy_mean_scale,
                     int frames_context, float proportion_threshold) {
    static_assert(MFCC_HIP_MAX_VAD_CONTEXT == mfcc_vad::kMaxContext, "context limit");
    if (!h || mode < MFCC_HIP_VAD_OFF || mode > MFCC_HIP_VAD_SELECT) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!vad_args_ok(int(row_width(h->r)), column, energy_threshold, energy_mean_scale, frames_context, proportion_threshold))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    h->post.vad_mode = mode;
    h->post.vad_column = column;
    h->post.vad_threshold = energy_threshold;
    h->post.vad_scale = energy_mean_scale;
    h->post.vad_context = frames_context;
    h->post.vad_proportion = proportion_threshold;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_vad_dev(mfcc_hip_handle *h, const void *d_rows, int row_width, int column, const size_t *seg_offsets,
                     size_t n_segs, float energy_threshold, float energy_mean_scale, int frames_context,
                     float proportion_threshold, void *d_voiced) {
    if (!h || !vad_args_ok(row_width, column, energy_threshold, energy_mean_scale, frames_context, proportion_threshold))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    // the rows read and the bytes written must not overlap
    const RowPtr ptr[] = {{d_rows, 4, size_t(row_width) * sizeof(float), kRead, false},
                          {d_voiced, 1, 1, kWrite, false}};
    const int rc = check_rows(RowCall{row_width, mfcc_vad::kMaxWidth, seg_offsets, n_segs, nullptr, ptr, 2});
    if (rc != kProceed) return rc < 0 ? rc : MFCC_HIP_SUCCESS;
    DeviceGuard guard(h->device);
    return vad_segments(h, static_cast<const float *>(d_rows), row_width, span_offsets(seg_offsets, n_segs),
                        VadArgs{column, energy_threshold, energy_mean_scale, frames_context, proportion_threshold},
                        static_cast<unsigned char *>(d_voiced));
}

int mfcc_hip_select_dev(mfcc_hip_handle *h, const void *d_in, int row_width, const void *d_voiced, const size_t *seg_offsets,
                        size_t n_segs, void *d_out, size_t out_capacity_rows, size_t *out_offsets) {
    if (!h || (n_segs && !out_offsets)) return MFCC_HIP_ERROR_INVALID_PARAM;
    // the rows and the mask read must not overlap the rows that may be written (every row may be voiced)
    const size_t row_bytes = size_t(row_width) * sizeof(float);
    const RowPtr ptr[] = {{d_in, 4, row_bytes, kRead, false}, {d_voiced, 1, 1, kRead, false},
                          {d_out, 4, row_bytes, kWritePacked, false}};
    const int rc = check_rows(RowCall{row_width, mfcc_vad::kMaxSelectWidth, seg_offsets, n_segs, nullptr, ptr, 3});
    if (rc == kNothing)
        return select_segments(h, nullptr, row_width, nullptr, span_offsets(seg_offsets, n_segs), nullptr, out_offsets);
    if (rc != kProceed) return rc;
    if (out_capacity_rows < seg_offsets[n_segs] - seg_offsets[0]) return MFCC_HIP_ERROR_BUFFER_SMALL;
    DeviceGuard guard(h->device);
    return select_segments(h, static_cast<const float *>(d_in), row_width, static_cast<const unsigned char *>(d_voiced),
                           span_offsets(seg_offsets, n_segs), static_cast<float *>(d_out), out_offsets);
}

const char *mfcc_hip_kernel_name(const mfcc_hip_handle *h, int fixed) {
    if (!h) return "";
    if (fixed) return h->fixed_kernel == FixedKernel::kFixed512 ? mfcc_fixed512::kernel_name() : "mfcc_fixed_kernel";
    switch (h->float_kernel) {
    case FloatKernel::kFused512W12: return mfcc_fused12::kernel_name();
    case FloatKernel::kFused512: return mfcc_fused::kernel_name();
    case FloatKernel::kFused512H160: return mfcc_fused160::kernel_name();
    case FloatKernel::kFused512H160Mb: return mfcc_fused160mb::kernel_name();
    case FloatKernel::kFused1024W12Bf: return mfcc_fused1024_w12bf::kernel_name();
    case FloatKernel::kFused1024W12F32: return mfcc_fused1024_w12::kernel_name();
    case FloatKernel::kFused1024Bf: return mfcc_fused1024::kernel_name();
    case FloatKernel::kFused1024F32: return mfcc_fused1024_f32::kernel_name();     // the same string as the bf16 form's
    case FloatKernel::kGeneric: break;
    }
    return "mfcc_float_generic_kernel";
}

// ---- sample formats (include/mfcc_hip.h: enum mfcc_hip_sample_format; kernel_decode.hpp)
size_t mfcc_hip_sample_size(int format) { return mfcc_decode::sample_size(format); }

int mfcc_hip_decode_host(int format, const void *in, size_t n, int16_t *out) {
    if (!mfcc_decode::known(format) || (n && (!in || !out))) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (n) mfcc_decode::decode_host(format, in, n, out);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_decode_dev(mfcc_hip_handle *h, int format, const void *d_in, size_t n, void *d_out) {
    if (!h || !mfcc_decode::known(format)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!n) return MFCC_HIP_SUCCESS;
    const size_t size = mfcc_decode::sample_size(format);
    const uintptr_t i_lo = reinterpret_cast<uintptr_t>(d_in), o_lo = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (i_lo & (size - 1)) || (o_lo & 1)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (ranges_overlap(i_lo, i_lo + n * size, o_lo, o_lo + n * sizeof(int16_t))) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    if (format == MFCC_HIP_SAMPLE_S16) {
        HIP_TRY(h, hipMemcpyAsync(d_out, d_in, n * sizeof(int16_t), hipMemcpyDeviceToDevice, h->stream));
        return MFCC_HIP_SUCCESS;
    }
    mfcc_decode::launch(format, d_in, static_cast<int16_t *>(d_out), n, 1, n, n, h->n_cu, h->stream);
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_set_sample_format(mfcc_hip_handle *h, int format) {
    if (!h || !mfcc_decode::known(format)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    h->sample_fmt = format;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_sample_format(const mfcc_hip_handle *h) { return h ? h->sample_fmt : MFCC_HIP_SAMPLE_S16; }

// ---- sample rates (include/mfcc_hip.h: "sample rates"): the direct entries
int mfcc_hip_resample_geometry(int in_rate, int out_rate, int *L, int *M, int *K) {
    mfcc_rs::Geometry g;
    const int rc = rs_geometry(in_rate, out_rate, g);
    if (rc) return rc;
    if (L) *L = g.L;
    if (M) *M = g.M;
    if (K) *K = g.K;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_resample_count(int in_rate, int out_rate, size_t n, size_t *n_out) {
    mfcc_rs::Geometry g;
    const int rc = rs_geometry(in_rate, out_rate, g);
    if (rc) return rc;
    if (!n_out || n >= mfcc_rs::kMaxLen) return MFCC_HIP_ERROR_INVALID_PARAM;
    *n_out = size_t(mfcc_rs::count(n, g.L, g.M));
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_resample_taps(int in_rate, int out_rate, int16_t *buf, size_t cap, size_t *n) {
    mfcc_rs::Geometry g;
    std::vector<int16_t> t;
    const int rc = rs_table(in_rate, out_rate, g, t);
    if (rc) return rc;
    if (n) *n = t.size();
    if (cap < t.size()) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (!buf) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::memcpy(buf, t.data(), t.size() * sizeof(int16_t));
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_resample_host(int in_rate, int out_rate, const int16_t *in, size_t n, int16_t *out, size_t cap) {
    mfcc_rs::Geometry g;
    std::vector<int16_t> t;
    const int rc = rs_table(in_rate, out_rate, g, t);
    if (rc) return rc;
    if (n >= mfcc_rs::kMaxLen) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t n_out = size_t(mfcc_rs::count(n, g.L, g.M));
    if (cap < n_out) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (n && (!in || !out)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (n) mfcc_rs::resample_host(g, t.data(), in, (long long)n, 0, (long long)n_out, out);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_resample_dev(mfcc_hip_handle *h, int in_rate, int out_rate, const void *d_in, size_t n, void *d_out, size_t cap) {
    if (!h) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_rs::Geometry g;
    int rc = rs_geometry(in_rate, out_rate, g);
    if (rc) return rc;
    if (n >= mfcc_rs::kMaxLen) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t n_out = size_t(mfcc_rs::count(n, g.L, g.M));
    if (cap < n_out) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (!n) return MFCC_HIP_SUCCESS;
    const uintptr_t i_lo = reinterpret_cast<uintptr_t>(d_in), o_lo = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (i_lo & 1) || (o_lo & 1)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (ranges_overlap(i_lo, i_lo + n * sizeof(int16_t), o_lo, o_lo + n_out * sizeof(int16_t))) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    mfcc_rs::Taps a;
    if ((rc = rs_bind(h, in_rate, out_rate, a))) return rc;
    mfcc_rs::launch(a, static_cast<const int16_t *>(d_in), (long long)n, static_cast<int16_t *>(d_out), (long long)n_out, 1, 0, 0,
                    nullptr, 0, h->n_cu, h->stream);
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_set_input_rate(mfcc_hip_handle *h, int in_rate) {
    if (!h || in_rate < 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    if (in_rate == 0 || in_rate == h->r.sample_rate) {
        h->input_rate = 0;
        return MFCC_HIP_SUCCESS;
    }
    DeviceGuard guard(h->device);
    mfcc_rs::Taps a;
    const int rc = rs_bind(h, in_rate, h->r.sample_rate, a);          // the ratio's refusals; the table is on the device
    if (rc) return rc;
    h->input_rate = in_rate;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_input_rate(const mfcc_hip_handle *h) { return h ? h->input_rate : 0; }

// ---- centring (include/mfcc_hip.h: "centring"): the geometry, the host rule, the direct entry
static int center_resolve(const mfcc_hip_params *p, int frame_length, int mode, mfcc_center::Geom &g) {
    Resolved r;
    const int rc = resolve_framed(p, frame_length, r);
    if (rc) return rc;
    if (mode != MFCC_HIP_CENTER_REFLECT && mode != MFCC_HIP_CENTER_ZEROS) return MFCC_HIP_ERROR_INVALID_PARAM;
    g = center_geom(r, mode);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_center_geometry(const mfcc_hip_params *p, int frame_length, int mode, size_t n, size_t *n_frames, size_t *left,
                             size_t *padded) {
    mfcc_center::Geom g;
    const int rc = center_resolve(p, frame_length, mode, g);
    if (rc) return rc;
    if (n_frames) *n_frames = mfcc_center::frames(g, n);
    if (left) *left = size_t(g.left);
    if (padded) *padded = mfcc_center::padded(g, n);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_center_host(const mfcc_hip_params *p, int frame_length, int mode, const int16_t *in, size_t n, int16_t *out,
                         size_t cap, size_t *n_out) {
    mfcc_center::Geom g;
    const int rc = center_resolve(p, frame_length, mode, g);
    if (rc) return rc;
    const size_t np = mfcc_center::padded(g, n);
    if (n_out) *n_out = np;
    if (cap < np) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (np && (!in || !out)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (np) mfcc_center::center_host(g, in, n, out);
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_center_dev(mfcc_hip_handle *h, int mode, int format, const void *d_in, size_t n, void *d_out, size_t cap,
                        size_t *n_out) {
    if (!h || !mfcc_decode::known(format) || (mode != MFCC_HIP_CENTER_REFLECT && mode != MFCC_HIP_CENTER_ZEROS))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    const mfcc_center::Geom g = center_geom(h->r, mode);
    const size_t np = mfcc_center::padded(g, n);
    if (n_out) *n_out = np;
    if (cap < np) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (!np) return MFCC_HIP_SUCCESS;
    const size_t size = mfcc_decode::sample_size(format);
    const uintptr_t i_lo = reinterpret_cast<uintptr_t>(d_in), o_lo = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (i_lo & (size - 1)) || (o_lo & 1)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (ranges_overlap(i_lo, i_lo + n * size, o_lo, o_lo + np * sizeof(int16_t))) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    mfcc_center::launch_dense(format, d_in, static_cast<int16_t *>(d_out), n, np, 1, n, np, g, h->n_cu, h->stream);
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_set_center(mfcc_hip_handle *h, int mode) {
    if (!h || !mfcc_center::known(mode)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->n_sessions > 0) return MFCC_HIP_ERROR_BUSY;
    // the padded signal is framed by MFCC_HIP_PAD_NOTEBOOK: the stream rule would add a zero-padded frame behind it
    if (mode != MFCC_HIP_CENTER_OFF && h->r.pad_mode != MFCC_HIP_PAD_NOTEBOOK) return MFCC_HIP_ERROR_UNSUPPORTED;
    h->center = mode;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_center(const mfcc_hip_handle *h) { return h ? h->center : MFCC_HIP_CENTER_OFF; }

// float coefficients -> the int16 a `.mfcc` file holds: astype(np.int16) of software/lift.py:39 (truncate)
static inline int16_t to_mfcc_i16(float v) {
    if (!(v == v)) v = 0.0f;
    if (v > 32767.0f) v = 32767.0f;
    if (v < -32768.0f) v = -32768.0f;
    return int16_t(v);
}

int mfcc_hip_convert_wav(mfcc_hip_handle *h, const char *wav_in, const char *mfcc_out, int fixed,
                         size_t *n_frames_out) {
    if (!h || !wav_in || !mfcc_out) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (is_logmel(h->r)) return MFCC_HIP_ERROR_UNSUPPORTED;     // a .mfcc file holds cepstra
    if (has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;   // ... raw ones, n_cep wide, of every frame
    if (fixed && h->center) return MFCC_HIP_ERROR_UNSUPPORTED;  // the fixed-point framing is the RTL's
    std::vector<int16_t> pcm;
    int rc = read_wav_i16(wav_in, rated(h) ? h->input_rate : h->r.sample_rate, pcm);
    if (rc) return rc;
    const size_t nf = count_frames(h->r, framed_len(h, samples_of(h), own_rate_len(h, pcm.size())));
    std::vector<int16_t> cep(nf * size_t(h->r.n_cep));
    // the file's 16-bit PCM, whatever the handle's sample format, at the rate the handle reads
    const Samples pcm16{MFCC_HIP_SAMPLE_S16, h->input_rate, h->center};
    if (fixed) {
        rc = process_host<int16_t>(h, call_of(h, Kind::kFeatures, true), pcm16, pcm.data(), pcm.size(), 1, cep.data(), cep.size(), nullptr);
        if (rc) return rc;
    } else {
        std::vector<float> f(cep.size());
        rc = process_host<float>(h, call_of(h, Kind::kFeatures, false), pcm16, pcm.data(), pcm.size(), 1, f.data(), f.size(), nullptr);
        if (rc) return rc;
        for (size_t i = 0; i < f.size(); ++i) cep[i] = to_mfcc_i16(f[i]);
    }
    FILE *o = std::fopen(mfcc_out, "wb");
    if (!o) return MFCC_HIP_ERROR_IO;
    size_t wr = cep.empty() ? 0 : std::fwrite(cep.data(), sizeof(int16_t), cep.size(), o);
    std::fclose(o);
    if (wr != cep.size()) return MFCC_HIP_ERROR_IO;
    if (n_frames_out) *n_frames_out = nf;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_convert_wavs(mfcc_hip_handle *h, const char *const *wav_in, const char *const *mfcc_out, size_t n_files,
                          int fixed, size_t *n_frames_each) {
    if (!h || (n_files && (!wav_in || !mfcc_out))) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (is_logmel(h->r)) return MFCC_HIP_ERROR_UNSUPPORTED;     // a .mfcc file holds cepstra
    if (has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;   // ... raw ones, n_cep wide, of every frame
    if (fixed && h->center) return MFCC_HIP_ERROR_UNSUPPORTED;  // the fixed-point framing is the RTL's
    std::vector<int16_t> pcm;
    std::vector<size_t> off(n_files + 1, 0), fo(n_files + 1, 0);
    for (size_t i = 0; i < n_files; ++i) {
        if (!wav_in[i] || !mfcc_out[i]) return MFCC_HIP_ERROR_INVALID_PARAM;
        std::vector<int16_t> one;
        int rc = read_wav_i16(wav_in[i], rated(h) ? h->input_rate : h->r.sample_rate, one);
        if (rc) return rc;
        pcm.insert(pcm.end(), one.begin(), one.end());
        off[i + 1] = pcm.size();
    }
    size_t total = 0;
    for (size_t i = 0; i < n_files; ++i) total += count_frames(h->r, framed_len(h, samples_of(h), own_rate_len(h, off[i + 1] - off[i])));
    const size_t ncep = size_t(h->r.n_cep);
    std::vector<int16_t> cep(total * ncep);
    int rc;
    const Samples pcm16{MFCC_HIP_SAMPLE_S16, h->input_rate, h->center};
    if (fixed) {
        rc = process_ragged<int16_t>(h, call_of(h, Kind::kFeatures, true), pcm16, pcm.data(), off.data(), n_files, cep.data(),
                                     cep.size(), fo.data());
        if (rc) return rc;
    } else {
        std::vector<float> f(cep.size());
        rc = process_ragged<float>(h, call_of(h, Kind::kFeatures, false), pcm16, pcm.data(), off.data(), n_files, f.data(),
                                   f.size(), fo.data());
        if (rc) return rc;
        for (size_t i = 0; i < f.size(); ++i) cep[i] = to_mfcc_i16(f[i]);
    }
    for (size_t i = 0; i < n_files; ++i) {
        const size_t nf = fo[i + 1] - fo[i];
        FILE *o = std::fopen(mfcc_out[i], "wb");
        if (!o) return MFCC_HIP_ERROR_IO;
        const size_t want = nf * ncep;
        const size_t wr = want ? std::fwrite(cep.data() + fo[i] * ncep, sizeof(int16_t), want, o) : 0;
        std::fclose(o);
        if (wr != want) return MFCC_HIP_ERROR_IO;
        if (n_frames_each) n_frames_each[i] = nf;
    }
    return MFCC_HIP_SUCCESS;
}

// ---- online / streaming session (include/mfcc_hip.h: mfcc_hip_stream_*) -----------------------------------
// Device buffer layout, both ping-pong buffers: [0] = the history sample x[first - 1] (0 after reset),
// [1 .. 1 + pending) = the samples of the frame in progress, then the new samples of this push.

}  // extern "C"

struct mfcc_hip_stream {
    mfcc_hip_handle *h = nullptr;
    bool fixed = false;
    int16_t *buf[2] = {nullptr, nullptr};
    size_t cap = 0;                 // samples each buffer holds behind the history slot
    int cur = 0;                    // buffer that holds history + pending
    size_t pending = 0;
    void *d_out = nullptr;
    size_t d_out_bytes = 0;
};

namespace {

int stream_reserve(mfcc_hip_stream *s, size_t samples, size_t out_bytes) {
    mfcc_hip_handle *h = s->h;
    if (samples > s->cap) {
        const size_t want = samples + samples / 2 + 4096;
        int16_t *nb[2] = {nullptr, nullptr};
        for (int i = 0; i < 2; ++i) HIP_TRY(h, hipMalloc(reinterpret_cast<void **>(&nb[i]), (want + 1 + 64) * sizeof(int16_t)));
        // carry history + pending over (the other buffer holds nothing that is still needed)
        HIP_TRY(h, hipMemsetAsync(nb[0], 0, sizeof(int16_t), h->stream));
        if (s->buf[s->cur])
            HIP_TRY(h, hipMemcpyAsync(nb[0], s->buf[s->cur], (1 + s->pending) * sizeof(int16_t), hipMemcpyDeviceToDevice,
                                      h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < 2; ++i) {
            if (s->buf[i]) (void)hipFree(s->buf[i]);
            s->buf[i] = nb[i];
        }
        s->cur = 0;
        s->cap = want;
    }
    if (out_bytes > s->d_out_bytes) {
        if (s->d_out) HIP_TRY(h, hipFree(s->d_out));
        s->d_out = nullptr;
        s->d_out_bytes = 0;
        const size_t want = out_bytes + out_bytes / 2 + 4096;
        HIP_TRY(h, hipMalloc(&s->d_out, want));
        s->d_out_bytes = want;
    }
    return MFCC_HIP_SUCCESS;
}

// run `nf` frames over history + the first `total` samples of the current buffer, copy them to `out`
int stream_emit(mfcc_hip_stream *s, size_t total, size_t nf, void *out) {
    mfcc_hip_handle *h = s->h;
    const size_t esz = s->fixed ? sizeof(int16_t) : sizeof(float);
    const size_t bytes = nf * row_width(h->r) * esz;
    int rc = launch(h, call_of(h, Kind::kFeatures, s->fixed), s->buf[s->cur], total, total + 1, 1, /*halo=*/1, s->d_out, nullptr, nf);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, s->d_out, bytes, hipMemcpyDeviceToHost, h->stream));
    return MFCC_HIP_SUCCESS;
}

}  // namespace

extern "C" {

int mfcc_hip_stream_create(mfcc_hip_handle *h, int fixed, mfcc_hip_stream **out) {
    if (!h || !out) return MFCC_HIP_ERROR_INVALID_PARAM;
    *out = nullptr;
    if (h->destroy_pending) return MFCC_HIP_ERROR_INVALID_PARAM;        // the handle was already given back
    if (h->post.norm != MFCC_HIP_NORMALIZE_NONE) return MFCC_HIP_ERROR_UNSUPPORTED;   // per-call statistics of a stream
    if (h->post.pcen_on) return MFCC_HIP_ERROR_UNSUPPORTED;                           // ... and a per-call smoother
    if (h->post.delta_order) return MFCC_HIP_ERROR_UNSUPPORTED;     // deltas need 2 K N frames of lookahead
    if (h->post.vad_mode) return MFCC_HIP_ERROR_UNSUPPORTED;        // the threshold's mean is a whole-segment statistic
    if (rated(h)) return MFCC_HIP_ERROR_UNSUPPORTED;           // a line's rate conversion keeps state between pushes
    if (h->center) return MFCC_HIP_ERROR_UNSUPPORTED;          // a centred line holds back PL + 1 samples, flushes several frames
    if (fixed && h->fixed_kernel == FixedKernel::kNone) return MFCC_HIP_ERROR_UNSUPPORTED;
    mfcc_hip_stream *s = new (std::nothrow) mfcc_hip_stream();
    if (!s) return MFCC_HIP_ERROR_NO_MEM;
    s->h = h;
    s->fixed = fixed != 0;
    ++h->n_sessions;
    DeviceGuard guard(h->device);
    int rc = stream_reserve(s, size_t(h->r.frame_len) * 8, size_t(64) * row_width(h->r) * sizeof(float));
    if (rc) {
        mfcc_hip_stream_destroy(s);
        return rc;
    }
    *out = s;
    return MFCC_HIP_SUCCESS;
}

void mfcc_hip_stream_destroy(mfcc_hip_stream *s) {
    if (!s) return;
    mfcc_hip_handle *h = s->h;
    {
        DeviceGuard guard(h->device);
        (void)hipStreamSynchronize(h->stream);
        for (int i = 0; i < 2; ++i)
            if (s->buf[i]) (void)hipFree(s->buf[i]);
        if (s->d_out) (void)hipFree(s->d_out);
        delete s;
    }
    if (--h->n_sessions == 0 && h->destroy_pending) mfcc_hip_destroy(h);
}

int mfcc_hip_stream_reset(mfcc_hip_stream *s) {
    if (!s) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(s->h->device);
    s->pending = 0;
    HIP_TRY(s->h, hipMemsetAsync(s->buf[s->cur], 0, sizeof(int16_t), s->h->stream));     // history := 0
    HIP_TRY(s->h, hipStreamSynchronize(s->h->stream));
    return MFCC_HIP_SUCCESS;
}

size_t mfcc_hip_stream_pending(const mfcc_hip_stream *s) { return s ? s->pending : 0; }

size_t mfcc_hip_stream_max_frames(const mfcc_hip_stream *s, size_t n) {
    return s ? (s->pending + n) / size_t(s->h->r.hop) + 1 : 0;
}

int mfcc_hip_stream_push(mfcc_hip_stream *s, const int16_t *samples, size_t n, void *out, size_t cap,
                         size_t *n_frames_out) {
    if (!s || (n && !samples)) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = s->h;
    const size_t flen = size_t(h->r.frame_len), hop = size_t(h->r.hop), ncep = row_width(h->r);
    const size_t total = s->pending + n;
    const size_t nf = total >= flen ? (total - flen) / hop + 1 : 0;          // frames this push completes
    if (n_frames_out) *n_frames_out = nf;
    if (nf && (!out || cap < nf * ncep)) return MFCC_HIP_ERROR_BUFFER_SMALL;  // nothing consumed yet
    DeviceGuard guard(h->device);
    int rc = stream_reserve(s, total, nf * ncep * sizeof(float));
    if (rc) return rc;
    if (n && decodes(h->sample_fmt)) {
        // the raw bytes to the device, decoded straight to their place behind the pending samples
        const size_t raw = n * sample_bytes(h->sample_fmt);
        if ((rc = ensure(h, h->d_raw, raw + 64)) || (rc = scratch_acquire(h))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_raw.p, samples, raw, hipMemcpyHostToDevice, h->stream));
        if ((rc = decode_rows(h, h->sample_fmt, h->d_raw.p, n, 1, n, s->buf[s->cur] + 1 + s->pending, n)) || (rc = scratch_release(h)))
            return rc;
    } else if (n) {
        HIP_TRY(h, hipMemcpyAsync(s->buf[s->cur] + 1 + s->pending, samples, n * sizeof(int16_t), hipMemcpyHostToDevice,
                                  h->stream));
    }
    if (nf) {
        rc = stream_emit(s, total, nf, out);
        if (rc) return rc;
        // the next frame starts nf hops further on: its history sample and what is already there move to the
        // front of the other buffer
        const size_t used = nf * hop;
        HIP_TRY(h, hipMemcpyAsync(s->buf[s->cur ^ 1], s->buf[s->cur] + used, (1 + total - used) * sizeof(int16_t),
                                  hipMemcpyDeviceToDevice, h->stream));
        s->cur ^= 1;
        s->pending = total - used;
    } else {
        s->pending = total;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // `samples` and `out` belong to the caller again
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_stream_flush(mfcc_hip_stream *s, void *out, size_t cap, size_t *n_frames_out) {
    if (!s) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = s->h;
    const size_t nf = h->r.pad_mode == MFCC_HIP_PAD_STREAM ? 1 : 0;
    if (n_frames_out) *n_frames_out = nf;
    if (nf && (!out || cap < row_width(h->r))) return MFCC_HIP_ERROR_BUFFER_SMALL;
    DeviceGuard guard(h->device);
    if (nf) {
        // the zero-padded tail frame of main.c:134-144: the pending samples, then zeros (the kernels read
        // x[i] = 0 beyond the `total` samples they are given)
        int rc = stream_emit(s, s->pending, 1, out);
        if (rc) return rc;
    }
    return mfcc_hip_stream_reset(s);
}

// ---- live objects: what a stream bank, a gate tracker and a resampler share (the session above keeps buffers of its own
// and is timed against the bank in profiles/session_bank_of_one.txt).  Each keeps a
// handle `h`, `n` lines, device allocations of its own and per-line counts on the host, and counts as a session of its
// handle (include/mfcc_hip.h: the lifetime rule at mfcc_hip_destroy)

}  // extern "C"

namespace {

// The first checks of every create: INVALID_PARAM for a missing handle or out pointer, then -- *out cleared -- for a
// handle already given back or no lines.  The object's own checks follow
template <class T>
int live_check(const mfcc_hip_handle *h, size_t n_lines, T **out) {
    if (!h || !out) return MFCC_HIP_ERROR_INVALID_PARAM;
    *out = nullptr;
    return h->destroy_pending || !n_lines ? MFCC_HIP_ERROR_INVALID_PARAM : MFCC_HIP_SUCCESS;
}

// a new object of n_lines lines that counts as a session of h from here on; NULL: no memory
template <class T>
T *live_new(mfcc_hip_handle *h, size_t n_lines) {
    T *o = new (std::nothrow) T();
    if (!o) return nullptr;
    o->h = h;
    o->n = n_lines;
    ++h->n_sessions;
    return o;
}

// The object's work drained -- a push may be in flight on a caller's stream --, its device memory (T::owned) freed, the
// object deleted and its handle released: the last one frees a handle that was already given back
template <class T>
void live_destroy(T *o) {
    if (!o) return;
    mfcc_hip_handle *h = o->h;
    {
        DeviceGuard guard(h->device);
        if (h->scratch_used) (void)hipEventSynchronize(h->scratch_done);
        (void)hipStreamSynchronize(h->stream);
        for (void *p : o->owned())
            if (p) (void)hipFree(p);
        delete o;
    }
    if (--h->n_sessions == 0 && h->destroy_pending) mfcc_hip_destroy(h);
}

// the end of a create: e is what its allocations and copies answered
template <class T>
int live_created(T *o, hipError_t e, T **out) {
    if (e == hipSuccess) {
        *out = o;
        return MFCC_HIP_SUCCESS;
    }
    o->h->last_hip = int(e);
    live_destroy(o);
    return e == hipErrorOutOfMemory ? MFCC_HIP_ERROR_NO_MEM : MFCC_HIP_ERROR_OTHER;
}

// a count per line, copied to the caller
template <class T>
int live_counts(const T *o, std::vector<size_t> T::*count, size_t *dst) {
    if (!o || !dst) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::copy((o->*count).begin(), (o->*count).end(), dst);
    return MFCC_HIP_SUCCESS;
}

// `idx` of a flush / reset / window request as a list: NULL = every index below `size`, else n distinct ones below it
int live_lines(size_t size, const size_t *idx, size_t n, std::vector<size_t> &list) {
    list.clear();
    if (!idx) {
        for (size_t u = 0; u < size; ++u) list.push_back(u);
        return MFCC_HIP_SUCCESS;
    }
    std::vector<char> hit(size, 0);
    for (size_t i = 0; i < n; ++i) {
        if (idx[i] >= size || hit[idx[i]]) return MFCC_HIP_ERROR_INVALID_PARAM;
        hit[idx[i]] = 1;
        list.push_back(idx[i]);
    }
    return MFCC_HIP_SUCCESS;
}

// The listed lines back in the reset state: these counts of theirs are 0.  The counts travel with the records of every
// launch, and a line whose count is 0 reads nothing of what it has on the device
void live_zero(const std::vector<size_t> &list, std::initializer_list<std::vector<size_t> *> counts) {
    for (std::vector<size_t> *c : counts)
        for (size_t u : list) (*c)[u] = 0;
}

// a reset that is nothing more: `lines` as a list (NULL: every line), then that count of theirs to 0
template <class T>
int live_reset(T *o, const size_t *lines, size_t n, std::vector<size_t> T::*count) {
    if (!o) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::vector<size_t> list;
    const int rc = live_lines(o->n, lines, n, list);
    if (!rc) live_zero(list, {&(o->*count)});
    return rc;
}

}  // namespace

extern "C" {

// ---- stream bank (include/mfcc_hip.h: mfcc_hip_bank_*; kernel_stream_bank.hpp) -------------
// N sessions whose state rows ([history | pending], frame_len int16 each) lie in one device allocation.  A push is planned on
// the host from lengths alone, described by one record per stream in the pinned descriptor pool and carried out by ONE
// launch of bank_advance_kernel, ONE launch of the frame kernels over the active streams' rows of the work buffer W
// (h->d_in) and, when the streams complete different numbers of frames, ONE row gather out of h->d_out.
// An online bank (mfcc_hip_bank_create_online) keeps raw rows and static rows per stream as
// well: its frame launch always goes to h->d_out, and the CMVN, delta and carry kernels of
// kernel_stream_bank_online.hpp follow on the same stream; there is no gather, the delta kernel writes packed rows.

}  // extern "C"

struct mfcc_hip_bank {
    mfcc_hip_handle *h = nullptr;
    Kind kind = Kind::kFeatures;         // what its frame launch computes: the handle's own rows, or its filterbank rows
    bool fixed = false;
    size_t n = 0;                        // streams
    mfcc_bank::Settings s{};             // what the plans of a push, flush or reset read (bank_plan.hpp)
    int16_t *d_state = nullptr;          // [n][frame_len]
    std::vector<size_t> pending, after;  // the host mirror and the plan of the push in progress
    // staging of the host-buffer entries (mfcc_hip_bank_push, mfcc_hip_bank_flush): the flat samples and the rows
    DevBuf st_in, st_out;
    // online bank (mfcc_hip_bank_create_online; kernel_stream_bank_online.hpp): causal CMVN
    // over `window` rows and deltas of s.order x `dwin`, lag s.L = order * dwin.  seen[u] = frames computed since reset,
    // held[u] <= lag = finished rows not yet returned; both depend on chunk lengths only
    int norm = MFCC_HIP_NORMALIZE_NONE, window = 0, depth = 0, dwin = 0;
    float *d_ring = nullptr;             // [n][depth][W] raw rows (norm != NONE)
    float *d_tail = nullptr;             // [n][2 lag][W] static rows (lag > 0)
    std::vector<size_t> seen, held, held_after, raw_fo;
    // PCEN of an online bank (mfcc_hip_bank_create_online_pcen): the parameters and, on
    // the device, [n][2][W] carry and local smoother per (stream, column), then the decay table A_k
    mfcc_pcen::Prm pcen_prm{};
    float *d_pcen = nullptr;
    std::vector<void *> owned() const { return {d_state, d_ring, d_tail, d_pcen, st_in.p, st_out.p}; }
    ~mfcc_hip_bank() {                   // in front of the handle's release (live_destroy)
        if (kind == Kind::kFbank) --h->n_fbank_banks;
    }
};

namespace {

inline mfcc_bank::State bank_state(const mfcc_hip_bank *b) {
    return mfcc_bank::State{b->pending.data(), b->seen.data(), b->held.data()};
}

// a record table of the descriptor block at the front of h->d_out
template <class T>
inline const T *desc_table(const mfcc_hip_handle *h, const mfcc_bank::Table &t) {
    return reinterpret_cast<const T *>(static_cast<const long long *>(h->d_out.p) + t.off);
}

template <typename OutT>
void bank_gather(mfcc_hip_handle *h, const mfcc_bank::Layout &l, const void *d_rows, void *y, int W) {
    const unsigned blocks = (unsigned)std::min<size_t>(l.gather.n, size_t(h->n_cu) * 8);
    hipLaunchKernelGGL(gather_rows_kernel<OutT>, dim3(blocks), dim3(256), 0, h->stream, static_cast<const OutT *>(d_rows),
                       static_cast<OutT *>(y), desc_table<long long>(h, l.gather), (long long)l.gather.n, W);
}

// What follows the frame launch of a push or an end, on the handle's stream; y: the rows of the result.  A plain bank
// gathers the rows of a mixed push.  An online bank runs PCEN over the fresh raw rows -- in place when CMVN or deltas
// follow (the PCEN rows are what enters the ring and the tail), else straight to y -- then CMVN, the deltas and, in a
// push, the carry into ring and tail (a flush resets instead)
void bank_passes(mfcc_hip_bank *b, const mfcc_bank::Layout &l, void *y) {
    mfcc_hip_handle *h = b->h;
    const mfcc_bank::Settings &s = b->s;
    const int W = int(s.W);
    const size_t cap = size_t(h->n_cu) * 8;
    float *d_raw = reinterpret_cast<float *>(static_cast<char *>(h->d_out.p) + l.raw_off);
    float *d_stat = reinterpret_cast<float *>(static_cast<char *>(h->d_out.p) + l.stat_off), *out = static_cast<float *>(y);
    if (!s.online()) {
        if (l.gather.n) b->fixed ? bank_gather<int16_t>(h, l, d_raw, y, W) : bank_gather<float>(h, l, d_raw, y, W);
        return;
    }
    if (l.pcen.n) {
        const size_t blocks = std::min((l.pcen.n * s.W + mfcc_pcen::kThreads - 1) / mfcc_pcen::kThreads, cap);
        hipLaunchKernelGGL(mfcc_pcen::online_pcen_kernel, dim3((unsigned)blocks), dim3(mfcc_pcen::kThreads), 0, h->stream, d_raw,
                           s.post() ? d_raw : out, desc_table<mfcc_pcen::OnlineRec>(h, l.pcen), (long long)l.pcen.n, W,
                           b->pcen_prm, static_cast<const float *>(b->d_pcen + b->n * 2 * s.W), b->d_pcen);
    }
    if (l.cmvn.n) {
        const size_t G = size_t(mfcc_online::kThreads / W), blocks = std::min((l.cmvn.n + G - 1) / G, cap);
        hipLaunchKernelGGL(mfcc_online::online_cmvn_kernel, dim3((unsigned)blocks), dim3(mfcc_online::kThreads), 0, h->stream,
                           b->d_ring, d_raw, s.order ? d_stat : out, desc_table<mfcc_online::Rec>(h, l.cmvn),
                           (long long)l.cmvn.n, W, b->window, b->depth, b->norm);
    }
    const float *stat = s.norm ? d_stat : d_raw;
    if (l.delta.n && mfcc_online::wide_rows(s.W))          // s.g is the wide tile's (bank_create)
        mfcc_online::launch_deltas_wide(b->d_tail, stat, out, desc_table<mfcc_online::Rec>(h, l.delta), (long long)l.delta.n, W,
                                        s.order, b->dwin, mfcc_delta::delta_scale(b->dwin),
                                        (unsigned)std::min(l.delta.n, cap), h->stream);
    else if (l.delta.n)
        hipLaunchKernelGGL(mfcc_online::online_deltas_kernel, dim3((unsigned)std::min(l.delta.n, cap)),
                           dim3(mfcc_online::kThreads), 0, h->stream, b->d_tail, stat, out,
                           desc_table<mfcc_online::Rec>(h, l.delta), (long long)l.delta.n, W, s.order, b->dwin,
                           mfcc_delta::delta_scale(b->dwin));
    if (l.carry.n)
        hipLaunchKernelGGL(mfcc_online::online_carry_kernel, dim3((unsigned)std::min(l.carry.n, cap)),
                           dim3(mfcc_online::kThreads), 0, h->stream, b->d_ring, b->d_tail, d_raw, stat,
                           desc_table<mfcc_online::Rec>(h, l.carry), (long long)l.carry.n, W, b->depth, 2 * int(s.L));
}

// The push proper: device buffers, asynchronous on the handle's stream.  Stream u's chunk is d_samples[offsets[u] - shift ..
// offsets[u + 1] - shift); cap counts elements of the bank's (expanded) rows.  The frame launch runs once over the work
// buffer as [active] channels of nfmax frames: straight into d_out when a plain bank's streams are in lockstep, else
// into the scratch behind the descriptors, and bank_passes follow.  Nothing is consumed unless MFCC_HIP_SUCCESS is returned
int bank_advance(mfcc_hip_bank *b, const int16_t *d_samples, size_t shift, const size_t *offsets, void *d_out, size_t cap,
                 size_t *frame_offsets) {
    mfcc_hip_handle *h = b->h;
    const mfcc_bank::State st = bank_state(b);
    size_t *rfo = b->raw_fo.data();
    mfcc_bank::Layout l;
    int rc = mfcc_bank::push_plan(b->s, st, offsets, b->n, d_samples != nullptr, d_out != nullptr, cap, frame_offsets,
                                  b->after.data(), b->held_after.data(), rfo, l);
    if (rc || !l.n_rec) return rc;
    // a sample format: the span offsets[0] .. offsets[n] of the chunks is decoded into the handle's scratch area in front
    // of the parking kernel, which then reads its chunks there, counted from the span's start
    const int fmt = h->sample_fmt;
    const bool dec = decodes(fmt);
    const size_t span = offsets[b->n] - offsets[0];
    const void *d_span = dec ? sample_at(fmt, d_samples, offsets[0] - shift) : nullptr;
    if (dec && !sample_aligned(fmt, d_samples)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (dec) shift = offsets[0];
    DeviceGuard guard(h->device);
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    if ((rc = desc_acquire(h, l.desc_ll, &pd))) return rc;
    mfcc_bank::push_fill(b->s, st, offsets, shift, b->n, frame_offsets, rfo, l, pd->p);
    if (l.in_bytes && (rc = ensure(h, h->d_in, l.in_bytes))) return rc;
    if (dec && (rc = ensure(h, h->d_dec, span * sizeof(int16_t) + 64))) return rc;
    if ((rc = desc_stage(h, h->d_out, l.out_bytes, pd, l.desc_ll))) return rc;
    if (dec) {
        if ((rc = decode_rows(h, fmt, d_span, span, 1, span, static_cast<int16_t *>(h->d_dec.p), span))) return rc;
        d_samples = static_cast<const int16_t *>(h->d_dec.p);
    }
    int16_t *d_w = static_cast<int16_t *>(h->d_in.p);
    const unsigned blocks = (unsigned)std::min<size_t>(l.n_rec, size_t(h->n_cu) * 8);
    hipLaunchKernelGGL(mfcc_bank::bank_advance_kernel, dim3(blocks), dim3(mfcc_bank::kThreads), 0, h->stream, d_samples,
                       b->d_state, d_w, desc_table<mfcc_bank::Rec>(h, l.bank), (long long)l.n_rec, (long long)l.n_active,
                       (long long)l.stride, h->r.frame_len, h->r.hop);
    if (l.n_active) {
        void *d_rows = l.direct ? d_out : static_cast<char *>(h->d_out.p) + l.raw_off;
        if ((rc = launch(h, call_of(h, b->kind, b->fixed), d_w, l.stride - 1, l.stride, l.n_active, /*halo=*/1, d_rows, nullptr, l.nfmax))) return rc;
        bank_passes(b, l, d_out);
    }
    HIP_TRY(h, hipGetLastError());
    if ((rc = scratch_release(h))) return rc;
    for (size_t u = 0; u < b->n; ++u) b->seen[u] += rfo[u + 1] - rfo[u];
    b->pending.swap(b->after);
    b->held.swap(b->held_after);
    return MFCC_HIP_SUCCESS;
}

// The end of the listed streams.  give: a flush, to host memory (synchronous): with the handle's pad mode STREAM the
// zero-padded tail frame (main.c:134-144: one frame over history | pending | zeros) joins each stream as its last row,
// the held rows and that one are returned with the end clamped -- fo[i + 1] - fo[i] rows of stream list[i] (fo NULL:
// not wanted).  Without give: a reset, nothing is returned.  Either way the streams are back in the reset state.  The
// ring and the tail of an online bank are not cleared: with seen = 0 nothing of them is read
int bank_end(mfcc_hip_bank *b, const std::vector<size_t> &list, bool give, void *out, size_t cap, size_t *fo) {
    mfcc_hip_handle *h = b->h;
    const mfcc_bank::State st = bank_state(b);
    const bool emit = give && h->r.pad_mode == MFCC_HIP_PAD_STREAM;
    if (!fo) fo = b->raw_fo.data();                      // list.size() <= b->n
    mfcc_bank::Layout l;
    int rc = mfcc_bank::end_plan(b->s, st, list.data(), list.size(), emit, give, out != nullptr, cap, fo, l);
    if (rc || !l.n_rec) return rc;
    const size_t result_bytes = fo[l.n_rec] * b->s.out_width() * b->s.elem;
    DeviceGuard guard(h->device);
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    if ((rc = desc_acquire(h, l.desc_ll, &pd))) return rc;
    mfcc_bank::end_fill(b->s, st, list.data(), fo, l, pd->p);
    if (l.in_bytes && (rc = ensure(h, h->d_in, l.in_bytes))) return rc;
    if (result_bytes && (rc = ensure(h, b->st_out, result_bytes + 64))) return rc;
    if ((rc = desc_stage(h, h->d_out, l.out_bytes, pd, l.desc_ll))) return rc;
    int16_t *d_w = emit ? static_cast<int16_t *>(h->d_in.p) : nullptr;
    const unsigned blocks = (unsigned)std::min<size_t>(l.n_rec, size_t(h->n_cu) * 8);
    hipLaunchKernelGGL(mfcc_bank::bank_flush_kernel, dim3(blocks), dim3(mfcc_bank::kThreads), 0, h->stream, b->d_state, d_w,
                       desc_table<mfcc_bank::Rec>(h, l.bank), (long long)l.n_rec, (long long)l.stride, h->r.frame_len);
    if (emit) {
        void *d_rows = l.direct ? b->st_out.p : static_cast<char *>(h->d_out.p) + l.raw_off;
        if ((rc = launch(h, call_of(h, b->kind, b->fixed), d_w, l.stride - 1, l.stride, l.n_active, /*halo=*/1, d_rows, nullptr, 1))) return rc;
    }
    bank_passes(b, l, b->st_out.p);
    if (result_bytes) HIP_TRY(h, hipMemcpyAsync(out, b->st_out.p, result_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipGetLastError());
    if ((rc = scratch_release(h))) return rc;
    live_zero(list, {&b->pending, &b->seen, &b->held});
    // as it has been: a plain bank waits for its tail frames, an online one after every flush
    if (emit || (give && b->s.online())) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MFCC_HIP_SUCCESS;
}

// a bank on a checked handle whose frame launch is c; norm / order as validated by the caller (NONE and 0: a plain bank)
int bank_create(mfcc_hip_handle *h, const Call &c, size_t n_streams, int norm, int window, int order, int dwin,
                mfcc_hip_bank **out, const mfcc_pcen::Prm *pcen = nullptr) {
    mfcc_hip_bank *b = live_new<mfcc_hip_bank>(h, n_streams);
    if (!b) return MFCC_HIP_ERROR_NO_MEM;
    const bool fixed = c.fixed;
    b->kind = c.kind;
    if (c.kind == Kind::kFbank) ++h->n_fbank_banks;
    b->fixed = fixed;
    b->pending.assign(n_streams, 0);
    b->after.assign(n_streams, 0);
    b->seen.assign(n_streams, 0);
    b->held.assign(n_streams, 0);
    b->held_after.assign(n_streams, 0);
    b->raw_fo.assign(n_streams + 1, 0);
    mfcc_bank::Settings &s = b->s;
    const size_t W = c.width;
    s.flen = size_t(h->r.frame_len);
    s.hop = size_t(h->r.hop);
    s.W = W;
    s.elem = fixed ? sizeof(int16_t) : sizeof(float);
    s.pcen = pcen != nullptr;
    if (pcen) b->pcen_prm = *pcen;
    if (norm != MFCC_HIP_NORMALIZE_NONE) {
        s.norm = true;
        s.S = size_t(mfcc_slide::run_rows(window));
        b->norm = norm;
        b->window = window;
        b->depth = window + int(s.S);
    }
    if (order) {
        s.order = order;
        s.L = size_t(order * dwin);
        s.g = size_t(mfcc_online::delta_tile_rows(int(W), order, dwin));
        b->dwin = dwin;
    }
    DeviceGuard guard(h->device);
    const size_t bytes = n_streams * s.flen * sizeof(int16_t);
    const size_t ring_bytes = n_streams * size_t(b->depth) * W * sizeof(float);
    const size_t tail_bytes = n_streams * 2 * s.L * W * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_state), bytes + 64);
    if (e == hipSuccess && ring_bytes) e = hipMalloc(reinterpret_cast<void **>(&b->d_ring), ring_bytes + 64);
    if (e == hipSuccess && tail_bytes) e = hipMalloc(reinterpret_cast<void **>(&b->d_tail), tail_bytes + 64);
    if (e == hipSuccess && s.pcen) {
        const size_t state_floats = n_streams * 2 * W;
        e = hipMalloc(reinterpret_cast<void **>(&b->d_pcen), (state_floats + mfcc_pcen::kTile) * sizeof(float) + 64);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b->d_pcen + state_floats, b->pcen_prm.decay, sizeof b->pcen_prm.decay, hipMemcpyHostToDevice,
                               h->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(b->d_state, 0, bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    return live_created(b, e, out);
}

// The checks the create entries share, then the bank.  The bank's settings are its own: the handle must be a raw
// one (what mfcc_hip_stream_create refuses: per-call statistics, lookahead and whole-segment thresholds of a stream)
// that can run the path asked for; an online bank (float) takes log-mel rows where it has PCEN.  A filterbank bank
// (kind kFbank, float) wants the handle's matrix instead -- in log2 where it has PCEN, which reads log2 energies --
// and the handle's own post settings do not apply to it, as on every filterbank call
int bank_create_checked(mfcc_hip_handle *h, Kind kind, int fixed, bool online, size_t n_streams, const mfcc_hip_pcen *p,
                        int normalize, int normalize_window, int delta_order, int delta_window, mfcc_hip_bank **out) {
    if (live_check(h, n_streams, out) || (p && !pcen_ok(p))) return MFCC_HIP_ERROR_INVALID_PARAM;
    const bool fb = kind == Kind::kFbank;
    // a bank takes its settings at creation and its frame launch is the raw kernel: no settings of the handle's behind it
    if (fb ? !h->fb_dev || has_post(h->fb_post) : has_post(h->post)) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (rated(h)) return MFCC_HIP_ERROR_UNSUPPORTED;           // a line's rate conversion keeps state between pushes
    if (h->center) return MFCC_HIP_ERROR_UNSUPPORTED;          // a centred line holds back PL + 1 samples, flushes several frames
    if (p && !(fb ? h->fb_scale == MFCC_HIP_FBANK_LOG2 : is_logmel(h->r))) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (fixed && h->fixed_kernel == FixedKernel::kNone) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (online && h->r.float_impl == MFCC_HIP_IMPL_FUSED512 && !is_fused512(h->float_kernel)) return MFCC_HIP_ERROR_UNSUPPORTED;
    if (normalize != MFCC_HIP_NORMALIZE_NONE && normalize != MFCC_HIP_NORMALIZE_MEAN && normalize != MFCC_HIP_NORMALIZE_MEAN_VAR)
        return MFCC_HIP_ERROR_INVALID_PARAM;
    if (normalize != MFCC_HIP_NORMALIZE_NONE && (normalize_window < 1 || normalize_window > MFCC_HIP_MAX_NORMALIZE_WINDOW))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    if (delta_order < 0 || delta_order > 2 || delta_window < 1 || delta_window > mfcc_delta::kMaxWindow)
        return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_pcen::Prm prm{};
    if (p) prm = pcen_prm(*p);
    return bank_create(h, call_of(h, kind, fixed != 0), n_streams, normalize, normalize_window, delta_order, delta_window, out,
                       p ? &prm : nullptr);
}

}  // namespace

extern "C" {

int mfcc_hip_bank_create(mfcc_hip_handle *h, int fixed, size_t n_streams, mfcc_hip_bank **out) {
    return bank_create_checked(h, Kind::kFeatures, fixed, false, n_streams, nullptr, MFCC_HIP_NORMALIZE_NONE, 0, 0, 1, out);
}

int mfcc_hip_bank_create_online(mfcc_hip_handle *h, size_t n_streams, int normalize, int normalize_window, int delta_order,
                                int delta_window, mfcc_hip_bank **out) {
    return bank_create_checked(h, Kind::kFeatures, 0, true, n_streams, nullptr, normalize, normalize_window, delta_order,
                               delta_window, out);
}

// p == NULL: no PCEN, mfcc_hip_bank_create_online
int mfcc_hip_bank_create_online_pcen(mfcc_hip_handle *h, size_t n_streams, const mfcc_hip_pcen *p, int normalize,
                                     int normalize_window, int delta_order, int delta_window, mfcc_hip_bank **out) {
    return bank_create_checked(h, Kind::kFeatures, 0, true, n_streams, p, normalize, normalize_window, delta_order, delta_window,
                               out);
}

// the rows are the handle's filterbank rows; p == NULL: no PCEN
int mfcc_hip_bank_create_filterbank(mfcc_hip_handle *h, size_t n_streams, const mfcc_hip_pcen *p, int normalize, int normalize_window,
                               int delta_order, int delta_window, mfcc_hip_bank **out) {
    return bank_create_checked(h, Kind::kFbank, 0, true, n_streams, p, normalize, normalize_window, delta_order, delta_window,
                               out);
}

size_t mfcc_hip_bank_row_width(const mfcc_hip_bank *b) { return b ? b->s.out_width() : 0; }

int mfcc_hip_bank_lag(const mfcc_hip_bank *b) { return b ? int(b->s.L) : 0; }

int mfcc_hip_bank_held(const mfcc_hip_bank *b, size_t *held) { return live_counts(b, &mfcc_hip_bank::held, held); }

int mfcc_hip_bank_plan_online(const mfcc_hip_params *p, int lag, const size_t *pending, const size_t *held,
                              const size_t *offsets, size_t n_streams, size_t *frame_offsets, size_t *pending_after,
                              size_t *held_after) {
    return mfcc_hip_bank_plan_online_framed(p, 0, lag, pending, held, offsets, n_streams, frame_offsets, pending_after,
                                            held_after);
}

int mfcc_hip_bank_plan_online_framed(const mfcc_hip_params *p, int frame_length, int lag, const size_t *pending,
                                     const size_t *held, const size_t *offsets, size_t n_streams, size_t *frame_offsets,
                                     size_t *pending_after, size_t *held_after) {
    if (!p || lag < 0 || !pending || !held || !offsets || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    Resolved r;
    const int rc = resolve_framed(p, frame_length, r);
    if (rc) return rc;
    return mfcc_bank::plan_streams(size_t(r.frame_len), size_t(r.hop), size_t(lag), pending, held, offsets, n_streams,
                                   frame_offsets, pending_after, held_after, nullptr);
}

int mfcc_hip_bank_flush_ragged(mfcc_hip_bank *b, const size_t *streams, size_t n, void *out, size_t out_capacity,
                               size_t *frame_offsets) {
    if (!b || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::vector<size_t> list;
    const int rc = live_lines(b->n, streams, n, list);
    return rc ? rc : bank_end(b, list, true, out, out_capacity, frame_offsets);
}

void mfcc_hip_bank_destroy(mfcc_hip_bank *b) { live_destroy(b); }

size_t mfcc_hip_bank_size(const mfcc_hip_bank *b) { return b ? b->n : 0; }

int mfcc_hip_bank_pending(const mfcc_hip_bank *b, size_t *pending) { return live_counts(b, &mfcc_hip_bank::pending, pending); }

int mfcc_hip_bank_plan(const mfcc_hip_params *p, const size_t *pending, const size_t *offsets, size_t n_streams,
                       size_t *frame_offsets, size_t *pending_after) {
    return mfcc_hip_bank_plan_framed(p, 0, pending, offsets, n_streams, frame_offsets, pending_after);
}

int mfcc_hip_bank_plan_framed(const mfcc_hip_params *p, int frame_length, const size_t *pending, const size_t *offsets,
                              size_t n_streams, size_t *frame_offsets, size_t *pending_after) {
    if (!p || !pending || !offsets || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    Resolved r;
    const int rc = resolve_framed(p, frame_length, r);
    if (rc) return rc;
    return mfcc_bank::plan_streams(size_t(r.frame_len), size_t(r.hop), 0, pending, nullptr, offsets, n_streams, frame_offsets,
                                   pending_after, nullptr, nullptr);
}

int mfcc_hip_bank_push_dev(mfcc_hip_bank *b, const void *d_samples, const size_t *offsets, void *d_out, size_t out_capacity,
                           size_t *frame_offsets) {
    if (!b || !offsets || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    return bank_advance(b, static_cast<const int16_t *>(d_samples), 0, offsets, d_out, out_capacity, frame_offsets);
}

int mfcc_hip_bank_push(mfcc_hip_bank *b, const int16_t *samples, const size_t *offsets, void *out, size_t out_capacity,
                       size_t *frame_offsets) {
    if (!b || !offsets || !frame_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = b->h;
    const size_t W = b->s.out_width(), esz = b->s.elem;
    // the plan first: a refused push must not have copied anything
    int rc = mfcc_bank::plan_streams(b->s.flen, b->s.hop, b->s.L, b->pending.data(), b->held.data(), offsets, b->n, frame_offsets,
                                     nullptr, nullptr, nullptr);
    if (rc) return rc;
    const size_t total = frame_offsets[b->n], span = offsets[b->n] - offsets[0];
    if (total && (!out || out_capacity < total * W)) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (!span) return MFCC_HIP_SUCCESS;
    if (!samples) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    const size_t raw = span * sample_bytes(h->sample_fmt);              // the chunks as they are: the device push decodes them
    if ((rc = ensure(h, b->st_in, raw + 64))) return rc;
    if ((rc = ensure(h, b->st_out, total * W * esz + 64))) return rc;
    HIP_TRY(h, hipMemcpyAsync(b->st_in.p, sample_at(h->sample_fmt, samples, offsets[0]), raw, hipMemcpyHostToDevice, h->stream));
    rc = bank_advance(b, static_cast<const int16_t *>(b->st_in.p), offsets[0], offsets, b->st_out.p, total * W, frame_offsets);
    if (!rc && total) HIP_TRY(h, hipMemcpyAsync(out, b->st_out.p, total * W * esz, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));        // `samples` and `out` belong to the caller again
    return rc;
}

int mfcc_hip_bank_flush(mfcc_hip_bank *b, const size_t *streams, size_t n, void *out, size_t out_capacity,
                        size_t *n_frames_out) {
    if (!b) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::vector<size_t> list;
    const int rc = live_lines(b->n, streams, n, list);
    if (rc) return rc;
    if (b->s.L > 0) return MFCC_HIP_ERROR_UNSUPPORTED;      // ragged output: mfcc_hip_bank_flush_ragged
    if (n_frames_out) *n_frames_out = b->h->r.pad_mode == MFCC_HIP_PAD_STREAM ? list.size() : 0;
    return bank_end(b, list, true, out, out_capacity, nullptr);
}

int mfcc_hip_bank_reset(mfcc_hip_bank *b, const size_t *streams, size_t n) {
    if (!b) return MFCC_HIP_ERROR_INVALID_PARAM;
    std::vector<size_t> list;
    const int rc = live_lines(b->n, streams, n, list);
    return rc ? rc : bank_end(b, list, false, nullptr, 0, nullptr);
}

}  // extern "C"

// ---- the receiver's power gate and window extraction on int16 rows (kernel_gate.hpp, DESIGN.md sections 4.10 and
// 6c-quater).  The one-shot entries tile the WINDOW index space of the segments; the tracker keeps a ring of rows per
// line on the device and its frame counts on the host.
struct mfcc_hip_gate {
    mfcc_hip_handle *h = nullptr;
    size_t n = 0;                        // lines
    mfcc_gate::Geo g{};
    int D = 0;                           // ring depth: n_frames + stride - 1
    long long threshold = 0;
    int16_t *d_ring = nullptr;           // [n][D][n_cep]
    std::vector<size_t> seen;            // frames since create / reset: depends on chunk lengths only
    std::vector<void *> owned() const { return {d_ring}; }
};

namespace {

inline size_t gate_windows(size_t T, size_t n_frames, size_t stride) {
    return T >= n_frames ? (T - n_frames) / stride + 1 : 0;
}

inline bool gate_shape_ok(int n_cep, int n_frames, int stride) {
    return n_cep >= 1 && n_cep <= mfcc_gate::kMaxWidth && n_frames >= 1 && n_frames <= MFCC_HIP_MAX_GATE_WINDOW &&
           stride >= 1 && stride <= MFCC_HIP_MAX_GATE_WINDOW;
}

// win_offsets (n_segs + 1) of segments off; INVALID_PARAM where off decreases
int gate_count(size_t n_frames, size_t stride, const size_t *off, size_t n_segs, size_t *win_offsets) {
    win_offsets[0] = 0;
    for (size_t k = 0; k < n_segs; ++k) {
        if (off[k + 1] < off[k]) return MFCC_HIP_ERROR_INVALID_PARAM;
        win_offsets[k + 1] = win_offsets[k] + gate_windows(off[k + 1] - off[k], n_frames, stride);
    }
    return MFCC_HIP_SUCCESS;
}

// The tiles of tw windows of segments off[0 .. n_segs] (rows; wo their window offsets, wo[n_segs] > 0), staged in
// h->d_sel behind `areas`: a plan over the window index space whose extra column is delta[k] = off[k] - wo[k] * stride
int gate_stage(mfcc_hip_handle *h, const size_t *off, const size_t *wo, size_t n_segs, size_t stride, size_t tw,
               const Area *areas, int n_areas, Staged &st, mfcc_gate::Wins &w) {
    const Column delta{off, stride};
    const int rc = seg_stage(h, span_offsets(wo, n_segs), 1, int(tw), &delta, h->d_sel, areas, n_areas, st);
    if (rc) return rc;
    const bool equal = !st.s.blk;                      // equal segments: their rows, as first_row() steps through them
    w = mfcc_gate::Wins{st.s, st.extra, equal ? (long long)off[0] : 0, equal ? (long long)(off[1] - off[0]) : 0};
    return MFCC_HIP_SUCCESS;
}

inline unsigned gate_grid(const mfcc_hip_handle *h, long long want) {
    return unsigned(std::max<long long>(1, std::min<long long>(want, (long long)h->n_cu * 8)));
}

}  // namespace

extern "C" {

int mfcc_hip_eval_power32(const int16_t *window, int n_cep, int n_frames, size_t head, int32_t *power_out) {
    if (!window || n_cep <= 0 || n_frames <= 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t size = size_t(n_cep) * size_t(n_frames);
    if (head >= size) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t first = 1 * size / 3, last = 2 * size / 3;
    uint32_t acc = 0;                                  // the reference's `int power`, wrapping as two's complement
    for (size_t i = first; i < last; i += size_t(n_cep)) {
        size_t k = head + i;
        if (k >= size) k -= size;
        acc += uint32_t(int32_t(window[k]) * int32_t(window[k]));
    }
    const int32_t power = int32_t(acc);
    if (power_out) *power_out = power;
    return power >= 100000000 ? 1 : 0;                 // POWER_THRESHOLD, cepstrum.c:13
}

int mfcc_hip_gate_count(int n_frames, int stride, const size_t *seg_offsets, size_t n_segs, size_t *win_offsets) {
    if (!gate_shape_ok(1, n_frames, stride) || !win_offsets || (n_segs && !seg_offsets)) return MFCC_HIP_ERROR_INVALID_PARAM;
    return gate_count(size_t(n_frames), size_t(stride), seg_offsets, n_segs, win_offsets);
}

int mfcc_hip_gate_dev(mfcc_hip_handle *h, const void *d_rows, int n_cep, const size_t *seg_offsets, size_t n_segs,
                      int n_frames, int stride, long long threshold, void *d_power, void *d_gate, void *d_gate_ref) {
    static_assert(MFCC_HIP_MAX_GATE_WINDOW == mfcc_gate::kMaxWindow, "window limit");
    if (!h || !gate_shape_ok(n_cep, n_frames, stride) || threshold < 0 || (n_segs && !seg_offsets))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    std::vector<size_t> wo(n_segs + 1);
    int rc = gate_count(size_t(n_frames), size_t(stride), seg_offsets, n_segs, wo.data());
    if (rc) return rc;
    // the rows read and the entries written (one per window; an output may be NULL) must not overlap each other.  No
    // window: nothing to write, the pointers are not looked at
    const RowPtr ptr[] = {{d_rows, 2, size_t(n_cep) * sizeof(int16_t), kRead, false},
                          {d_power, 8, sizeof(long long), kWritePacked, true},
                          {d_gate, 1, 1, kWritePacked, true},
                          {d_gate_ref, 1, 1, kWritePacked, true}};
    rc = check_rows(RowCall{n_cep, mfcc_gate::kMaxWidth, seg_offsets, n_segs, wo.data(), ptr, 4});
    if (rc != kProceed) return rc < 0 ? rc : MFCC_HIP_SUCCESS;
    if (!d_power && !d_gate && !d_gate_ref) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    const mfcc_gate::Geo g = mfcc_gate::geometry(n_cep, n_frames, stride);
    Staged st;
    mfcc_gate::Wins w;
    if ((rc = gate_stage(h, seg_offsets, wo.data(), n_segs, size_t(stride), size_t(mfcc_gate::power_tile_wins(g.K, stride)),
                         nullptr, 0, st, w)))
        return rc;
    hipLaunchKernelGGL(mfcc_gate::gate_power_kernel, dim3(gate_grid(h, w.s.n_blocks)), dim3(mfcc_gate::kThreads), 0, h->stream,
                       static_cast<const int16_t *>(d_rows), w, g, threshold, static_cast<long long *>(d_power),
                       static_cast<unsigned char *>(d_gate), static_cast<unsigned char *>(d_gate_ref));
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

int mfcc_hip_gate_windows_dev(mfcc_hip_handle *h, const void *d_rows, int n_cep, const size_t *seg_offsets, size_t n_segs,
                              int n_frames, int stride, const void *d_mask, void *d_out, void *d_starts,
                              size_t out_capacity_windows, size_t *out_offsets) {
    if (!h || !gate_shape_ok(n_cep, n_frames, stride) || (n_segs && (!seg_offsets || !out_offsets)))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    std::vector<size_t> wo(n_segs + 1);
    int rc = gate_count(size_t(n_frames), size_t(stride), seg_offsets, n_segs, wo.data());
    if (rc) return rc;
    const size_t total = wo[n_segs];
    // how much is written is not known yet: the outputs' alignment now, their ranges below
    const size_t row_bytes = size_t(n_cep) * sizeof(int16_t);
    const RowPtr ptr[] = {{d_rows, 2, row_bytes, kRead, false}, {d_mask, 1, 1, kRead, false},
                          {d_out, 2, 0, kUnsized, true}, {d_starts, 8, 0, kUnsized, true}};
    rc = check_rows(RowCall{n_cep, mfcc_gate::kMaxWidth, seg_offsets, n_segs, wo.data(), ptr, 4});
    if (rc == kNothing) {
        for (size_t k = 0; k <= n_segs && out_offsets; ++k) out_offsets[k] = 0;
        return MFCC_HIP_SUCCESS;
    }
    if (rc != kProceed) return rc;
    DeviceGuard guard(h->device);
    const mfcc_gate::Geo g = mfcc_gate::geometry(n_cep, n_frames, stride);
    Staged st;
    mfcc_gate::Wins w;
    if ((rc = gate_stage(h, seg_offsets, wo.data(), n_segs, size_t(stride), size_t(mfcc_gate::kSelTileWins),
                         kSelectAreas, 3, st, w)))
        return rc;
    const SelPlan sel = sel_plan_of(st);
    const unsigned grid = gate_grid(h, w.s.n_blocks);
    const unsigned char *mask = static_cast<const unsigned char *>(d_mask);
    // counts and prefix over the window index space: the selection's own kernels, which only need tile_of
    hipLaunchKernelGGL(mfcc_vad::vad_count_kernel, dim3(grid), dim3(mfcc_vad::kThreads), 0, h->stream, mask, w.s, sel.counts);
    hipLaunchKernelGGL(mfcc_vad::vad_scan_kernel, dim3(1), dim3(mfcc_vad::kScanThreads), 0, h->stream, w.s,
                       static_cast<const unsigned *>(sel.counts), sel.tile_off, sel.seg_off);
    HIP_TRY(h, hipGetLastError());
    static_assert(sizeof(size_t) == sizeof(long long), "segment offsets are copied as they are");
    HIP_TRY(h, hipMemcpyAsync(out_offsets, sel.seg_off, (n_segs + 1) * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the count depends on the data
    const size_t n_sel = out_offsets[n_segs];
    rc = MFCC_HIP_SUCCESS;
    if (out_capacity_windows < n_sel) {
        rc = MFCC_HIP_ERROR_BUFFER_SMALL;
    } else if (n_sel) {
        // what is read must not overlap what is written
        const size_t win_bytes = size_t(n_frames) * row_bytes;
        const uintptr_t in_lo = reinterpret_cast<uintptr_t>(d_rows) + seg_offsets[0] * row_bytes;
        const uintptr_t in_hi = reinterpret_cast<uintptr_t>(d_rows) + seg_offsets[n_segs] * row_bytes;
        const uintptr_t m_lo = reinterpret_cast<uintptr_t>(d_mask), m_hi = m_lo + total;
        const uintptr_t o_lo = reinterpret_cast<uintptr_t>(d_out), o_hi = o_lo + n_sel * win_bytes;
        const uintptr_t s_lo = reinterpret_cast<uintptr_t>(d_starts), s_hi = s_lo + n_sel * sizeof(long long);
        if (!d_out || ranges_overlap(in_lo, in_hi, o_lo, o_hi) || ranges_overlap(m_lo, m_hi, o_lo, o_hi) ||
            (d_starts && (ranges_overlap(in_lo, in_hi, s_lo, s_hi) || ranges_overlap(m_lo, m_hi, s_lo, s_hi) ||
                          ranges_overlap(o_lo, o_hi, s_lo, s_hi))))
            rc = MFCC_HIP_ERROR_INVALID_PARAM;
        else
            hipLaunchKernelGGL(mfcc_gate::gate_gather_kernel, dim3(grid), dim3(mfcc_gate::kThreads), 0, h->stream,
                               static_cast<const int16_t *>(d_rows), mask, w, g, static_cast<const long long *>(sel.tile_off),
                               static_cast<int16_t *>(d_out), static_cast<long long *>(d_starts));
    }
    const int rc2 = scratch_release(h);
    if (rc) return rc;
    HIP_TRY(h, hipGetLastError());
    return rc2;
}

int mfcc_hip_gate_plan(int n_frames, int stride, const size_t *seen, const size_t *frame_offsets, size_t n_lines,
                       size_t *win_offsets, size_t *seen_after) {
    if (!gate_shape_ok(1, n_frames, stride) || !win_offsets || (n_lines && (!seen || !frame_offsets)))
        return MFCC_HIP_ERROR_INVALID_PARAM;
    win_offsets[0] = 0;
    for (size_t u = 0; u < n_lines; ++u) {
        if (frame_offsets[u + 1] < frame_offsets[u]) return MFCC_HIP_ERROR_INVALID_PARAM;
        const size_t after = seen[u] + (frame_offsets[u + 1] - frame_offsets[u]);
        // the windows whose last row is one of the new ones: those of `after` rows that `seen` rows did not have
        win_offsets[u + 1] = win_offsets[u] + gate_windows(after, size_t(n_frames), size_t(stride)) -
                             gate_windows(seen[u], size_t(n_frames), size_t(stride));
        if (seen_after) seen_after[u] = after;
    }
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_gate_create(mfcc_hip_handle *h, size_t n_lines, int n_cep, int n_frames, int stride, long long threshold,
                         mfcc_hip_gate **out) {
    if (live_check(h, n_lines, out) || !gate_shape_ok(n_cep, n_frames, stride) || threshold < 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_gate *g = live_new<mfcc_hip_gate>(h, n_lines);
    if (!g) return MFCC_HIP_ERROR_NO_MEM;
    g->g = mfcc_gate::geometry(n_cep, n_frames, stride);
    g->D = n_frames + stride - 1;
    g->threshold = threshold;
    g->seen.assign(n_lines, 0);
    DeviceGuard guard(h->device);
    return live_created(g, hipMalloc(reinterpret_cast<void **>(&g->d_ring), n_lines * size_t(g->D) * size_t(n_cep) * sizeof(int16_t) + 64), out);
}

void mfcc_hip_gate_destroy(mfcc_hip_gate *g) { live_destroy(g); }

int mfcc_hip_gate_seen(const mfcc_hip_gate *g, size_t *seen) { return live_counts(g, &mfcc_hip_gate::seen, seen); }

int mfcc_hip_gate_push_dev(mfcc_hip_gate *g, const void *d_rows, const size_t *frame_offsets, void *d_power, void *d_gate,
                           void *d_gate_ref, size_t capacity_windows, size_t *win_offsets) {
    if (!g || !frame_offsets || !win_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = g->h;
    const mfcc_gate::Geo &geo = g->g;
    const size_t n = g->n, nfr = size_t(geo.n_frames), stride = size_t(geo.stride);
    int rc = mfcc_hip_gate_plan(geo.n_frames, geo.stride, g->seen.data(), frame_offsets, n, win_offsets, nullptr);
    if (rc) return rc;
    const size_t total = win_offsets[n];
    if (total && !d_power && !d_gate && !d_gate_ref) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (reinterpret_cast<uintptr_t>(d_power) & 7) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (capacity_windows < total) return MFCC_HIP_ERROR_BUFFER_SMALL;
    size_t n_rec = 0, nwmax = 0;
    for (size_t u = 0; u < n; ++u) {
        if (frame_offsets[u + 1] == frame_offsets[u]) continue;
        ++n_rec;
        nwmax = std::max(nwmax, win_offsets[u + 1] - win_offsets[u]);
    }
    if (!n_rec) return MFCC_HIP_SUCCESS;
    if (!d_rows || (reinterpret_cast<uintptr_t>(d_rows) & 1)) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    static_assert(sizeof(mfcc_gate::Rec) == mfcc_gate::kRecLL * sizeof(long long), "record layout");
    const size_t rec_ll = mfcc_gate::kRecLL * n_rec;
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    if ((rc = desc_acquire(h, rec_ll, &pd))) return rc;
    auto *rec = reinterpret_cast<mfcc_gate::Rec *>(pd->p);
    size_t a = 0;
    for (size_t u = 0; u < n; ++u) {
        const size_t nf = frame_offsets[u + 1] - frame_offsets[u];
        if (!nf) continue;
        rec[a++] = mfcc_gate::Rec{(long long)u, (long long)frame_offsets[u], (long long)g->seen[u], (long long)nf,
                                  (long long)gate_windows(g->seen[u], nfr, stride),
                                  (long long)(win_offsets[u + 1] - win_offsets[u]), (long long)win_offsets[u], 0};
    }
    // the records at the front of h->d_out, as the banks keep theirs
    if ((rc = desc_stage(h, h->d_out, rec_ll * sizeof(long long) + 64, pd, rec_ll))) return rc;
    auto *d_rec = static_cast<const mfcc_gate::Rec *>(h->d_out.p);
    const int16_t *fresh = static_cast<const int16_t *>(d_rows);
    if (nwmax)
        hipLaunchKernelGGL(mfcc_gate::gate_live_kernel,
                           dim3(gate_grid(h, (long long)((n_rec * nwmax + mfcc_gate::kThreads - 1) / mfcc_gate::kThreads))),
                           dim3(mfcc_gate::kThreads), 0, h->stream, static_cast<const int16_t *>(g->d_ring), fresh, d_rec,
                           (long long)n_rec, (long long)nwmax, geo, g->D, g->threshold, static_cast<long long *>(d_power),
                           static_cast<unsigned char *>(d_gate), static_cast<unsigned char *>(d_gate_ref));
    hipLaunchKernelGGL(mfcc_gate::gate_carry_kernel, dim3(gate_grid(h, (long long)n_rec)), dim3(mfcc_gate::kThreads), 0,
                       h->stream, g->d_ring, fresh, d_rec, (long long)n_rec, geo.n_cep, g->D);
    HIP_TRY(h, hipGetLastError());
    if ((rc = scratch_release(h))) return rc;
    for (size_t u = 0; u < n; ++u) g->seen[u] += frame_offsets[u + 1] - frame_offsets[u];
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_gate_reset(mfcc_hip_gate *g, const size_t *lines, size_t n) { return live_reset(g, lines, n, &mfcc_hip_gate::seen); }

int mfcc_hip_gate_window_dev(mfcc_hip_gate *g, const size_t *lines, size_t n, void *d_out) {
    if (!g || (n && !lines)) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = g->h;
    const mfcc_gate::Geo &geo = g->g;
    if (!n) return MFCC_HIP_SUCCESS;
    std::vector<size_t> list;
    if (live_lines(g->n, lines, n, list)) return MFCC_HIP_ERROR_INVALID_PARAM;
    for (size_t u : list)
        if (g->seen[u] < size_t(geo.n_frames)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 1)) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    const size_t rec_ll = 2 * n;
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    int rc = desc_acquire(h, rec_ll, &pd);
    if (rc) return rc;
    auto *rec = reinterpret_cast<mfcc_gate::WinRec *>(pd->p);
    for (size_t i = 0; i < n; ++i) {
        const size_t last = gate_windows(g->seen[lines[i]], size_t(geo.n_frames), size_t(geo.stride)) - 1;
        rec[i] = mfcc_gate::WinRec{(long long)lines[i], (long long)(last * size_t(geo.stride))};
    }
    if ((rc = desc_stage(h, h->d_out, rec_ll * sizeof(long long) + 64, pd, rec_ll))) return rc;
    hipLaunchKernelGGL(mfcc_gate::gate_window_kernel, dim3(gate_grid(h, (long long)n)), dim3(mfcc_gate::kThreads), 0, h->stream,
                       static_cast<const int16_t *>(g->d_ring), static_cast<const mfcc_gate::WinRec *>(h->d_out.p), (long long)n,
                       geo, g->D, static_cast<int16_t *>(d_out));
    HIP_TRY(h, hipGetLastError());
    return scratch_release(h);
}

// ---- live lines (include/mfcc_hip.h: mfcc_hip_resampler): the streaming form of the rule.  A line keeps the count of
// its samples on the host and its last K - 1 samples on the device, in two buffers used in turn
struct mfcc_hip_resampler {
    mfcc_hip_handle *h = nullptr;
    size_t n = 0;                        // lines
    int fmt = MFCC_HIP_SAMPLE_S16, in_rate = 0, out_rate = 0;
    mfcc_rs::Geometry g;
    int16_t *d_taps = nullptr;           // the ratio's table
    int16_t *d_hist = nullptr;           // [n][2][hist_stride]
    size_t hist_stride = 0;              // K - 1 rounded up to 8
    std::vector<size_t> seen;            // samples since create / reset / flush: depends on chunk lengths only
    std::vector<unsigned char> cur;      // which of a line's two buffers holds its history
    std::vector<void *> owned() const { return {d_taps, d_hist}; }
};

namespace {

// out_offsets of a push (flush = 0: every line's chunk offsets[u] .. offsets[u + 1] on top of seen[u]) or of a flush behind
// it (flush != 0; offsets NULL: no chunks).  INVALID_PARAM where the offsets decrease or a line grows over the limit
int rs_stream_plan(const mfcc_rs::Geometry &g, const size_t *seen, const size_t *offsets, size_t n_lines, int flush,
                   size_t *out_offsets) {
    out_offsets[0] = 0;
    for (size_t u = 0; u < n_lines; ++u) {
        if (offsets && offsets[u + 1] < offsets[u]) return MFCC_HIP_ERROR_INVALID_PARAM;
        const size_t len = offsets ? offsets[u + 1] - offsets[u] : 0;
        if (seen[u] >= mfcc_rs::kMaxLen || len >= mfcc_rs::kMaxLen - seen[u]) return MFCC_HIP_ERROR_INVALID_PARAM;
        const size_t c = seen[u] + len;
        const size_t k = flush ? size_t(mfcc_rs::count(c, g.L, g.M) - mfcc_rs::emitted(c, g.L, g.M, g.H))
                               : size_t(mfcc_rs::emitted(c, g.L, g.M, g.H) - mfcc_rs::emitted(seen[u], g.L, g.M, g.H));
        out_offsets[u + 1] = out_offsets[u] + k;
    }
    return MFCC_HIP_SUCCESS;
}

// the segments of a push or a flush in one launch: the records through the pinned pool into h->d_rs
int rs_stream_launch(mfcc_hip_resampler *r, const std::vector<mfcc_rs::SegIn> &segs) {
    mfcc_hip_handle *h = r->h;
    mfcc_rs::CallPlan pl;
    if (!mfcc_rs::plan_call(segs.data(), segs.size(), pl)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (!pl.n_tiles) return MFCC_HIP_SUCCESS;
    mfcc_hip_handle::PinnedDesc *pd = nullptr;
    int rc = desc_acquire(h, pl.total_ll, &pd);
    if (rc) return rc;
    mfcc_rs::fill_call(segs.data(), segs.size(), pl, pd->p);
    if ((rc = desc_stage(h, h->d_rs, pl.bytes, pd, pl.total_ll))) return rc;
    const mfcc_rs::Taps a{r->d_taps, r->g.L, r->g.M, r->g.H, r->g.K};
    mfcc_rs::launch(a, nullptr, 0, nullptr, 0, (long long)segs.size(), 0, 0, static_cast<const long long *>(h->d_rs.p),
                    (long long)pl.n_tiles, h->n_cu, h->stream);
    HIP_TRY(h, hipGetLastError());
    return MFCC_HIP_SUCCESS;
}

inline int16_t *rs_hist(const mfcc_hip_resampler *r, size_t line, int which) {
    return r->d_hist + (2 * line + size_t(which)) * r->hist_stride;
}

}  // namespace

int mfcc_hip_resampler_plan(int in_rate, int out_rate, const size_t *seen, const size_t *offsets, size_t n_lines, int flush,
                            size_t *out_offsets) {
    mfcc_rs::Geometry g;
    const int rc = rs_geometry(in_rate, out_rate, g);
    if (rc) return rc;
    if (!out_offsets || (n_lines && !seen) || (!flush && n_lines && !offsets)) return MFCC_HIP_ERROR_INVALID_PARAM;
    return rs_stream_plan(g, seen, offsets, n_lines, flush, out_offsets);
}

int mfcc_hip_resampler_create(mfcc_hip_handle *h, size_t n_lines, int sample_format, int in_rate, int out_rate,
                              mfcc_hip_resampler **out) {
    if (live_check(h, n_lines, out) || !mfcc_decode::known(sample_format)) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (h->center) return MFCC_HIP_ERROR_UNSUPPORTED;          // its lines feed a bank, and a centred handle has none
    mfcc_rs::Geometry g;
    std::vector<int16_t> t;
    const int rc = rs_table(in_rate, out_rate, g, t);
    if (rc) return rc;
    mfcc_hip_resampler *r = live_new<mfcc_hip_resampler>(h, n_lines);
    if (!r) return MFCC_HIP_ERROR_NO_MEM;
    r->fmt = sample_format;
    r->in_rate = in_rate;
    r->out_rate = out_rate;
    r->g = g;
    r->hist_stride = (size_t(g.K) - 1 + 7) & ~size_t(7);
    r->seen.assign(n_lines, 0);
    r->cur.assign(n_lines, 0);
    DeviceGuard guard(h->device);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&r->d_taps), t.size() * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&r->d_hist), 2 * n_lines * r->hist_stride * sizeof(int16_t));
    if (e == hipSuccess) e = hipMemcpy(r->d_taps, t.data(), t.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    return live_created(r, e, out);
}

void mfcc_hip_resampler_destroy(mfcc_hip_resampler *r) { live_destroy(r); }

int mfcc_hip_resampler_seen(const mfcc_hip_resampler *r, size_t *seen) { return live_counts(r, &mfcc_hip_resampler::seen, seen); }

int mfcc_hip_resampler_reset(mfcc_hip_resampler *r, const size_t *lines, size_t n) {
    return live_reset(r, lines, n, &mfcc_hip_resampler::seen);
}

int mfcc_hip_resampler_push_dev(mfcc_hip_resampler *r, const void *d_in, const size_t *offsets, void *d_out, size_t cap,
                                size_t *out_offsets) {
    if (!r || !offsets || !out_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = r->h;
    const mfcc_rs::Geometry &g = r->g;
    int rc = rs_stream_plan(g, r->seen.data(), offsets, r->n, 0, out_offsets);
    if (rc) return rc;
    const size_t span = offsets[r->n] - offsets[0], ssz = mfcc_decode::sample_size(r->fmt);
    if (cap < out_offsets[r->n]) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (!span) return MFCC_HIP_SUCCESS;
    if (!d_in || (reinterpret_cast<uintptr_t>(d_in) & (ssz - 1))) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (out_offsets[r->n] && (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 1))) return MFCC_HIP_ERROR_INVALID_PARAM;
    DeviceGuard guard(h->device);
    // the chunks as int16: decoded in front, like a bank's push
    const int16_t *src = static_cast<const int16_t *>(d_in) + offsets[0];
    if (r->fmt != MFCC_HIP_SAMPLE_S16) {
        if ((rc = ensure(h, h->d_dec, span * sizeof(int16_t) + 64)) || (rc = scratch_acquire(h))) return rc;
        if (!mfcc_decode::launch(r->fmt, static_cast<const char *>(d_in) + offsets[0] * ssz, static_cast<int16_t *>(h->d_dec.p), span,
                                 1, span, span, h->n_cu, h->stream))
            return MFCC_HIP_ERROR_INVALID_PARAM;
        HIP_TRY(h, hipGetLastError());
        src = static_cast<const int16_t *>(h->d_dec.p);
    }
    std::vector<mfcc_rs::SegIn> segs;
    segs.reserve(r->n);
    for (size_t u = 0; u < r->n; ++u) {
        const size_t len = offsets[u + 1] - offsets[u];
        if (!len) continue;
        mfcc_rs::SegIn s;
        s.in = reinterpret_cast<uintptr_t>(src + (offsets[u] - offsets[0]));
        s.n = len;
        s.out = reinterpret_cast<uintptr_t>(static_cast<int16_t *>(d_out) + out_offsets[u]);
        s.c0 = r->seen[u];
        s.m0 = mfcc_rs::emitted(r->seen[u], g.L, g.M, g.H);
        s.m1 = mfcc_rs::emitted(r->seen[u] + len, g.L, g.M, g.H);
        s.hist = r->seen[u] ? reinterpret_cast<uintptr_t>(rs_hist(r, u, r->cur[u])) : 0;      // a fresh line: zeros
        s.hist_new = reinterpret_cast<uintptr_t>(rs_hist(r, u, r->cur[u] ^ 1));
        segs.push_back(s);
    }
    if ((rc = rs_stream_launch(r, segs)) || (rc = scratch_release(h))) return rc;
    for (size_t u = 0; u < r->n; ++u) {
        const size_t len = offsets[u + 1] - offsets[u];
        if (!len) continue;
        r->seen[u] += len;
        r->cur[u] ^= 1;
    }
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_resampler_flush_dev(mfcc_hip_resampler *r, const size_t *lines, size_t n, void *d_out, size_t cap,
                                 size_t *out_offsets) {
    if (!r || !out_offsets) return MFCC_HIP_ERROR_INVALID_PARAM;
    mfcc_hip_handle *h = r->h;
    const mfcc_rs::Geometry &g = r->g;
    std::vector<size_t> list;                           // lines == NULL: every line
    int rc = live_lines(r->n, lines, n, list);
    if (rc) return rc;
    std::vector<size_t> seen(list.size());
    for (size_t i = 0; i < list.size(); ++i) seen[i] = r->seen[list[i]];
    if ((rc = rs_stream_plan(g, seen.data(), nullptr, list.size(), 1, out_offsets))) return rc;
    const size_t total = out_offsets[list.size()];
    if (cap < total) return MFCC_HIP_ERROR_BUFFER_SMALL;
    if (total && (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 1))) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (total) {
        DeviceGuard guard(h->device);
        std::vector<mfcc_rs::SegIn> segs;
        for (size_t i = 0; i < list.size(); ++i) {
            if (out_offsets[i + 1] == out_offsets[i]) continue;
            mfcc_rs::SegIn s;                                           // no chunk: the history, then zeros
            s.out = reinterpret_cast<uintptr_t>(static_cast<int16_t *>(d_out) + out_offsets[i]);
            s.c0 = seen[i];
            s.m0 = mfcc_rs::emitted(seen[i], g.L, g.M, g.H);
            s.m1 = mfcc_rs::count(seen[i], g.L, g.M);
            s.hist = reinterpret_cast<uintptr_t>(rs_hist(r, list[i], r->cur[list[i]]));
            segs.push_back(s);
        }
        if ((rc = rs_stream_launch(r, segs)) || (rc = scratch_release(h))) return rc;
    }
    live_zero(list, {&r->seen});
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_lift_file(const char *mfcc_in, const char *lift_out, int n_cep, double L, size_t *n_frames_out) {
    if (!mfcc_in || !lift_out || n_cep <= 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    FILE *f = std::fopen(mfcc_in, "rb");
    if (!f) return MFCC_HIP_ERROR_IO;
    std::vector<int16_t> v;
    int16_t buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(int16_t), 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    if (v.size() % size_t(n_cep)) return MFCC_HIP_ERROR_INVALID_PARAM;       // np.reshape(raw, (-1, NCEPSTRUMS)) would raise
    std::vector<double> lift(n_cep, 1.0);
    if (L > 0.0)
        for (int n = 0; n < n_cep; ++n) lift[n] = 1.0 + (L / 2.0) * std::sin(mfcc_tables::kPi * double(n) / L);
    for (size_t i = 0; i < v.size(); ++i) {
        // lift.py:39: (lift * cepstra).astype(np.int16) -- truncation toward zero; a value beyond int16 keeps
        // its low 16 bits (C conversion through a wider integer, what NumPy does on x86-64)
        const double x = lift[i % size_t(n_cep)] * double(v[i]);
        v[i] = int16_t(uint16_t(int64_t(x)));
    }
    FILE *o = std::fopen(lift_out, "wb");
    if (!o) return MFCC_HIP_ERROR_IO;
    const size_t wr = v.empty() ? 0 : std::fwrite(v.data(), sizeof(int16_t), v.size(), o);
    std::fclose(o);
    if (wr != v.size()) return MFCC_HIP_ERROR_IO;
    if (n_frames_out) *n_frames_out = v.size() / size_t(n_cep);
    return MFCC_HIP_SUCCESS;
}

// ---- serial wire format + power gate (host only): magic.py:9-41, serial.c:89-122, cepstrum.c:15-71,161-183
size_t mfcc_hip_serial_packed_size(size_t n_frames, int n_cep) {
    return n_cep > 0 ? n_frames * 2 * (size_t(n_cep) + 1) : 0;
}

int mfcc_hip_serial_pack(const int16_t *cep, size_t n_frames, int n_cep, uint8_t *out, size_t out_capacity) {
    if (n_cep <= 0 || (n_frames && (!cep || !out))) return MFCC_HIP_ERROR_INVALID_PARAM;
    if (out_capacity < mfcc_hip_serial_packed_size(n_frames, n_cep)) return MFCC_HIP_ERROR_BUFFER_SMALL;
    uint8_t *p = out;
    for (size_t f = 0; f < n_frames; ++f) {
        *p++ = 0xa5;                                   // MagicInserter: 0xa55a first, high byte first on the wire
        *p++ = 0x5a;
        for (int c = 0; c < n_cep; ++c) {
            const uint16_t v = (uint16_t)cep[f * n_cep + c];
            *p++ = (uint8_t)(v >> 8);
            *p++ = (uint8_t)(v & 0xff);
        }
    }
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_serial_unpack(const uint8_t *bytes, size_t n_bytes, int n_cep, int16_t *cep, size_t max_frames,
                           size_t *n_frames_out, size_t *consumed_out) {
    if (n_cep <= 0 || (n_bytes && !bytes) || (max_frames && !cep)) return MFCC_HIP_ERROR_INVALID_PARAM;
    size_t pos = 0, frames = 0, consumed = 0;
    const size_t col = size_t(n_cep) * 2;
    while (frames < max_frames) {
        // expect_magic: skip to 0xa5; the byte after it must be 0x5a, otherwise both are dropped
        size_t q = pos;
        bool aligned = false;
        while (!aligned) {
            while (q < n_bytes && bytes[q] != 0xa5) ++q;
            if (q + 1 >= n_bytes) { q = n_bytes; break; }
            aligned = bytes[q + 1] == 0x5a;
            q += 2;
        }
        if (!aligned || q + col > n_bytes) break;
        for (int c = 0; c < n_cep; ++c)
            cep[frames * n_cep + c] = (int16_t)(uint16_t)((bytes[q + 2 * c] << 8) | bytes[q + 2 * c + 1]);
        pos = q + col;
        consumed = pos;
        ++frames;
    }
    if (n_frames_out) *n_frames_out = frames;
    if (consumed_out) *consumed_out = consumed;
    return MFCC_HIP_SUCCESS;
}

int mfcc_hip_eval_power(const int16_t *window, int n_cep, int n_frames, size_t head, long long *power_out) {
    if (!window || n_cep <= 0 || n_frames <= 0) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t size = size_t(n_cep) * size_t(n_frames);
    if (head >= size) return MFCC_HIP_ERROR_INVALID_PARAM;
    const size_t first = 1 * size / 3, last = 2 * size / 3;
    long long power = 0;
    for (size_t i = first; i < last; i += size_t(n_cep)) {
        size_t k = head + i;
        if (k >= size) k -= size;
        power += (long long)window[k] * (long long)window[k];
    }
    if (power_out) *power_out = power;
    return power >= 100000000ll ? 1 : 0;               // POWER_THRESHOLD, cepstrum.c:13
}

#ifdef MFCC_W12_STAMPS
int mfcc_hip_debug_read_stamps12(unsigned long long *dst) {
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(mfcc_fused12::g_stamps12), sizeof(unsigned long long) * 48) != hipSuccess)
        return MFCC_HIP_ERROR_OTHER;
    unsigned long long z[48] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mfcc_fused12::g_stamps12), z, sizeof z) != hipSuccess) return MFCC_HIP_ERROR_OTHER;
    return MFCC_HIP_SUCCESS;
}
#endif

#ifdef MFCC_1K12_STAMPS
extern "C" int mfcc_hip_debug_read_stamps1k(unsigned long long *dst) {
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(mfcc_fused1024_w12bf::g_stamps1k), sizeof(unsigned long long) * 144) != hipSuccess)
        return MFCC_HIP_ERROR_OTHER;
    unsigned long long z[144] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mfcc_fused1024_w12bf::g_stamps1k), z, sizeof z) != hipSuccess) return MFCC_HIP_ERROR_OTHER;
    return MFCC_HIP_SUCCESS;
}
#endif
#ifdef MFCC_FUSED_STAMPS
// diagnostic build only: copy out and clear the per-phase cycle sums of the fused kernel
int mfcc_hip_debug_read_stamps(unsigned long long *dst) {
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(mfcc_fused::g_stamps), sizeof(unsigned long long) * 64) != hipSuccess)  // 4 x 12 phases + 16
        return MFCC_HIP_ERROR_OTHER;
    unsigned long long z[64] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mfcc_fused::g_stamps), z, sizeof z) != hipSuccess) return MFCC_HIP_ERROR_OTHER;
    return MFCC_HIP_SUCCESS;
}
#endif

}  // extern "C"
