// Per-segment normalization and deltas of rows of 65 .. 128 floats (the filterbank post-passes)
// as a translation unit, and so a device code object, of its own: the lines of kernel_normalize.hpp and kernel_deltas.hpp
// compiled a second time, with LDS arrays of 128 columns and a delta tile of mfcc_post::kDeltaWideLdsFloats.  mfcc_hip.hip
// only calls the two launchers below, and the code object of the MFCC kernels is what it is without them.
#define MFCC_POST_WIDE_UNIT
#include "kernel_deltas.hpp"
#include "post_wide.hpp"

namespace mfcc_post_wide {

static_assert(mfcc_norm_wide::kMaxWidth == mfcc_post::kWideWidth && mfcc_delta_wide::kMaxWidth == mfcc_post::kWideWidth, "row width");
static_assert(mfcc_norm_wide::kTileFloats == mfcc_post::kNormTileFloats, "stats tile");
static_assert(sizeof(mfcc_norm_wide::Part) == 24, "the partials' layout is normalize_pass's");
static_assert(mfcc_delta_wide::kMaxWindow == mfcc_post::kMaxDeltaWindow, "delta window");
// the requirement of section 4.22: at least 8 emitted rows at the widest row, order 2, the longest window
static_assert(mfcc_post::delta_wide_tile_rows(mfcc_post::kWideWidth, 2, mfcc_post::kMaxDeltaWindow) >= 8, "wide delta tile");

void launch_normalize(float *rows, const mfcc_norm::Segs &s, void *part, void *coef, int mode, int n_cu, hipStream_t stream) {
    using namespace mfcc_norm_wide;
    Part *p = static_cast<Part *>(part);
    float2 *cf = static_cast<float2 *>(coef);
    const unsigned grid = mfcc_post::wide_grid(s.n_blocks, n_cu), grid_f = mfcc_post::wide_grid(s.n_segs, n_cu);
    hipLaunchKernelGGL(normalize_stats_wide_kernel, dim3(grid), dim3(kThreads), 0, stream, static_cast<const float *>(rows), s, p);
    hipLaunchKernelGGL(normalize_finalize_wide_kernel, dim3(grid_f), dim3(kThreads), 0, stream, s, static_cast<const Part *>(p), cf,
                       mode);
    hipLaunchKernelGGL(normalize_apply_wide_kernel, dim3(grid), dim3(kThreads), 0, stream, rows, s, static_cast<const float2 *>(cf));
}

bool launch_deltas(const float *in, float *out, const mfcc_norm::Segs &s, int order, int window, int n_cu, hipStream_t stream) {
    const mfcc_delta_wide::DeltasKernel kernel = mfcc_delta_wide::deltas_kernel_of(order, window);
    if (!kernel) return false;
    hipLaunchKernelGGL(kernel, dim3(mfcc_post::wide_grid(s.n_blocks, n_cu)), dim3(mfcc_delta_wide::kThreads), 0, stream, in, out, s,
                       mfcc_delta_wide::delta_scale(window));
    return true;
}

}  // namespace mfcc_post_wide
