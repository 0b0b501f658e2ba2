// The launchers of post_wide.hip: per-segment normalization and deltas of rows of 65 .. 128 floats, the filterbank
// post-passes (include/mfcc_hip.h: "filterbank post-passes").  mfcc_hip.hip calls these two
// functions from normalize_pass and deltas_pass and sees nothing else of that unit: its own code object stays what it is.
#pragma once

#include <hip/hip_runtime.h>

#include "post_plan.hpp"
#include "seg_plan.hpp"

namespace mfcc_post_wide {

// stats, finalize, apply, as normalize_pass enqueues the narrow three.  s: tiles of mfcc_post::norm_tile_rows(width) rows;
// part: n_blocks * W * 24 bytes, coef: n_segs * W * 8 bytes; mode: 1 = mean, 2 = mean and variance
void launch_normalize(float *rows, const mfcc_norm::Segs &s, void *part, void *coef, int mode, int n_cu, hipStream_t stream);

// s: tiles of mfcc_post::delta_wide_tile_rows(width, order, window) rows.  false: no kernel for (order, window)
bool launch_deltas(const float *in, float *out, const mfcc_norm::Segs &s, int order, int window, int n_cu, hipStream_t stream);

}  // namespace mfcc_post_wide
