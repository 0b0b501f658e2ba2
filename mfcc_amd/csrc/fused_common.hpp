// Helpers shared by the fused float kernels (kernel_fused512.hpp, kernel_fused1024.hpp): the uniform tile
// cursor, the geometry of a tile's sample window, exact integer pre-emphasis, the LDS-only barrier.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_generic.hpp"
#include "launch_geom.hpp"

namespace mfcc_fc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a full workgroup fence: it also
// drains vmcnt, i.e. waits for the prefetch loads of the next tile and for role 0's output stores,
// which nothing on the other side of the barrier depends on.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Uniform (SGPR) cursor over the workgroup's tiles: tile = ch * tiles_per_ch + t_in.  Advancing by
// the grid size is a handful of scalar adds with one carry -- no multiply or division in the loop
// (a wave's scalar instructions issue ~10 clocks apart; the multiply form of this cost ~450 clocks
// per tile in every wave).
struct Cursor {
    int ch, t_in;
    const int16_t *ptr;      // the tile's first sample: s.pcm + ch * ch_stride + t_in * kTileHop
};

// LaunchGeom of a stream (launch_geom.hpp); false: the problem does not fit the kernel's 32-bit tile arithmetic
inline bool launch_geom(const mfcc_k::StreamDesc &s, int n_cu, TileShape k, GridRule rule, int guard_bits, LaunchGeom &g,
                        unsigned &workgroups) {
    return launch_geom(s.frames_per_ch, s.total_frames, s.ch_stride, s.n_samples, s.halo, n_cu, k, rule, guard_bits, g,
                       workgroups);
}

__device__ __forceinline__ void advance(Cursor &c, const LaunchGeom &g) {
    c.t_in += g.grid_mod;
    c.ch += g.grid_div;
    c.ptr += g.step_ptr;
    if (c.t_in >= g.tiles_per_ch) {
        c.t_in -= g.tiles_per_ch;
        ++c.ch;
        c.ptr += g.wrap_ptr;
    }
}

// uniform (scalar) geometry of a tile's window; every wave computes it, fetchers or not
struct Window {
    const int16_t *ptr;      // the tile's first sample
    int t_in;
    int shift;
    bool inside;             // whole window (and the dword in front of it) lies inside the channel
};

__device__ __forceinline__ Window window_of(const Cursor &c, const LaunchGeom &g) {
    Window w;
    w.ptr = c.ptr;
    w.t_in = c.t_in;
    const int mis = (int)((reinterpret_cast<uintptr_t>(c.ptr) & 15) >> 1);   // samples past alignment
    // t_lo / t_hi (launch_geom.hpp): first - 7 - 2 >= -halo (the dword in front of piece 0) and first + kSUsed <= n_samples
    w.inside = c.t_in >= g.t_lo && c.t_in <= g.t_hi;
    w.shift = w.inside ? mis : 0;
    return w;
}

// e[k] = den x[k] - num x[k-1] for the 8 samples packed in v, x[-1] = high half of prev; pair = (int16 -num, int16 den),
// by default the reference's 32 x[k] - 31 x[k-1].  One v_dot2_i32_i16 per sample (the three-operand form: for the builtin
// hipcc picks v_dot2c, which costs an extra v_mov 0 per sample); the 1 / den is in the window table.
// No int -> float conversion: the dot product's addend is 0x4B400000, the bits of the float 1.5 * 2^23, whose ulp is 1 --
// so for |e| < 2^22 the integer sum IS the float 12582912 + e, and ONE packed subtraction per pair of samples takes the
// bias off again, exactly: 4 instructions per pair of samples instead of 5.
// Range: |x| <= 2^15, so |e| <= (num + den) 2^15.  The default pair gives 63 * 2^15 < 2^21; a pair from the tables struct
// (the four-wave 512 kernels and the power tile) has num + den <= 127 (tables.hpp: kMaxFusedPreemphSum), so
// |e| <= 127 * 2^15 < 2^22 and 12582912 + e stays inside [2^23, 2^24), where the float's ulp is 1.  The host refuses to build
// those kernels' tables for a larger pair (num + den <= 255 keeps |e| < 2^23, exact in fp32, but not under this bias).
// The kernels that do not pass a pair (twelve-wave 512, the 1024 forms) keep the constant at compile time.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void preemph8(int prev, const i32x4 &v, float *__restrict__ dst, const int pair = 0x0020ffe1) {
    const int c3132 = pair;                        // default: (int16 -31, int16 32)
    const int bias_bits = 0x4B400000;              // 12582912.0f (a VGPR: VOP3 takes one scalar operand on gfx9)
    const f32x2 bias = {12582912.0f, 12582912.0f};
    f32x2 e[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int before = m ? v[m - 1] : prev;
        const int pe = (int)__builtin_amdgcn_alignbit((unsigned)v[m], (unsigned)before, 16u);   // (x[2m-1], x[2m])
        int e0, e1;
        asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(e0) : "v"(pe), "s"(c3132), "v"(bias_bits));
        asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(e1) : "v"(v[m]), "s"(c3132), "v"(bias_bits));
        e[m] = (f32x2){__int_as_float(e0), __int_as_float(e1)} - bias;
    }
    reinterpret_cast<f32x4 *>(dst)[0] = (f32x4){e[0].x, e[0].y, e[1].x, e[1].y};
    reinterpret_cast<f32x4 *>(dst)[1] = (f32x4){e[2].x, e[2].y, e[3].x, e[3].y};
}

}  // namespace mfcc_fc
