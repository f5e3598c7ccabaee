// Stage A, shared by the two instances of the streaming kernel (cape_cell_moments.hip) and the per-cell / strip kernels (cape_cell_fit.hip):
// the pixel accumulators of plane_segment.cpp:131-152 on top of depth_map_transformation.cpp:123-138 and the continuity
// step of plane_segment.cpp:44-60.
#pragma once
#include <hip/hip_runtime.h>

#include "cape_device.h"
#include "cape_internal.h"

namespace cape {


// tuning knobs of the BAND instance of the streaming kernel (CAPE_A1=bands; overridable for A/B builds, see profiles/sweep.py).
// Four measured-and-rejected variants of it (LDS-DMA ring prefetch, ds_add_f64 partials, v_pk_mul_f32 pixel pairs, a
// three-buffer prefetch) lived here behind macros through round 2; their numbers are kept in DESIGN.md 4.1, their code in the
// history (commit 4d9050d).
#ifndef CAPE_A_GROUP
#define CAPE_A_GROUP 2   // image rows per prefetch group
#endif
#ifndef CAPE_A_WAVES
#define CAPE_A_WAVES 4   // __launch_bounds__ waves per SIMD of the streaming kernel (measured: 4 -> 1.46 ms, 5 -> 1.49 ms, 3 -> 2.6 ms)
#endif

// ... and of the shipped lane-per-cell instance: independent waves of 64 cells, no LDS, no barrier (measured, 4 096 frames of
// 640x480, profiles/a1_lane_per_cell.txt)
#ifndef CAPE_A1_CELL_WAVES
#define CAPE_A1_CELL_WAVES 4   // __launch_bounds__ waves per SIMD: 4 (128 VGPRs, no scratch) -> 1.158 ms, 3 (155 VGPRs) -> 1.132 ms
#endif
#ifndef CAPE_A1_FUSED_WAVES
#define CAPE_A1_FUSED_WAVES 4  // the same bound for the fused instance (the lane fits its cell's plane too): profiles/a_fused.txt
#endif
#ifndef CAPE_A1_CELL_THREADS
#define CAPE_A1_CELL_THREADS 256 // waves x 64 per workgroup; the waves do not talk to each other: 64 -> 1.173 ms, 256 -> 1.158, 512 -> 1.161
#endif
#ifndef CAPE_A1_CELL_LOAD_POLICY
#define CAPE_A1_CELL_LOAD_POLICY 0 // cache policy bits of the image loads: 0 = plain (served by L1) -> 1.158 ms, 2 = nt (bypasses L1) -> 2.05 ms
#endif
constexpr int kThreadsCells = CAPE_A1_CELL_THREADS;
static_assert(kThreadsCells % 64 == 0 && kThreadsCells >= 64 && kThreadsCells <= 1024, "whole waves");

constexpr int kThreadsA = 320;
constexpr int kBandThreads = 160;
[[maybe_unused]] constexpr int kPartStride = 11; // 10 f64 per thread, padded against LDS bank conflicts

struct PxAcc
{
    double S[9];
    uint32_t n;
    // z range of the valid pixels, as bit patterns (non-negative floats order like unsigned integers): zmaxBits is the
    // greatest pattern, zminBits1 the smallest (pattern - 1) -- the -1 wraps the +0 of an invalid pixel to 0xFFFFFFFF, the
    // neutral element of the minimum, with one v_sub_u32 (which issues at twice the rate of the selects it replaces)
    uint32_t zminBits1, zmaxBits;
};

// One pixel of plane_segment.cpp:131-152 on top of depth_map_transformation.cpp:123-138.
__device__ __forceinline__ float acc_px(float zr, double a, double b, PxAcc& A)
{
    const bool valid = zr > 0.0f;       // `if (z > 0)` ; NaN is invalid
    const float z = valid ? zr : 0.0f;  // invalid pixels add +0 to every sum
    A.n += valid ? 1u : 0u;
    const double zd = (double)z;
    // ScreenCoordinate::to_camera_coordinates (point_coordinates.cpp:150-167): x = z * fl(fl(k00*u) + k02) in f64, the
    // cloud stores static_cast<float>(x) (depth_map_transformation.cpp:133-135)
    const float x = (float)(zd * a);
    const float y = (float)(zd * b);
    // float values / float products widened into double accumulators (types.hpp:84: SQR on the operand's own type)
    A.S[0] += (double)x;
    A.S[1] += (double)y;
    A.S[2] += zd;
    A.S[3] += (double)(x * x);
    A.S[4] += (double)(y * y);
    A.S[5] += (double)(z * z);
    A.S[6] += (double)(x * y);
    A.S[7] += (double)(y * z);
    A.S[8] += (double)(x * z);
    return z; // the clamped depth (+0 if invalid): what the exactness guard looks at
}

// The same pixel in the streaming kernel, WITHOUT the validity test: a compare, a select and a carry add are three
// four-cycle instructions per pixel (profiles/r02_valu_rates.txt).  A pixel that is +0 adds +0 to every sum on its own, and
// a cell that holds anything else the reference would call invalid or that poisons a sum -- a negative depth, -0, NaN,
// +inf: every bit pattern above 0x7F7FFFFF -- is caught by the per-cell range guard (its largest pattern is tracked anyway)
// and redone by A2 with acc_px in the reference's order.  What is left to count is the non-zero pixels: v_min_u32 + v_add_u32.
// The count can only be too HIGH in a cell the guard rejects, never too low, so A2's "enough points for the in-order
// pass?" test errs on the side of redoing the cell.  Returns the bit pattern for the guard.
// (The six f32 products stay plain C: spelled as inline v_mul_f32_e32 they pin the schedule and the kernel spills -- 128 VGPRs +
// scratch.  What keeps the SLP vectoriser from pairing them into v_pk_mul_f32 + register-pair moves is -fno-slp-vectorize on
// cape_cell_moments.hip, see its header.)
__device__ __forceinline__ uint32_t acc_px_fast(float z, double a, double b, PxAcc& A)
{
    const uint32_t bits = __float_as_uint(z);
    A.n += min(bits, 1u);
    const double zd = (double)z;
    const float x = (float)(zd * a);
    const float y = (float)(zd * b);
    A.S[0] += (double)x;
    A.S[1] += (double)y;
    A.S[2] += zd;
    A.S[3] += (double)(x * x);
    A.S[4] += (double)(y * y);
    A.S[5] += (double)(z * z);
    A.S[6] += (double)(x * y);
    A.S[7] += (double)(y * z);
    A.S[8] += (double)(x * z);
    return bits;
}

__device__ __forceinline__ void acc_f4(const float4& v, double a0, double a1, double a2, double a3, double b, PxAcc& A)
{
    const uint32_t bx = acc_px_fast(v.x, a0, b, A);
    const uint32_t by = acc_px_fast(v.y, a1, b, A);
    const uint32_t bz = acc_px_fast(v.z, a2, b, A);
    const uint32_t bw = acc_px_fast(v.w, a3, b, A);
    // z range of the pixels (exactness guard) on the bit patterns: v_max3_u32 / v_min3_u32 + four v_sub_u32; a pattern with
    // the sign bit or above +inf's ends up in zmaxBits and fails the guard
    A.zmaxBits = max(max(A.zmaxBits, bx), max(by, max(bz, bw)));
    A.zminBits1 = min(min(A.zminBits1, bx - 1u), min(by - 1u, min(bz - 1u, bw - 1u)));
}

// plane_segment.cpp:44-60
__device__ __forceinline__ bool is_continuous(float pixelDepth, float& last)
{
    if (pixelDepth > 0)
    {
        if ((double)fabsf(pixelDepth - last) <= 4.0 * depth_quantization((double)pixelDepth))
        {
            last = pixelDepth;
            return true;
        }
        return false;
    }
    return true;
}

// The same step as straight-line code for a scan that runs every step on every lane: once a step has failed the scan's verdict
// is false whatever follows (the reference's `&&` stops calling the function there), so the later values of `last` are never
// observed and nothing needs to branch.
__device__ __forceinline__ bool is_continuous_flat(float pixelDepth, float& last)
{
    const bool positive = pixelDepth > 0; // NaN: not positive -> the step passes, like the reference's `if`
    const bool close = (double)fabsf(pixelDepth - last) <= 4.0 * depth_quantization((double)pixelDepth);
    last = (positive & close) ? pixelDepth : last;
    return !positive | close;
}

// The same step decided in f32 wherever f32 can decide it: eleven instructions against the sixteen of the f64 form.  Returns
// the verdict and raises `unsure` when it might differ from is_continuous_flat's; the caller then runs the f64 form -- of the whole
// scan (band instance, strip kernel) or of that step from the same `last` (lane-per-cell instance: a sure lane's f32 verdict
// and `last` ARE the f64 ones, by the margin below, so redoing a step for the whole wave changes nothing for it).
//   The f64 verdict is d <= R with d = |z - last| (an f32 difference in both forms: the same bits) and
// R = 4 max(P(z), 0.5), P = c0 + c1 z + c2 z^2 evaluated in f64 (relative error ~2^-50, nothing at the scale below).
//   r below is max(4 P, 2) by two f32 fma on the constants rounded to f32 (u = 2^-24 each): its distance from the exact value
// is at most 3 u (4 |c0| + 4 c1 z + 4 c2 z^2) = 3 u (4 P + 8 |c0|) for z > 0.  Where 4 P >= 2 that is 3 u (1 + 4.24 / 2) R
// = 9.4 u R, and where 4 P < 2 both sides are clamped to 2 (max is 1-Lipschitz): |r - R| <= 2^-20 R for every z > 0 whose
// polynomial does not overflow.
//   t = fl(d - r) has the sign of d - r and at most (1 + u) times its magnitude.  If |t| > 2^-16 r then
//     |d - r| > 2^-16 r / (1 + u) >= 2^-16 (1 - 2^-20) R / (1 + 2^-24) > 2^-20 R >= |r - R|,
// so d - R = (d - r) + (r - R) has the sign of d - r, which is the sign of t: `t <= 0` IS the f64 verdict.
//   Everything else is `unsure`: d within 2^-16 of the threshold, d NaN (then t is NaN and the compare fails), and z so large
// that the f32 polynomial overflows -- then r = +inf and t is -inf or NaN, never beyond 2^-16 r = +inf.  z <= 0 or NaN
// passes whatever d is, like the reference's `if`, and never raises `unsure`.
__device__ __forceinline__ bool is_continuous_flat_f32(float pixelDepth, float& last, bool& unsure)
{
    // depth_quantization's constants (cape_device.h) times the 4 of the test
    constexpr float c2 = (float)(4.0 * (2.73 * ((1.0 / 1000.0) * (1.0 / 1000.0))));
    constexpr float c1 = (float)(4.0 * (0.74 / 1000.0));
    constexpr float c0 = (float)(4.0 * -0.53);
    const bool positive = pixelDepth > 0;
    const float r = fmaxf(fmaf(fmaf(c2, pixelDepth, c1), pixelDepth, c0), 2.0f);
    const float t = fabsf(pixelDepth - last) - r;
    const bool notSure = !(fabsf(t) > r * 0x1p-16f);
    const bool close = t <= 0;
    unsure |= positive & notSure;
    last = (positive & close) ? pixelDepth : last;
    return !positive | close;
}

} // namespace cape
