// Stage A -- fused back-projection + per-cell PCA for gfx950.  Two parts, one launch where the grid allows it:
//
//   A1 cape_cell_moments_kernel : the HBM/FP64-issue bound streaming pass.  Reads the row-major depth image once,
//      back-projects on the fly and leaves, per cell, the nine moment sums + count, the result of the continuity
//      cross scan and the exactness verdict.  Replaces Depth_Map_Transformation::get_organized_cloud_array
//      (reference src/features/primitives/depth_map_transformation.cpp:89-142) and the scan + accumulation part of
//      Plane_Segment::init_plane_segment (plane_segment.cpp:44-152).  The 3.7 MB organised cloud is never built.
//   A2 the per-cell fit (cape_cell_plane.h) : one lane per cell: validity gates, Plane_Segment::fit_plane
//      (plane_segment.cpp:155-168, 205-284), the merge tolerance of init_planar_cell_fitting
//      (primitive_detection.cpp:201-220), the histogram bin of init_histogram (primitive_detection.cpp:253-254 +
//      histogram.hpp:48-54) and the merge predicates of the cell's left and upper edges.  The lane that summed a cell
//      holds everything the fit reads, so in the FUSED instance it carries on with it (below); elsewhere A2 is
//      cape_cell_plane_kernel (cape_cell_fit.hip), which loads what A1 stored.
//
// A1 mapping, the shipped instance (cape_cell_moments_kernel, "cells"): one LANE per cell.  A wave is 64 consecutive cells of a
// frame in cell-row-major order, lane l of wave w owns cell 64 w + l and walks its 20 rows of 20 pixels (80 contiguous, 16-B
// aligned bytes per row: five 16-B loads through L1, where the lanes' pieces meet in their 128-B lines).  The lane keeps the
// cell's 20 column factors, its nine sums, count and z range in registers, takes one step of the vertical continuity scan per
// row and the horizontal scan's 19 steps at row 10, and stores its 80 B of sums and its aux record itself: no LDS, no
// barrier, no second pass; a wave leaves as soon as its last pixel is summed.  Any grid goes through the same code (waves
// may start and end inside a cell row; the last wave of a frame may be partial).  128 VGPRs, 4 waves per SIMD.
// FUSED = true is the same kernel with A2 behind the last pixel, for the grids on which a 256-lane workgroup -- four waves of 64
// consecutive cells -- is exactly a tile of A2's 256-thread instance (cell_fused_eligible: 640x480 is 3 tiles of 8 cell rows per
// frame): the lane runs cell_fit_and_bin on the sums in its registers (the column factors' 40 registers are dead by then), stores
// the sums once, and the workgroup publishes its planes in LDS (16 KB), meets at ONE barrier and evaluates the left and up edge
// predicates as an A2 tile does (tile_publish_and_finish).  No lane leaves ahead of that barrier: every lane of every workgroup
// holds a cell, which launch_cell_fused checks.  A2's launch, its 96 B per cell of loads and the cache contents that A1's image
// loads cost it are gone: 1.565 against 1.615 ms per 4 096 frames (profiles/a_fused.txt); same 128 VGPRs, no scratch.
// The band instance (cape_cell_moments_bands_kernel, CAPE_A1=bands: the bit-for-bit twin of the tests and the in-build A/B
// partner): one 320-thread workgroup = two "bands" (band = 20 image rows x 640 pixels = 32 cells).  Thread t owns
// float4 column q = t % 160 of band t / 160 and walks the band's 20 rows, so every wave-level load is a contiguous
// 16 B/lane segment of the row-major image; a float4 never straddles a cell (20 = 5 float4).  Rows are loaded two
// at a time (CAPE_A_GROUP), ping-pong buffered, one group ahead of the arithmetic (non-temporal: the image is read once).  Per-thread partial sums (f64) meet in LDS; 5 partials = one cell.
// Numbers of both: profiles/a1_lane_per_cell.txt.
// The sums are exact in f64 for ANY summation order when the addends' exponent span is < 21 bits;
// a per-cell z-range guard decides whether that holds, otherwise A2 redoes the cell in the reference's pixel order.
// That is also why the two instances leave the same bits.
//
// This file is compiled with -fno-slp-vectorize (Makefile): left to itself the SLP vectoriser pairs the six
// f32 products of a pixel into v_pk_mul_f32, which costs as much as the two v_mul_f32_e32 it replaces on gfx950
// (profiles/r02_valu_rates.txt: 4.5 against 2 x 2.3 cycles) PLUS the v_mov_b32 / v_pk_mov_b32 that build its register pairs
// (36 moves per 16 pixels; 94 -> 84 VGPRs without them).  A2 and the strip kernel (cape_cell_fit.hip) keep the vectoriser:
// A2 measured 2 % slower without it.  The fit of the fused instance is compiled without it like the rest of this file (the row
// loop loses 6 % with it); what that costs the fit on its own was not measured apart.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cape_cell_plane.h"

namespace cape {

template <bool U16> __global__ __launch_bounds__(kThreadsA, CAPE_A_WAVES) void cape_cell_moments_bands_kernel(StageAParams p)
{
    // LDS: per-thread partials (written behind the row loop) and the 64 cells' centre row / centre column samples (written in it)
    __shared__ double s_part[kThreadsA * kPartStride]; // [thread][9 sums, count, (zmin,zmax) packed in the pad slot]
    __shared__ float s_row[64 * kCell];  // local row 10 of every cell (idx 200..219)
    __shared__ float s_col[64 * kCell];  // local column 10 of every cell (idx 10, 30, ..., 390)
    __shared__ float s_corner[64 * 2];   // first and last pixel of every cell (the centre pixel is s_row[.. + 10])
    __shared__ float s_trash[kThreadsA + kCell]; // where the lanes that do not hold a cell's centre column send their row's store

    const int t = threadIdx.x;
    const int frame = blockIdx.x / p.pairsPerFrame;
    const int pair = blockIdx.x - frame * p.pairsPerFrame;
    const size_t frameOff = (size_t)frame * p.W * p.H;

    // The workgroup's two bands are consecutive, so the second one's cell row and 640-pixel segment follow from the first's
    // without a second division -- and both are uniform: they live in scalar registers, for the streaming lanes (which pick
    // theirs with one select per quantity) and for the reduce and aux stores behind the barrier alike.
    const int band0 = pair * 2;
    const int cellRow0 = band0 / p.segsPerRow;
    const int seg0 = band0 - cellRow0 * p.segsPerRow;
    const bool wrap = seg0 + 1 == p.segsPerRow;
    const int cellRowOf[2] = {cellRow0, cellRow0 + (wrap ? 1 : 0)};
    const int segOf[2] = {seg0, wrap ? 0 : seg0 + 1};
    const bool bandExists[2] = {band0 < p.bandsPerFrame, band0 + 1 < p.bandsPerFrame};
    // what a streaming lane needs of its band, multiplied out per band (scalar) before the lane picks one
    // (readfirstlane of a uniform value is a scalar move; it keeps the compiler from turning "select of two products" back
    // into "product of a select", a vector multiply)
    const int firstRowOf[2] = {__builtin_amdgcn_readfirstlane(cellRowOf[0] * kCell), __builtin_amdgcn_readfirstlane(cellRowOf[1] * kCell)};
    const int firstColOf[2] = {__builtin_amdgcn_readfirstlane(segOf[0] * 640), __builtin_amdgcn_readfirstlane(segOf[1] * 640)};
    const uint32_t firstPixOf[2] = {(uint32_t)__builtin_amdgcn_readfirstlane(firstRowOf[0] * p.W), (uint32_t)__builtin_amdgcn_readfirstlane(firstRowOf[1] * p.W)};
    const int colLimitOf[2] = {bandExists[0] ? p.W : 0, bandExists[1] ? p.W : 0};

    const int bsel = t / kBandThreads;
    const int q = t - bsel * kBandThreads;
    const int row0 = bsel ? firstRowOf[1] : firstRowOf[0];
    const int col0 = (bsel ? firstColOf[1] : firstColOf[0]) + q * 4;
    const bool active = col0 < (bsel ? colLimitOf[1] : colLimitOf[0]);
    const int cseg = q / 5;          // cell within the band segment
    const int j = q - cseg * 5;      // float4 within the cell row
    const int lcell = bsel * 32 + cseg;

    // ------------------------------------------------------------------ streaming accumulation
    PxAcc A;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        A.S[k] = 0.0;
    A.n = 0;
    A.zminBits1 = 0xFFFFFFFFu;
    A.zmaxBits = 0u;
    if (active)
    {
        const double a0 = p.acol[col0], a1 = p.acol[col0 + 1], a2 = p.acol[col0 + 2], a3 = p.acol[col0 + 3];
        // addresses = one base per FRAME (uniform: it lives in scalar registers and advances row by row with scalar adds)
        // + one 32-bit element offset per thread (its column inside the frame): no 64-bit vector address arithmetic per load
        const uint32_t pixOff32 = (bsel ? firstPixOf[1] : firstPixOf[0]) + (uint32_t)col0;
        const float* frameBase = p.depth + frameOff;                 // float32 millimetres
        const uint16_t* frameBase16 = p.depth_u16 + frameOff;        // raw sensor units (U16 variant)
        const float scale16 = p.u16_scale;
        const double* brow = p.brow + row0;
        const size_t W = (size_t)p.W;

        // rows in groups of kGroup, ping-pong buffered: the loads of group g+1 are in flight while group g is summed
        constexpr int kGroup = CAPE_A_GROUP, kGroups = kCell / kGroup;
        static_assert(kCell % kGroup == 0 && kGroups % 2 == 0, "the ping-pong loop consumes two groups per trip");
        // the buffers hold what was LOADED (float4, or the raw ushort4 of the U16 variant): converting at load time would
        // make every load wait for its data on the spot and serialise the prefetch with the arithmetic
        using Raw = typename std::conditional<U16, ushort4, float4>::type;
        Raw bufA[kGroup], bufB[kGroup];
        auto load_group = [&](Raw (&buf)[kGroup], int g) {
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
            {
                const size_t rowOff = (size_t)(kGroup * g + i) * W; // uniform
                // non-temporal: the image is read exactly once, nothing of it is worth a cache line (1 % by interleaved A/B runs)
                if constexpr (U16)
                {
                    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
                    const u16x4 v = __builtin_nontemporal_load(reinterpret_cast<const u16x4*>((frameBase16 + rowOff) + pixOff32));
                    buf[i] = make_ushort4(v.x, v.y, v.z, v.w);
                }
                else
                {
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>((frameBase + rowOff) + pixOff32));
                    buf[i] = make_float4(v.x, v.y, v.z, v.w);
                }
            }
        };
        auto to_f4 = [&](const Raw& rw) {
            if constexpr (U16)
            {
                // N4: the PNG payload of the TUM / CAPE datasets, converted exactly like
                // cv::Mat::convertTo(CV_32F, scale) does (examples/main_TUM.cpp:242): float(raw) * float(scale)
                // (one v_mul_f32_e32 each: this file is compiled without the SLP vectoriser, which used to pair them into
                // v_pk_mul_f32 + register-pair moves -- 2.00 ms per 4 096 frames packed against 1.54 ms; through round 4 they
                // were inline asm for that reason)
                return make_float4((float)rw.x * scale16, (float)rw.y * scale16, (float)rw.z * scale16, (float)rw.w * scale16);
            }
            else
            {
                return rw;
            }
        };
        // samples for the continuity cross scan and the tolerance corners.  The centre column is one store per row by EVERY
        // lane -- the lane that holds pixel column 10 of its cell (j == 2) into s_col, the others into a trash slot of their
        // own: a predicated store costs the wave an exec-mask round trip per row.  First / last pixel of the cell come from
        // the peeled first / last trip (compile-time rows), the centre row from the trip that holds row 10.
        float* const colp = (j == 2) ? &s_col[lcell * kCell] : &s_trash[t];
        auto sum_group = [&](const Raw (&rawbuf)[kGroup], int g, auto where) {
            constexpr int kWhere = decltype(where)::value; // 0: first trip, 1: loop, 2: last trip
            float4 buf[kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
                buf[i] = to_f4(rawbuf[i]);
#pragma unroll
            for (int i = 0; i < kGroup; ++i)
            {
                const int r = kGroup * g + i;
                acc_f4(buf[i], a0, a1, a2, a3, brow[r], A);
                colp[r] = buf[i].z; // pixel column 10 of the cell (lanes j == 2)
                if (kWhere == 1 && r == kCell / 2)
                    *reinterpret_cast<float4*>(&s_row[lcell * kCell + 4 * j]) = buf[i];
                if (kWhere == 0 && i == 0 && g == 0 && j == 0)
                    s_corner[lcell * 2] = buf[i].x;
                if (kWhere == 2 && r == kCell - 1 && j == 4)
                    s_corner[lcell * 2 + 1] = buf[i].w;
            }
        };
        using First = std::integral_constant<int, 0>;
        using Loop = std::integral_constant<int, 1>;
        using Last = std::integral_constant<int, 2>;
        static_assert(kGroups >= 6 && (kCell / 2) / kGroup >= 2 && (kCell / 2) / kGroup < kGroups - 2, "row 10 belongs to a trip of the loop");
        load_group(bufA, 0);
        // first and last trip peeled: compile-time rows for the corner samples, and no `if (g + 2 < kGroups)` inside the loop
        // (with it the loop carried both buffers through copies, eight v_mov_b64 per trip)
        load_group(bufB, 1);
        sum_group(bufA, 0, First{});
        load_group(bufA, 2);
        sum_group(bufB, 1, First{});
#pragma unroll 1
        for (int g = 2; g < kGroups - 2; g += 2)
        {
            load_group(bufB, g + 1);
            sum_group(bufA, g, Loop{});
            load_group(bufA, g + 2);
            sum_group(bufB, g + 1, Loop{});
        }
        load_group(bufB, kGroups - 1);
        sum_group(bufA, kGroups - 2, Last{});
        sum_group(bufB, kGroups - 1, Last{});
    }
    {
        double* dst = s_part + t * kPartStride;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            dst[k] = A.S[k];
        dst[9] = (double)A.n;
        reinterpret_cast<uint2*>(dst + 10)[0] = make_uint2(A.zminBits1, A.zmaxBits);
    }
    __syncthreads();

    // ------------------------------------------------------------------ behind the barrier: wave 4 sums, waves 0..3 scan
    // The workgroup's LDS and wave slots are held until its last wave leaves, so the work behind the last pixel is spread for
    // LATENCY: the 5-partials sums on one wave beside the scans, the scans cut in four (below) -- profiles/r04_a1_phases.txt.
    const int w = __builtin_amdgcn_readfirstlane(t >> 6); // the wave: uniform, so what follows from it stays in scalar registers
    if (w == 4)
    {
        // 5 partials -> one cell (exact, any order).  A band's 32 cells are consecutive in cell_sums, so its output is one
        // block of 320 doubles ([cell][10]) and lane l takes doubles l, l + 64, .. of BOTH bands: consecutive lanes store
        // consecutive doubles from a uniform base, and the LDS source of double o = 10 cell + quantity,
        // s_part[5 cell * kPartStride + quantity] = s_part[o + (5 kPartStride - 10) cell], is shared by the two bands.
        const int l = t & 63;
        static_assert(kBandThreads == 32 * 5 && kSumStride == 10, "a band is 32 cells of 5 partials, a cell 10 sums");
        double* dst[2];
        int lim[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
        {
            dst[cb] = p.cell_sums + ((size_t)frame * p.cells + cellRowOf[cb] * p.hCells + segOf[cb] * 32) * kSumStride;
            lim[cb] = bandExists[cb] ? p.hCells - segOf[cb] * 32 : 0; // cells of the band that exist
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
        {
            const int o = l + 64 * k;
            const int cs = o / kSumStride;
            const double* src = s_part + o + (5 * kPartStride - kSumStride) * cs;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
            {
                if (cs < lim[cb])
                {
                    const double* sp = src + cb * kBandThreads * kPartStride;
                    double acc = sp[0];
                    acc += sp[kPartStride];
                    acc += sp[2 * kPartStride];
                    acc += sp[3 * kPartStride];
                    acc += sp[4 * kPartStride];
                    dst[cb][o] = acc;
                }
            }
        }
        return;
    }

    // Continuity cross scans, four lane-tasks per cell, sixteen cells per wave: lane = (task, cell) with task = horizontal /
    // vertical x first / second half of the scan's steps; the four verdicts meet through two cross-lane reads.
    //   is_cell_horizontal_continuous (plane_segment.cpp:82-100): local row 10, idx 200..219, steps 1..19
    //   is_cell_vertical_continuous (:62-80): local column 10, idx 10, 30, .., 370: steps 1..18 (the loop stops before idx 390)
    // A step only needs `last`, the latest depth that passed.  If the first half (seed test, steps 1..9) passes, every positive
    // depth in it has become `last` in turn, so the second half (steps 10..) starts from the last positive depth among steps
    // 1..9, else from the seed max(z[0], z[1]) -- and if the first half fails the cell is discontinuous whatever the second
    // half says.  The steps are straight-line code, so all four tasks are one instruction stream of ten steps: in f32
    // (is_continuous_flat_f32), and once more in f64 (is_continuous_flat) if some step of some lane of the wave sits too close
    // to its threshold for f32 to call.  (Through round 4 wave 0 ran both scans of all 64 cells one behind the other, 37
    // branching steps on a lone wave; round 3's other extreme -- one lane per TEST on all five waves, a look-back loop per
    // test -- measured slower.)
    const int l = t & 63;
    const int c64 = w * 16 + (l & 15);   // cell of the workgroup (= lcell of the lanes that streamed it)
    const bool vertical = (l & 32) != 0;
    const bool second = (l & 16) != 0;
    bool continuous;
    {
        const float* zs = (vertical ? s_col : s_row) + c64 * kCell;
        const float seed = std_maxf(zs[0], zs[1]);
        float start = seed;
#pragma unroll
        for (int i = 1; i <= 9; ++i)
        {
            const float z = zs[i];
            start = (second && z > 0) ? z : start;
        }
        const bool seeded = second || !(seed <= 0);
        const float* zt = zs + (second ? 10 : 1);
        const int steps = second ? (vertical ? 9 : 10) : 9;
        float zk[10];
#pragma unroll
        for (int k = 0; k < 10; ++k)
            zk[k] = zt[k];
        float last = start;
        bool unsure = false;
        continuous = seeded;
#pragma unroll
        for (int k = 0; k < 10; ++k)
        {
            // a step beyond the scan's last neither counts nor may ask for the f64 pass
            bool stepUnsure = false;
            const bool pass = is_continuous_flat_f32(zk[k], last, stepUnsure);
            continuous &= pass | (k >= steps);
            unsure |= stepUnsure & (k < steps);
        }
        if (__any(unsure))
        {
            last = start;
            continuous = seeded;
#pragma unroll
            for (int k = 0; k < 10; ++k)
            {
                const bool pass = is_continuous_flat(zk[k], last);
                continuous &= pass | (k >= steps);
            }
        }
        continuous &= __shfl_xor((int)continuous, 16) != 0;
        continuous &= __shfl_xor((int)continuous, 32) != 0;
    }
    const int fb = w >> 1, fs = (w & 1) * 16 + (l & 15); // c64 >> 5, c64 & 31
    if ((l >> 4) != 0 || !(fb ? bandExists[1] : bandExists[0]))
        return;
    const int fRow = fb ? cellRowOf[1] : cellRowOf[0];
    const int fCol = (fb ? segOf[1] : segOf[0]) * 32 + fs;
    if (fCol >= p.hCells)
        return;
    // exactness guard: all addends of every sum within 2^20 of each other (see header)
    uint32_t zminBits1 = 0xFFFFFFFFu, zmaxBits = 0u;
    uint32_t n = 0;
    {
        const int pbase = fb * kBandThreads + fs * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k)
        {
            const uint2 zr = reinterpret_cast<const uint2*>(s_part + (pbase + k) * kPartStride + 10)[0];
            zminBits1 = min(zminBits1, zr.x);
            zmaxBits = max(zmaxBits, zr.y);
            n += (uint32_t)s_part[(pbase + k) * kPartStride + 9];
        }
    }
    // back to depths: with n > 0 at least one pixel was valid, so the minimum is a real pattern - 1
    const float zmin = __uint_as_float(zminBits1 + 1u), zmax = __uint_as_float(zmaxBits);
    const float rab = fmaxf(p.ratio_col[fCol], p.ratio_row[fRow]);
    // all pixels +0 or positive and finite (acc_px_fast's precondition), and their range within the exactness bound
    const bool exact_ok = zmaxBits <= 0x7F7FFFFFu && ((n == 0) || (zmax * rab <= 512.0f * zmin));

    const size_t gcell = (size_t)frame * p.cells + fRow * p.hCells + fCol;
    CellAux aux;
    aux.z0 = s_corner[c64 * 2];
    aux.z399 = s_corner[c64 * 2 + 1];
    aux.flags = (n & kCountMask) | (continuous ? kAuxContinuous : 0u) | (exact_ok ? kAuxExact : 0u);
    aux.zc = s_row[c64 * kCell + kCell / 2];
    p.cell_aux[gcell] = aux;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The lane-per-cell instance (see the header; the band instance above is kept selectable until the wide grids are measured).
// A wave is 64 consecutive cells of one frame, lane l of wave w owns cell 64 w + l: its nine sums, count, z range, both
// continuity scans and the corner / centre samples never leave its registers.  nWaves: frames x waves per frame.
template <bool U16, bool FUSED>
__global__ __launch_bounds__(kThreadsCells, FUSED ? CAPE_A1_FUSED_WAVES : CAPE_A1_CELL_WAVES) void cape_cell_moments_kernel(StageAParams p, int nWaves)
{
    // the wave: uniform, so the frame and its base address live in scalar registers
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kThreadsCells / 64) + (threadIdx.x >> 6)));
    // FUSED: every lane of every workgroup holds a cell (launch_cell_fused checks the grid), so nobody leaves ahead of the barrier
    if constexpr (!FUSED)
        if (gw >= nWaves)
            return; // the last workgroup's waves beyond the batch's last frame
    const int wavesPerFrame = (p.cells + 63) >> 6;
    const int frame = gw / wavesPerFrame;
    const int w = gw - frame * wavesPerFrame;
    const int cell = w * 64 + (int)(threadIdx.x & 63);
    if constexpr (!FUSED)
        if (cell >= p.cells)
            return; // (no barrier in this instance: a lane without a cell just leaves)
    const int cellRow = cell / p.hCells;
    const int cellCol = cell - cellRow * p.hCells;
    const size_t frameOff = (size_t)frame * p.W * p.H;

    PxAcc A;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        A.S[k] = 0.0;
    A.n = 0;
    A.zminBits1 = 0xFFFFFFFFu;
    A.zmaxBits = 0u;

    // the cell's 20 column factors: 40 VGPRs, loaded once
    double a[kCell];
    {
        const double2* ap = reinterpret_cast<const double2*>(p.acol + cellCol * kCell);
#pragma unroll
        for (int k = 0; k < kCell / 2; ++k)
        {
            const double2 v = ap[k];
            a[2 * k] = v.x;
            a[2 * k + 1] = v.y;
        }
    }
    // piece j of a row: four pixels and their column factors
    auto acc_piece = [&](const float4& v, int j, double b) { acc_f4(v, a[4 * j], a[4 * j + 1], a[4 * j + 2], a[4 * j + 3], b, A); };

    // Addresses: one buffer descriptor per FRAME (scalar registers; built from uniform values only), the row as the scalar
    // offset of the load, and ONE 32-bit byte offset per lane -- no 64-bit pointer per lane and per stream, which is what
    // loop strength reduction makes of plain pointers here.  A frame is far below the descriptor's 4 GB, and a load beyond the
    // frame would return zeros instead of faulting.
    constexpr uint32_t kPixBytes = U16 ? 2 : 4;
    const uint32_t pixByteOff = ((uint32_t)(cellRow * kCell) * (uint32_t)p.W + (uint32_t)(cellCol * kCell)) * kPixBytes;
    const uint32_t browByteOff = (uint32_t)(cellRow * kCell) * 8u;
    const uint32_t rowBytes = (uint32_t)p.W * kPixBytes;
    const float scale16 = p.u16_scale;
    auto uniform_ptr = [](const void* q) {
        const uint64_t u = reinterpret_cast<uint64_t>(q);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
        return reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
    };
    const void* frameBase = U16 ? (const void*)(p.depth_u16 + frameOff) : (const void*)(p.depth + frameOff);
    const __amdgpu_buffer_rsrc_t frameRsrc =
        __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(frameBase), 0, (int)((uint32_t)p.H * rowBytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t browRsrc = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(p.brow), 0, p.H * 8, 0x00020000);
    auto brow_at = [&](int r) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(browRsrc, browByteOff, r * 8, 0);
        return __hiloint2double((int)v.y, (int)v.x);
    };

    // a row of the cell as it was LOADED: five 16-B (8-B in the U16 variant) pieces of the lane's 80 (40) contiguous bytes.
    // Plain loads, not non-temporal ones: the five pieces share their 128-B lines with each other and with the neighbour lanes'.
    using Raw = typename std::conditional<U16, ushort4, float4>::type;
    constexpr int kQuads = kCell / 4;
    static_assert(kCell == 20, "five float4 per row, pixel column 10 = .z of piece 2");
    auto load_piece = [&](int r, int j) -> Raw {
        const int rowOff = r * (int)rowBytes; // uniform, and so is the piece: both travel in the load's scalar offset
        if constexpr (U16)
        {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(frameRsrc, pixByteOff, rowOff + 8 * j, CAPE_A1_CELL_LOAD_POLICY);
            return make_ushort4((unsigned short)(v.x & 0xFFFFu), (unsigned short)(v.x >> 16), (unsigned short)(v.y & 0xFFFFu), (unsigned short)(v.y >> 16));
        }
        else
        {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(frameRsrc, pixByteOff, rowOff + 16 * j, CAPE_A1_CELL_LOAD_POLICY);
            return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    };
    auto to_f4 = [&](const Raw& rw) {
        if constexpr (U16)
            return make_float4((float)rw.x * scale16, (float)rw.y * scale16, (float)rw.z * scale16, (float)rw.w * scale16); // see the band kernel
        else
            return rw;
    };

    // Continuity cross scans (plane_segment.cpp:62-100), one step at a time as the pixels stream by:
    //   vertical: local column 10, seeded with max(z[row 0], z[row 1]), one step per row 1..18 (the loop stops before row 19)
    //   horizontal: local row 10, seeded with max(z[0], z[1]), steps 1..19
    // A step runs in f32 (is_continuous_flat_f32); where some lane of the wave cannot call it, the wave redoes THAT step in f64
    // from the same `last`: a sure lane's f32 verdict and `last` are the f64 ones (margin proof in cape_cell_acc.h).
    // `counts`: uniform; a step that does not count neither fails the scan nor asks for the f64 form.
    auto scan_step = [](float z, float& last, bool& continuous, bool counts) {
        const float before = last;
        bool unsure = false;
        bool pass = is_continuous_flat_f32(z, last, unsure);
        if (__any(unsure & counts))
        {
            last = before;
            pass = is_continuous_flat(z, last);
        }
        continuous &= pass | !counts;
    };
    bool continuous = true;
    // The lane's cell in the per-cell arrays, worked out afresh where the results are stored: the lane id from mbcnt of an
    // all-ones mask, opaque to the compiler so that no index or address of the prologue is carried through the loops, where
    // every register counts.
    auto my_cell = [&]() {
        uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        asm volatile("" : "+v"(lane));
        return ((size_t)frame * p.cells + (size_t)(w * 64)) + lane;
    };

    // One row buffer in the source, refilled piece by piece: a piece of row r + 1 is requested as soon as the same piece of row r
    // has been taken out.  (The compiler gathers the five requests at the top of the row and so holds two rows after all; spelled
    // as two buffers with the scans inside the loop the same kernel spilled at 128 VGPRs.)
    Raw buf[kQuads];
#pragma unroll
    for (int j = 0; j < kQuads; ++j)
        buf[j] = load_piece(0, j);
    double b = brow_at(0);
    const float z0 = to_f4(buf[0]).x;
    float zc = 0.0f;
    float vLast = 0.0f;
    // A row's arithmetic is ONE straight-line block -- nothing in it depends on r but addresses -- and the vertical scan's step
    // comes behind it: its row-dependent parts are selects on the uniform r, its f64 form the row's only branch.
    //   row 0: last = z, and the step (z against itself) does not count;  row 1: last = max(last, z), which seeds the scan
    auto stream_row = [&](int r) {
        const double bn = brow_at(r + 1);
        float zv = 0.0f;
#pragma unroll
        for (int j = 0; j < kQuads; ++j)
        {
            const float4 v = to_f4(buf[j]);
            buf[j] = load_piece(r + 1, j);
            acc_piece(v, j, b);
            if (j == 2)
                zv = v.z; // pixel column 10
        }
        b = bn;
        const float seed = std_maxf(vLast, zv);
        vLast = r == 0 ? zv : (r == 1 ? seed : vLast);
        continuous &= (r != 1) | !(vLast <= 0);
        scan_step(zv, vLast, continuous, r != 0);
    };
#pragma unroll 1
    for (int r = 0; r < kCell / 2; ++r)
        stream_row(r);
    // row 10: the horizontal scan takes each piece's four steps right behind its arithmetic, then the piece is refilled
    {
        const int r = kCell / 2;
        float hLast = 0.0f;
#pragma unroll
        for (int j = 0; j < kQuads; ++j)
        {
            const float4 v = to_f4(buf[j]);
            buf[j] = load_piece(r + 1, j);
            acc_piece(v, j, b);
            if (j == 0)
            {
                hLast = std_maxf(v.x, v.y);
                continuous &= !(hLast <= 0);
            }
            else
            {
                scan_step(v.x, hLast, continuous, true);
            }
            scan_step(v.y, hLast, continuous, true);
            scan_step(v.z, hLast, continuous, true);
            scan_step(v.w, hLast, continuous, true);
            if (j == 2)
            {
                zc = v.z;
                scan_step(v.z, vLast, continuous, true);
            }
        }
        b = brow_at(r + 1); // (behind the scans, which leave no register pair for it)
    }
#pragma unroll 1
    for (int r = kCell / 2 + 1; r < kCell - 1; ++r)
        stream_row(r);
    // row 19: nothing left to load, no scan step (the vertical scan stops before it)
    float z399;
#pragma unroll
    for (int j = 0; j < kQuads; ++j)
    {
        const float4 v = to_f4(buf[j]);
        acc_piece(v, j, b);
        z399 = v.w;
    }

    // ------------------------------------------------------------------ the lane's cell leaves
    // exactness guard: all addends of every sum within 2^20 of each other (see header)
    const uint32_t n = A.n;
    // back to depths: with n > 0 at least one pixel was valid, so the minimum is a real pattern - 1
    const float zmin = __uint_as_float(A.zminBits1 + 1u), zmax = __uint_as_float(A.zmaxBits);
    // (the cell's row and column once more, from the fresh index: a division per cell is cheaper than a register per loop)
    const size_t gcell = my_cell();
    const int ecell = (int)(gcell - (size_t)frame * p.cells);
    int hCells = p.hCells;
    asm volatile("" : "+s"(hCells)); // (opaque, or the prologue's reciprocal of it is what gets carried through the loops)
    const int eRow = ecell / hCells;
    const int eCol = ecell - eRow * hCells;
    const float rab = fmaxf(p.ratio_col[eCol], p.ratio_row[eRow]);
    // all pixels +0 or positive and finite (acc_px_fast's precondition), and their range within the exactness bound
    const bool exact_ok = A.zmaxBits <= 0x7F7FFFFFu && ((n == 0) || (zmax * rab <= 512.0f * zmin));

    CellAux aux;
    aux.z0 = z0;
    aux.z399 = z399;
    aux.flags = (n & kCountMask) | (continuous ? kAuxContinuous : 0u) | (exact_ok ? kAuxExact : 0u);
    aux.zc = zc;
    p.cell_aux[gcell] = aux;
    double2* dst = reinterpret_cast<double2*>(p.cell_sums + gcell * kSumStride);
    static_assert(kSumStride == 10, "nine sums and the count: five 16-B stores");
    if constexpr (!FUSED)
    {
        dst[0] = make_double2(A.S[0], A.S[1]);
        dst[1] = make_double2(A.S[2], A.S[3]);
        dst[2] = make_double2(A.S[4], A.S[5]);
        dst[3] = make_double2(A.S[6], A.S[7]);
        dst[4] = make_double2(A.S[8], (double)n);
    }
    else
    {
        // The lane carries on with its cell: the fit on the sums it holds (the column factors' 40 registers are free by now),
        // the sums stored ONCE -- cleared or redone in pixel order where the fit says so --, and the workgroup, which is one
        // tile of stage A2 (256 consecutive cells = whole cell rows of one frame), does what such a tile does behind the fit.
        __shared__ CellPub s_pub[kThreadsCells];
        // (the lane's place in the workgroup from the fresh cell index, like everything else down here: a frame is whole workgroups)
        const int tid = (int)((uint32_t)ecell % (uint32_t)kThreadsCells);
        if (frame == 0 && ecell == 0)
            clear_grow_counters(p);
        CellFit cf;
        cell_fit_and_bin(p, frame, eRow, eCol, aux, A.S, cf);
        dst[0] = make_double2(A.S[0], A.S[1]);
        dst[1] = make_double2(A.S[2], A.S[3]);
        dst[2] = make_double2(A.S[4], A.S[5]);
        dst[3] = make_double2(A.S[6], A.S[7]);
        dst[4] = make_double2(A.S[8], (double)cf.n);
        tile_publish_and_finish(p, s_pub, tid, hCells, tid / hCells, eCol, true, gcell, cf);
    }
}

// The fused instance runs where its workgroups ARE the tiles of stage A2's 256-thread instance: 256 lanes, whole cell rows per
// workgroup, whole workgroups per frame -- no workgroup straddles a frame, no wave is partial, no lane is without a cell.
bool cell_fused_eligible(const StageAParams& p)
{
    return kThreadsCells == 256 && p.hCells > 0 && p.hCells <= 256 && 256 % p.hCells == 0 && p.cells % 256 == 0;
}

// stage A in one launch: A1's lanes fit their cells (the caller has checked that the split path would run the 256-thread A2)
hipError_t launch_cell_fused(const StageAParams& p, int nFrames, hipStream_t stream)
{
    // the kernel has no way out ahead of its barrier: it must never see a grid with a lane to spare
    if (!cell_fused_eligible(p) || p.a1Bands)
        return hipErrorInvalidConfiguration;
    constexpr int kWaves = kThreadsCells / 64;
    const int grid = nFrames * (p.cells / kThreadsCells);
    if (p.depth)
        hipLaunchKernelGGL((cape_cell_moments_kernel<false, true>), dim3(grid), dim3(kThreadsCells), 0, stream, p, grid * kWaves);
    else
        hipLaunchKernelGGL((cape_cell_moments_kernel<true, true>), dim3(grid), dim3(kThreadsCells), 0, stream, p, grid * kWaves);
    return hipGetLastError();
}

// every launch helper reports its own failure: hipGetLastError() right behind the launch (a later runtime call would
// overwrite the sticky-free error state on ROCm < 7)
hipError_t launch_cell_moments(const StageAParams& p, int nFrames, hipStream_t stream)
{
    if (p.a1Bands)
    {
        const int grid = nFrames * p.pairsPerFrame;
        if (p.depth)
            hipLaunchKernelGGL(cape_cell_moments_bands_kernel<false>, dim3(grid), dim3(kThreadsA), 0, stream, p);
        else
            hipLaunchKernelGGL(cape_cell_moments_bands_kernel<true>, dim3(grid), dim3(kThreadsA), 0, stream, p);
        return hipGetLastError();
    }
    // one wave per 64 cells of a frame, kThreadsCells / 64 independent waves per workgroup
    constexpr int kWaves = kThreadsCells / 64;
    const int waves = nFrames * ((p.cells + 63) / 64); // (cells <= 65535 per frame: far from 2^31 for any batch that fits the device)
    const int grid = (waves + kWaves - 1) / kWaves;
    if (p.depth)
        hipLaunchKernelGGL((cape_cell_moments_kernel<false, false>), dim3(grid), dim3(kThreadsCells), 0, stream, p, waves);
    else
        hipLaunchKernelGGL((cape_cell_moments_kernel<true, false>), dim3(grid), dim3(kThreadsCells), 0, stream, p, waves);
    return hipGetLastError();
}

} // namespace cape
