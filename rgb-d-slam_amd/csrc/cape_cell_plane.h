// Stage A behind a cell's last pixel, shared by every kernel that fits cell planes: the fused instance of the lane-per-cell
// kernel (cape_cell_moments.hip), the split kernel A2 and the strip kernel (both cape_cell_fit.hip).  One copy of every step:
// what is decided for ONE cell from its moment sums (cell_fit_and_bin) and what a workgroup of one lane per cell does with its
// cells' planes afterwards (tile_publish_and_finish).
#pragma once
#include <hip/hip_runtime.h>

#include "cape_cell_acc.h"

namespace cape {

#ifndef CAPE_A2_ABLATE
#define CAPE_A2_ABLATE 0
#endif
// What stage A2 decides for ONE cell from its moment sums and stage A1's verdicts: the in-order redo of a cell whose sums are
// not provably exact, the validity gates, Plane_Segment::fit_plane, the merge tolerance and the histogram bin.
struct CellFit
{
    PlaneFit f;
    bool planar;
    float tol;
    int bin;
    uint32_t nearEdge, inorder, n;
    bool rewrite; // S / n differ from what stage A1 summed (cleared, or redone in order): the caller stores them
};
__device__ __forceinline__ void cell_fit_and_bin(const StageAParams& p, int frame, int cellRow, int cellCol, const CellAux& aux, double (&S)[9],
                                                 CellFit& o)
{
    PlaneFit f;
    f.planar = false;
    f.nx = f.ny = f.nz = f.d = 0.0;
    f.cx = f.cy = f.cz = 0.0;
    f.mse = kDblMax;
    f.score = 0.0;
    bool planar = false;
    float tol = 0.0f;
    int bin = -1;
    uint32_t nearEdge = 0, inorder = 0;
    uint32_t n = aux.flags & kCountMask;
    const bool continuous = (aux.flags & kAuxContinuous) != 0;
    const bool exact_ok = (aux.flags & kAuxExact) != 0;
    bool rewrite = false;
    if (!exact_ok && continuous && n >= (uint32_t)(kPts / 2))
    {
        // in-order path: the reference's pixel order (plane_segment.cpp:131-152)
        inorder = 1;
        rewrite = true;
        const size_t cellOff = (size_t)frame * p.W * p.H + (size_t)(cellRow * kCell) * p.W + cellCol * kCell;
        PxAcc A;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            A.S[k] = 0.0;
        A.n = 0;
        A.zminBits1 = 0;
        A.zmaxBits = 0;
        for (int r = 0; r < kCell; ++r)
        {
            const double b = p.brow[cellRow * kCell + r];
            for (int c = 0; c < kCell; ++c)
            {
                const size_t o = cellOff + (size_t)r * p.W + c;
                const float zr = p.depth ? p.depth[o] : (float)p.depth_u16[o] * p.u16_scale;
                acc_px(zr, p.acol[cellCol * kCell + c], b, A);
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k)
            S[k] = A.S[k];
        n = A.n;
    }

    if (!continuous || n < (uint32_t)(kPts / 2))
    {
        // plane_segment.cpp:114-123: returns right after clear_plane_parameters()
#pragma unroll
        for (int k = 0; k < 9; ++k)
            S[k] = 0.0;
        n = 0;
        rewrite = true;
    }
    // (CAPE_A2_ABLATE: timing experiments only -- profiles/a2_ablation.sh builds one library per bit and reports what
    //  each part of the kernel costs; results of such a build are wrong by construction.  1 = no plane fit,
    //  2 = no histogram bin (acos / atan2), 4 = no edge predicates, 8 = no tolerance)
    else if (n >= (uint32_t)p.minZeroPointCount && !(CAPE_A2_ABLATE & 1))
    {
        fit_plane(S, n, f);
        const double qz = depth_quantization(f.cz);
        planar = f.mse <= qz * qz; // plane_segment.cpp:167
    }

    // _cellDistanceTols (primitive_detection.cpp:201-220): first and last cloud rows of the cell (zeros if invalid)
    if ((CAPE_A2_ABLATE & 1) && n >= (uint32_t)p.minZeroPointCount)
    {
        planar = S[2] > 0.0; // keep the downstream work alive without the fit
        f.nx = S[0] * 1e-9, f.ny = S[1] * 1e-9, f.nz = -0.5, f.d = S[2] * 1e-6, f.cx = S[0] / n, f.cy = S[1] / n, f.cz = S[2] / n;
    }
    if (planar)
    {
        const float z0 = aux.z0, z1 = aux.z399;
        const int u0 = cellCol * kCell, v0 = cellRow * kCell;
        float x0 = 0, y0 = 0, zz0 = 0, x1 = 0, y1 = 0, zz1 = 0;
        if (z0 > 0)
        {
            x0 = (float)((double)z0 * p.acol[u0]);
            y0 = (float)((double)z0 * p.brow[v0]);
            zz0 = z0;
        }
        if (z1 > 0)
        {
            x1 = (float)((double)z1 * p.acol[u0 + kCell - 1]);
            y1 = (float)((double)z1 * p.brow[v0 + kCell - 1]);
            zz1 = z1;
        }
        const float dx = x1 - x0, dy = y1 - y0, dz = zz1 - zz0;
        const float diam = (CAPE_A2_ABLATE & 8) ? dx : sqrtf(dx * dx + (dy * dy + dz * dz));
        tol = (CAPE_A2_ABLATE & 8) ? diam : std_minf(50.0f, diam * p.sinMerge * sqrtf((float)n));

        // init_histogram (primitive_detection.cpp:253-254) + Histogram::init_histogram (histogram.hpp:48-54)
        const double theta = (CAPE_A2_ABLATE & 2) ? -f.nz : acos(-f.nz);
        const double phi = (CAPE_A2_ABLATE & 2) ? f.nx : atan2(f.nx, f.ny);
        constexpr double kPi = 3.14159265358979323846;
        const double tx = 19.0 * (theta - 0.0) / kPi;
        const int xQ = (int)floor(tx);
        int yQ = 0;
        double ty = 0.5;
        if (xQ > 0)
        {
            ty = 19.0 * (phi - (-kPi)) / (kPi - (-kPi));
            yQ = (int)floor(ty);
        }
        bin = yQ * 20 + xQ;
        // libm tie guard: ocml vs glibc acos/atan2 may differ in the last ulp
        if (fabs(tx - rint(tx)) < 1e-9 || (xQ > 0 && fabs(ty - rint(ty)) < 1e-9))
            nearEdge = 1;
    }
    o.f = f;
    o.planar = planar;
    o.tol = tol;
    o.bin = bin;
    o.nearEdge = nearEdge;
    o.inorder = inorder;
    o.n = n;
    o.rewrite = rewrite;
}

// A workgroup owns a TILE of whole cell rows of one frame (THREADS cells at most, one lane per cell).  After the fit every
// cell publishes its plane (normal, d, centroid, merge tolerance) in LDS, and each lane evaluates region_growing's merge
// predicate for the directed edges to its left and upper neighbours -- the planes are still in registers here, whereas
// the grow kernel had to read all of them back (64 B per cell, a dozen exposed memory round trips per frame) to do the
// same.  Tiles are independent workgroups: the edges between the first row of a tile and the row above it (another
// workgroup's) are left to the grow kernel, which evaluates just those rows (2 of 23 row boundaries at 640x480).
// THREADS = 256 is the throughput instance of A2 and the workgroup of the fused A1 instance; THREADS = 1024 (A2 only) takes a
// 640x480 frame in a single tile and is launched for small batches, where the latency of one frame is what matters.
struct CellPub
{
    double nx, ny, nz, d, cx, cy, cz, tol;
};

// The block behind the fit, for a workgroup whose lane `tid` holds the fitted cell (lrow, cellCol) of its tile (`valid`: the
// lane holds a cell at all): publish, ONE barrier -- every lane of the workgroup must arrive here --, the merge predicates
// towards the left and upper neighbours, and the cell's plane, MSE, score, tolerance, bin and flags go to memory.
__device__ __forceinline__ void tile_publish_and_finish(const StageAParams& p, CellPub* s_pub, int tid, int HC, int lrow, int cellCol, bool valid,
                                                         size_t gcell, const CellFit& cf)
{
    const PlaneFit& f = cf.f;
    const bool planar = cf.planar;
    const float tol = cf.tol;
    const int bin = cf.bin;
    const uint32_t nearEdge = cf.nearEdge, inorder = cf.inorder, n = cf.n;

    // ---- publish, then the merge predicate of the directed edges to the left and upper neighbours
    CellPub me;
    me.nx = f.nx; me.ny = f.ny; me.nz = f.nz; me.d = f.d;
    me.cx = f.cx; me.cy = f.cy; me.cz = f.cz; me.tol = (double)tol;
    s_pub[tid] = me;
    __syncthreads();
    uint32_t edges = 0;
    if (valid)
    {
        if (cellCol > 0 && !(CAPE_A2_ABLATE & 4))
        {
            const CellPub L = s_pub[tid - 1];
            if (can_be_merged(L.nx, L.ny, L.nz, L.d, me.nx, me.ny, me.nz, me.cx, me.cy, me.cz, me.tol, p.cosMergeA))
                edges |= kFlagLeftToMe;
            if (can_be_merged(me.nx, me.ny, me.nz, me.d, L.nx, L.ny, L.nz, L.cx, L.cy, L.cz, L.tol, p.cosMergeA))
                edges |= kFlagMeToLeft;
        }
        if (lrow > 0 && !(CAPE_A2_ABLATE & 4)) // the tile's first row: its upper neighbours belong to another workgroup (see above)
        {
            const CellPub Up = s_pub[tid - HC];
            if (can_be_merged(Up.nx, Up.ny, Up.nz, Up.d, me.nx, me.ny, me.nz, me.cx, me.cy, me.cz, me.tol, p.cosMergeA))
                edges |= kFlagUpToMe;
            if (can_be_merged(me.nx, me.ny, me.nz, me.d, Up.nx, Up.ny, Up.nz, Up.cx, Up.cy, Up.cz, Up.tol, p.cosMergeA))
                edges |= kFlagMeToUp;
        }
        double* op = p.cell_plane + gcell * kPlaneStride;
        op[0] = f.nx; op[1] = f.ny; op[2] = f.nz; op[3] = f.d;
        op[4] = f.cx; op[5] = f.cy; op[6] = f.cz; op[7] = f.mse;
        p.cell_mse[gcell] = f.mse;
        p.cell_score[gcell] = f.score;
        p.cell_tol[gcell] = tol;
        p.cell_bins[gcell] = bin;
        p.cell_flags[gcell] = (n & kCountMask) | edges | (nearEdge ? kFlagNearEdge : 0u) | (inorder ? kFlagInorder : 0u) |
                              (planar ? kFlagPlanar : 0u);
    }
}

// The hand-over counters of the grow kernel, zeroed by one thread of whichever kernel ends stage A (StageAParams::clear0..4)
__device__ __forceinline__ void clear_grow_counters(const StageAParams& p)
{
    if (p.clear0)
        *p.clear0 = 0u;
    if (p.clear1)
        *p.clear1 = 0u;
    if (p.clear2)
    {
        *p.clear2 = 0u;
        if (p.clear2Buckets)
            for (int c = 1; c <= kResumeClasses; ++c)
                p.clear2[(size_t)c * p.clear2Buckets] = 0u;
    }
    if (p.clear3)
        *p.clear3 = 0u;
    if (p.clear4)
        p.clear4[0] = p.clear4[1] = 0u; // records handed out of the spill pool, frames through the general instance
}

} // namespace cape
