// The map polygon seen from a frame's camera, shared by the map matcher (cape_match_map.hip) and the visibility kernels
// (cape_map_visibility.hip): to_camera_space of the polygon's frame and of one ring vertex.  Both files compile their own copy
// (anonymous namespace; no device symbol crosses a file).
#pragma once
#include <hip/hip_runtime.h>

#include "cape_internal.h"

namespace cape {

namespace {

// to_camera_space of the map polygon's frame (polygon_coordinates.cpp:135-165): the centre through the transform, the axes through
// its rotation, re-normalised -- the statements of the pose path of cape_match_polygon.hip
struct CameraFrame
{
    double qc[3], qx[3], qy[3]; // the map polygon's own frame
    double nc[3], nx[3], ny[3]; // ... seen from the camera
};
__device__ __forceinline__ CameraFrame camera_frame(const double* Tm, const cape_map_plane& M)
{
    CameraFrame F;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        F.qc[r] = M.center[r], F.qx[r] = M.x_axis[r], F.qy[r] = M.y_axis[r];
#pragma unroll
    for (int r = 0; r < 3; ++r)
    {
        F.nc[r] = ((Tm[4 * r] * F.qc[0] + Tm[4 * r + 1] * F.qc[1]) + Tm[4 * r + 2] * F.qc[2]) + Tm[4 * r + 3];
        F.nx[r] = (Tm[4 * r] * F.qx[0] + Tm[4 * r + 1] * F.qx[1]) + Tm[4 * r + 2] * F.qx[2];
        F.ny[r] = (Tm[4 * r] * F.qy[0] + Tm[4 * r + 1] * F.qy[1]) + Tm[4 * r + 2] * F.qy[2];
    }
    const double lx = sqrt((F.nx[0] * F.nx[0] + F.nx[1] * F.nx[1]) + F.nx[2] * F.nx[2]), ly = sqrt((F.ny[0] * F.ny[0] + F.ny[1] * F.ny[1]) + F.ny[2] * F.ny[2]);
    if (lx > 0)
        F.nx[0] /= lx, F.nx[1] /= lx, F.nx[2] /= lx;
    if (ly > 0)
        F.ny[0] /= ly, F.ny[1] /= ly, F.ny[2] /= ly;
    return F;
}

// one vertex of a map ring seen from the camera, in the camera-space frame (transform_boundary, polygon.cpp:430-451)
__device__ __forceinline__ double2 to_camera_vertex(const double* Tm, const CameraFrame& F, double2 q)
{
    const double X = F.qc[0] + q.x * F.qx[0] + q.y * F.qy[0], Y = F.qc[1] + q.x * F.qx[1] + q.y * F.qy[1], Z = F.qc[2] + q.x * F.qx[2] + q.y * F.qy[2];
    const double mx = ((Tm[0] * X + Tm[1] * Y) + Tm[2] * Z) + Tm[3], my = ((Tm[4] * X + Tm[5] * Y) + Tm[6] * Z) + Tm[7],
                 mz = ((Tm[8] * X + Tm[9] * Y) + Tm[10] * Z) + Tm[11];
    const double dx = mx - F.nc[0], dy = my - F.nc[1], dz = mz - F.nc[2];
    return make_double2((F.nx[0] * dx + F.nx[1] * dy) + F.nx[2] * dz, (F.ny[0] * dx + F.ny[1] * dy) + F.ny[2] * dz);
}

} // namespace

} // namespace cape
