// A polygon seen from a frame's camera, shared by the map matcher (cape_match_map.hip), the visibility kernels
// (cape_map_visibility.hip), the pose path of the consecutive matchers (cape_match_polygon.hip, cape_match_wide.hip: the previous
// frame's polygon) and -- with the camera-to-world matrix, a detected polygon carried to the world -- the measurement kernel
// (cape_map_measure.hip): plane_to_camera of the plane, to_camera_space of the polygon's frame and of one ring vertex.  Every file
// compiles its own copy (anonymous namespace; no device symbol crosses a file).
#pragma once
#include <hip/hip_runtime.h>

#include "cape_internal.h"

namespace cape {

namespace {

// A plane (normal, d) through a transform: PlaneWorldCoordinates::to_camera_coordinates with the plane matrix [R 0; -t^T R 1]
// (camera_transformation.cpp:53-71); the PlaneCameraCoordinates constructor normalises the rotated normal (host:
// utils::plane_to_camera).  With the camera-to-world matrix it is the host's plane_to_world (cape_map_measure.hip).
__device__ __forceinline__ void plane_to_camera(const double* T, const double* normal, double d, double pn[3], double& pd)
{
    const double n0 = normal[0], n1 = normal[1], n2 = normal[2];
    const double r0 = (T[0] * n0 + T[1] * n1) + T[2] * n2, r1 = (T[4] * n0 + T[5] * n1) + T[6] * n2, r2 = (T[8] * n0 + T[9] * n1) + T[10] * n2;
    const double t0 = T[3], t1 = T[7], t2 = T[11];
    const double m0 = -((t0 * T[0] + t1 * T[4]) + t2 * T[8]), m1 = -((t0 * T[1] + t1 * T[5]) + t2 * T[9]), m2 = -((t0 * T[2] + t1 * T[6]) + t2 * T[10]);
    pd = ((m0 * n0 + m1 * n1) + m2 * n2) + d;
    const double nn = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    pn[0] = r0, pn[1] = r1, pn[2] = r2;
    if (nn > 0)
        pn[0] = r0 / nn, pn[1] = r1 / nn, pn[2] = r2 / nn;
}

// to_camera_space of a polygon's frame (polygon_coordinates.cpp:135-165): the centre through the transform, the axes through
// its rotation, re-normalised
struct CameraFrame
{
    double qc[3], qx[3], qy[3]; // the polygon's own frame
    double nc[3], nx[3], ny[3]; // ... seen from the camera
};
__device__ __forceinline__ CameraFrame camera_frame(const double* Tm, const double* center, const double* xAxis, const double* yAxis)
{
    CameraFrame F;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        F.qc[r] = center[r], F.qx[r] = xAxis[r], F.qy[r] = yAxis[r];
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
__device__ __forceinline__ CameraFrame camera_frame(const double* Tm, const cape_map_plane& M)
{
    return camera_frame(Tm, M.center, M.x_axis, M.y_axis);
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
