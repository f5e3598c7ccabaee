// Test hook: the host boundary-polygon class behind a C entry point, so that tests/test_gpu_polygon.py can compare the
// device polygons (cape_build_polygons) with it vertex for vertex through ctypes.  Not part of the product's C ABI.
#include <cmath>
#include <cstring>
#include <exception>
#include <vector>

#include "boundary_polygon.hpp"
#include "cape_hip.h"

extern "C" int cape_host_polygon(const double* points3, int n, const double* normal, const double* center, double* ring_out, int capacity,
                                 int* count_out, double* area_out, double* x_axis_out, double* y_axis_out, int* valid_out)
{
    using rgbd_slam::vector3;
    try
    {
        std::vector<vector3> pts;
        pts.reserve(n);
        for (int i = 0; i < n; ++i)
            pts.emplace_back(points3[3 * i], points3[3 * i + 1], points3[3 * i + 2]);
        const rgbd_slam::utils::Polygon poly(pts, vector3(normal[0], normal[1], normal[2]), vector3(center[0], center[1], center[2]));
        const auto& ring = poly.boundary();
        *count_out = static_cast<int>(ring.size());
        for (size_t i = 0; i < ring.size() && static_cast<int>(i) < capacity; ++i)
        {
            ring_out[2 * i] = ring[i][0];
            ring_out[2 * i + 1] = ring[i][1];
        }
        *area_out = poly.get_area();
        for (int k = 0; k < 3; ++k)
        {
            x_axis_out[k] = poly.get_x_axis()[k];
            y_axis_out[k] = poly.get_y_axis()[k];
        }
        *valid_out = (poly.is_valid() && poly.boundary_length() >= 3) ? 1 : 0;
        return 0;
    }
    catch (const std::exception&)
    {
        *count_out = 0;
        *valid_out = 0;
        return 1; // the constructor threw: fewer than 3 points / normal not unit
    }
}

// Polygon::inter_area of two polygons given by their rings and frames (the public explicit-ring constructor, like the overlay
// builds its CameraPolygons from the device's vertices): `a` is the detected polygon, `b` the projected one
// (map_primitive.cpp:137).  tests/test_gpu_match_polygon.py compares cape_match_polygons with it bit for bit.
extern "C" double cape_host_polygon_inter_area(const double* ring_a, int na, const double* x_a, const double* y_a, const double* c_a,
                                               const double* ring_b, int nb, const double* x_b, const double* y_b, const double* c_b,
                                               double* area_a_out, double* area_b_out)
{
    using rgbd_slam::vector2;
    using rgbd_slam::vector3;
    std::vector<vector2> ra, rb;
    for (int i = 0; i < na; ++i)
        ra.emplace_back(ring_a[2 * i], ring_a[2 * i + 1]);
    for (int i = 0; i < nb; ++i)
        rb.emplace_back(ring_b[2 * i], ring_b[2 * i + 1]);
    const rgbd_slam::utils::Polygon a(ra, vector3(x_a[0], x_a[1], x_a[2]), vector3(y_a[0], y_a[1], y_a[2]), vector3(c_a[0], c_a[1], c_a[2]));
    const rgbd_slam::utils::Polygon b(rb, vector3(x_b[0], x_b[1], x_b[2]), vector3(y_b[0], y_b[1], y_b[2]), vector3(c_b[0], c_b[1], c_b[2]));
    if (area_a_out)
        *area_a_out = a.get_area();
    if (area_b_out)
        *area_b_out = b.get_area();
    return a.inter_area(b);
}

// The same with the projected polygon seen through a pose first: a.inter_area(b.to_camera_space(worldToCamera))
// (map_primitive.cpp:103 then :137); plane_in / plane_out: (nx, ny, nz, d) of the map plane before / after
// to_camera_coordinates (map_primitive.cpp:100-101).  tests/test_gpu_match_pose.py compares cape_match_polygons_pose with it.
extern "C" double cape_host_polygon_inter_area_pose(const double* ring_a, int na, const double* x_a, const double* y_a, const double* c_a,
                                                    const double* ring_b, int nb, const double* x_b, const double* y_b, const double* c_b,
                                                    const double* world_to_camera, const double* plane_in, double* plane_out)
{
    using rgbd_slam::vector2;
    using rgbd_slam::vector3;
    std::vector<vector2> ra, rb;
    for (int i = 0; i < na; ++i)
        ra.emplace_back(ring_a[2 * i], ring_a[2 * i + 1]);
    for (int i = 0; i < nb; ++i)
        rb.emplace_back(ring_b[2 * i], ring_b[2 * i + 1]);
    const rgbd_slam::utils::Polygon a(ra, vector3(x_a[0], x_a[1], x_a[2]), vector3(y_a[0], y_a[1], y_a[2]), vector3(c_a[0], c_a[1], c_a[2]));
    const rgbd_slam::utils::Polygon b(rb, vector3(x_b[0], x_b[1], x_b[2]), vector3(y_b[0], y_b[1], y_b[2]), vector3(c_b[0], c_b[1], c_b[2]));
    if (plane_in && plane_out)
        rgbd_slam::utils::plane_to_camera(plane_in, plane_in[3], world_to_camera, plane_out, plane_out + 3);
    return a.inter_area(b.to_camera_space(world_to_camera));
}

// MapPlane::find_matches (map_primitive.cpp:91-161) as Feature_Map::get_matches drives it (feature_map.hpp:647-670), for ONE
// frame on the host class: the twin of cape_match_map (tests/test_gpu_map_match.py compares them bit for bit) and the answer
// for a frame the device flags CAPE_MATCH_EXACT_OVERFLOW.  The map is given as to cape_map_upload; the detected planes as the
// frame's kept planes: det_planes = n_det x (normal[3], d), det_frames = n_det x (x_axis[3], y_axis[3], center[3]), their rings
// one after the other in det_vertices (det_counts[i] vertices each), det_areas = the polygons' get_area() (NULL: the area of the
// ring).  world_to_camera: 16 doubles row-major (NULL = identity); skip: ceil(n_planes / 32) words (NULL: none skipped).
// Outputs: match[n_planes], map_of[n_det], inter_area[n_planes x n_det] (NULL: not kept) -- the area of every gated pair of a
// visited map plane with a positive projected area, -1 elsewhere.  Returns 0, or CAPE_ERR_INVALID_ARGUMENT for a ring outside
// its array / of fewer than 3 vertices or a map plane without rings.
extern "C" int cape_host_match_map(const cape_map_plane* planes, int32_t n_planes, const cape_map_ring* rings, int32_t n_rings,
                                   const double* vertices, int64_t n_vertices, int32_t n_det, const double* det_planes,
                                   const double* det_frames, const double* det_areas, const double* det_vertices, const int32_t* det_counts,
                                   const double* world_to_camera, const uint32_t* skip, uint32_t flags, int32_t* match, int32_t* map_of,
                                   double* inter_area)
{
    using rgbd_slam::vector2;
    using rgbd_slam::vector3;
    using rgbd_slam::utils::Polygon;
    static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double* T = world_to_camera ? world_to_camera : kIdentity;
    const double minCos = std::abs(std::cos(20.0 * M_PI / 180.0)); // parameters.hpp:92-93, shape_primitives.cpp:72-73
    const double maxDistance = 100.0;                              // parameters.hpp:94-95
    const double overlap = (flags & CAPE_MATCH_ADVANCED) ? static_cast<double>(0.4f) / 2 : static_cast<double>(0.4f);
    try
    {
        std::vector<Polygon> det;
        std::vector<double> detArea;
        size_t at = 0;
        for (int32_t i = 0; i < n_det; ++i)
        {
            std::vector<vector2> ring;
            for (int32_t v = 0; v < det_counts[i]; ++v, ++at)
                ring.emplace_back(det_vertices[2 * at], det_vertices[2 * at + 1]);
            const double* F = det_frames + 9 * i;
            det.emplace_back(ring, vector3(F[0], F[1], F[2]), vector3(F[3], F[4], F[5]), vector3(F[6], F[7], F[8]));
            detArea.push_back(det_areas ? det_areas[i] : det.back().get_area());
        }
        auto ring_of = [&](uint32_t r, std::vector<vector2>& out) {
            if (r >= (uint32_t)n_rings || rings[r].vertex_count < 3 || (int64_t)rings[r].vertex_offset + rings[r].vertex_count > n_vertices)
                return false;
            out.clear();
            for (uint32_t v = 0; v < rings[r].vertex_count; ++v)
            {
                const double* q = vertices + 2 * ((size_t)rings[r].vertex_offset + v);
                out.emplace_back(q[0], q[1]);
            }
            return true;
        };
        std::vector<char> matched(n_det, 0);
        for (int32_t i = 0; i < n_det; ++i)
            map_of[i] = -1;
        for (int32_t j = 0; j < n_planes; ++j)
        {
            match[j] = -1;
            if (inter_area)
                for (int32_t i = 0; i < n_det; ++i)
                    inter_area[(size_t)j * n_det + i] = -1.0;
        }
        for (int32_t j = 0; j < n_planes; ++j)
        {
            const cape_map_plane& M = planes[j];
            if (M.ring_count == 0)
                return CAPE_ERR_INVALID_ARGUMENT;
            std::vector<vector2> outer;
            std::vector<std::vector<vector2>> holes(M.ring_count - 1);
            if (!ring_of(M.ring_first, outer))
                return CAPE_ERR_INVALID_ARGUMENT;
            for (uint32_t k = 1; k < M.ring_count; ++k)
                if (!ring_of(M.ring_first + k, holes[k - 1]))
                    return CAPE_ERR_INVALID_ARGUMENT;
            if (skip && ((skip[j >> 5] >> (j & 31)) & 1u)) // is_moving() or not is_visible(worldToCamera): not visited
                continue;
            const Polygon mapPolygon(outer, holes, vector3(M.x_axis[0], M.x_axis[1], M.x_axis[2]), vector3(M.y_axis[0], M.y_axis[1], M.y_axis[2]),
                                     vector3(M.center[0], M.center[1], M.center[2]));
            double pn[3], pd;
            rgbd_slam::utils::plane_to_camera(M.normal, M.d, T, pn, &pd);
            const Polygon projected = mapPolygon.to_camera_space(T);
            if (projected.get_area() <= 0.0)
                continue;
            int selected = -1;
            double greatest = 0.0;
            for (int32_t i = 0; i < n_det; ++i)
            {
                const double* dn = det_planes + 4 * i;
                const double cosAngle = (dn[0] * pn[0] + dn[1] * pn[1]) + dn[2] * pn[2];
                if (!(std::abs(dn[3] - pd) < maxDistance) || !(std::abs(cosAngle) > minCos))
                    continue;
                const double ia = det[i].inter_area(projected);
                if (inter_area)
                    inter_area[(size_t)j * n_det + i] = ia;
                if (matched[i])
                    continue;
                if (ia > greatest && ia / detArea[i] >= overlap)
                {
                    selected = i;
                    greatest = ia;
                }
            }
            if (selected < 0 || (selected == 0 && !(flags & CAPE_MATCH_ALLOW_INDEX0))) // map_primitive.cpp:146
                continue;
            match[j] = selected;
            matched[selected] = 1;
            map_of[selected] = j;
        }
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}
