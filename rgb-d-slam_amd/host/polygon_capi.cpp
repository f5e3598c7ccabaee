// C entry points of libcape_primitives.so over the host boundary-polygon class.  None of them is part of libcape_hip's C ABI
// (include/cape_hip.h).  cape_host_polygon, cape_host_polygon_inter_area* and the cape_host_covariance / kalman hooks at the
// end are test hooks: the tests compare the device (or a numpy restatement) with them through ctypes.  cape_host_match_map,
// cape_host_match_planes, cape_host_map_visibility, cape_host_map_update and cape_host_shard_frame are host twins a caller may use,
// declared and described in cape_host_map.h: the first answers the frames cape_match_map flags, the second those the matchers of
// consecutive frames flag, the third decides which map planes cape_match_map visits, the fourth is the map update (cape_host_map_kalman and cape_host_map_union are the
// twins of its two device halves, cape_host_map_union_holes of the polygon half's holes mode, cape_host_map_commit of the commit that follows them, cape_host_map_maintain of the list maintenance behind it, cape_host_ring_union and cape_host_polygon_union of the union's debug entries), the fifth reads a gathered shard.  They share the conversions of the anonymous namespace below.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <limits>
#include <stdexcept>
#include <vector>

#include "boundary_polygon.hpp"
#include "map_tracking.hpp"
#include "cape_hip.h"
#include "cape_host_map.h"
#include "../csrc/cape_map_commit.h" // the commit's per-plane rules, shared with the plan kernel
#include "../csrc/cape_map_maintain.h" // the list maintenance's, likewise

namespace {

using rgbd_slam::vector2;
using rgbd_slam::vector3;
using rgbd_slam::utils::Polygon;

vector3 vec3(const double* p) { return vector3(p[0], p[1], p[2]); }
void put3(double* out, const vector3& v) { out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; }

// n (x, y) pairs as a ring of the host class
std::vector<vector2> ring_from(const double* xy, size_t n)
{
    std::vector<vector2> ring;
    for (size_t v = 0; v < n; ++v)
        ring.emplace_back(xy[2 * v], xy[2 * v + 1]);
    return ring;
}

// The polygon of map plane M: outer ring, holes, axes, centre (out NULL: the rings are checked, no polygon is built).  False for a
// plane without rings, a ring outside its array or one of fewer than 3 vertices.
bool map_polygon(const cape_host_map& map, const cape_map_plane& M, Polygon* out)
{
    if (M.ring_count == 0 || (uint64_t)M.ring_first + M.ring_count > (uint64_t)std::max(map.n_rings, 0))
        return false;
    std::vector<std::vector<vector2>> rings(M.ring_count);
    for (uint32_t k = 0; k < M.ring_count; ++k)
    {
        const cape_map_ring& R = map.rings[M.ring_first + k];
        if (R.vertex_count < 3 || (int64_t)R.vertex_offset + R.vertex_count > map.n_vertices)
            return false;
        rings[k] = ring_from(map.vertices + 2 * (size_t)R.vertex_offset, R.vertex_count);
    }
    if (out)
        *out = Polygon(rings[0], {rings.begin() + 1, rings.end()}, vec3(M.x_axis), vec3(M.y_axis), vec3(M.center));
    return true;
}

// A frame's kept planes as the host class's polygons.  False for a ring of fewer than min_count vertices or one that ends beyond
// n_vertices.
bool kept_polygons(const cape_host_planes& planes, int32_t min_count, std::vector<Polygon>& out)
{
    int64_t at = 0;
    for (int32_t i = 0; i < planes.n; ++i)
    {
        if (planes.counts[i] < min_count || at + planes.counts[i] > planes.n_vertices)
            return false;
        const double* F = planes.frames + 9 * i;
        out.emplace_back(ring_from(planes.vertices + 2 * at, planes.counts[i]), vec3(F), vec3(F + 3), vec3(F + 6));
        at += planes.counts[i];
    }
    return true;
}

// Row n of a frame's kept planes (its ring from vertex nv on) from the packed plane, its packed polygon and the host class's
// polygon of it; a NULL column is not written.
void put_kept_plane(const cape_host_planes& out, int32_t n, int64_t nv, const cape_packed_plane& pl, const cape_polygon& g, const Polygon& polygon)
{
    if (out.planes)
    {
        std::memcpy(out.planes + 4 * n, pl.normal, 3 * sizeof(double));
        out.planes[4 * n + 3] = pl.d;
    }
    if (out.cov)
    {
        // Plane_Segment::get_point_cloud_covariance: Matrix3d::inverse (cofactors) of {{Sxs,Sxy,Szx},{Sxy,Sys,Syz},{Szx,Syz,Szs}},
        // statement for statement what the grow kernels store in cape_plane_segment.cov
        const double* S = pl.sums;
        const double m[3][3] = {{S[3], S[6], S[8]}, {S[6], S[4], S[7]}, {S[8], S[7], S[5]}};
        const auto cof = [&](int i, int j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
        };
        const double c00 = cof(0, 0), c10 = cof(1, 0), c20 = cof(2, 0);
        const double det = (c00 * m[0][0] + c10 * m[1][0]) + c20 * m[2][0];
        const double invdet = 1.0 / det;
        double* r = out.cov + 9 * n;
        r[0] = c00 * invdet; r[1] = c10 * invdet; r[2] = c20 * invdet;
        for (int j = 1; j < 3; ++j)
            for (int i = 0; i < 3; ++i)
                r[3 * j + i] = cof(i, j) * invdet;
    }
    if (out.frames)
    {
        put3(out.frames + 9 * n, polygon.get_x_axis());
        put3(out.frames + 9 * n + 3, polygon.get_y_axis());
        std::memcpy(out.frames + 9 * n + 6, g.center, 3 * sizeof(double));
    }
    if (out.areas)
        out.areas[n] = polygon.get_area();
    if (out.vertices)
        for (uint32_t v = 0; v < g.vertex_count; ++v)
        {
            out.vertices[2 * (nv + v)] = polygon.boundary()[v][0];
            out.vertices[2 * (nv + v) + 1] = polygon.boundary()[v][1];
        }
    if (out.counts)
        out.counts[n] = (int32_t)g.vertex_count;
    if (out.segments)
        out.segments[n] = (int32_t)g.segment;
}

struct MapEntry
{
    cape_map_plane plane;
    cape_map_track track;
    Polygon polygon;
};

// The entries as a map in cape_map_upload's layout, each plane's frame and rings from its polygon.  The three counts are
// written either way; false, and nothing else written, if an array of `out` is too small or NULL.  `append` (the retired log): the
// entries go behind what `out` holds by its counts, which are advanced -- or, with false, left as they were.
bool put_map(std::vector<MapEntry>& entries, cape_host_map& out, bool append = false)
{
    const int32_t p0 = append ? out.n_planes : 0, r0 = append ? out.n_rings : 0;
    const int64_t v0 = append ? out.n_vertices : 0;
    int32_t nr = r0;
    int64_t nv = v0;
    for (const MapEntry& e : entries)
    {
        nr += 1 + (int32_t)e.polygon.interior_rings().size();
        nv += (int64_t)e.polygon.boundary().size();
        for (const auto& h : e.polygon.interior_rings())
            nv += (int64_t)h.size();
    }
    const bool fits = (int64_t)p0 + (int64_t)entries.size() <= out.planes_capacity && nr <= out.rings_capacity && nv <= out.vertices_capacity &&
                      out.planes && out.tracks && out.rings && out.vertices;
    if (!append || fits)
    {
        out.n_planes = p0 + (int32_t)entries.size();
        out.n_rings = nr;
        out.n_vertices = nv;
    }
    if (!fits)
        return false;
    int32_t r = r0;
    int64_t v = v0;
    for (size_t j = 0; j < entries.size(); ++j)
    {
        MapEntry& e = entries[j];
        put3(e.plane.x_axis, e.polygon.get_x_axis());
        put3(e.plane.y_axis, e.polygon.get_y_axis());
        put3(e.plane.center, e.polygon.get_center());
        e.plane.ring_first = (uint32_t)r;
        e.plane.ring_count = 1 + (uint32_t)e.polygon.interior_rings().size();
        auto put = [&](const std::vector<vector2>& ring) {
            out.rings[r].vertex_offset = (uint32_t)v;
            out.rings[r].vertex_count = (uint32_t)ring.size();
            ++r;
            for (const vector2& p : ring)
            {
                out.vertices[2 * v] = p[0];
                out.vertices[2 * v + 1] = p[1];
                ++v;
            }
        };
        put(e.polygon.boundary());
        for (const auto& h : e.polygon.interior_rings())
            put(h);
        out.planes[(size_t)p0 + j] = e.plane;
        out.tracks[(size_t)p0 + j] = e.track;
    }
    return true;
}

// Eigen's isApprox on 3-vectors: |a - b|^2 <= prec^2 min(|a|^2, |b|^2)
bool is_approx3(const vector3& a, const vector3& b)
{
    const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
    const double diff = (e0 * e0 + e1 * e1) + e2 * e2;
    const double na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double prec = 1e-12;
    return diff <= prec * prec * std::min(na, nb);
}

// CameraPolygon::to_world_space (polygon_coordinates.cpp:48-75): its norm and orthogonality checks, then the transform that
// to_camera_space restates with the camera-to-world matrix.  False where the reference throws.
bool to_world_space(const Polygon& p, const double* T, Polygon& out)
{
    using rgbd_slam::map_tracking::norm3;
    using rgbd_slam::map_tracking::normalize3;
    const vector3 x = p.get_x_axis(), y = p.get_y_axis();
    double nx[3] = {(T[0] * x[0] + T[1] * x[1]) + T[2] * x[2], (T[4] * x[0] + T[5] * x[1]) + T[6] * x[2], (T[8] * x[0] + T[9] * x[1]) + T[10] * x[2]};
    double ny[3] = {(T[0] * y[0] + T[1] * y[1]) + T[2] * y[2], (T[4] * y[0] + T[5] * y[1]) + T[6] * y[2], (T[8] * y[0] + T[9] * y[1]) + T[10] * y[2]};
    normalize3(nx);
    normalize3(ny);
    const double eps = std::numeric_limits<double>::epsilon();
    if (!(std::abs(norm3(nx) - 1.0) <= eps) || !(std::abs(norm3(ny) - 1.0) <= eps))
        return false;
    if (std::abs((ny[0] * nx[0] + ny[1] * nx[1]) + ny[2] * nx[2]) > .01)
        return false;
    out = p.to_camera_space(T);
    return true;
}

// The polygon step of Plane::update_boundary_polygon (plane_with_tracking.cpp:63-82) once the target frame is known, for
// cape_host_map_update and the twins of cape_map_union alike.  `poly` becomes the map polygon in the target frame -- Polygon::project
// returns the polygon itself if its frame is already the target (isApprox) -- and, if the step passes, its union with the detection
// (WorldPolygon::merge: merge_union of the detection projected into this frame; merge_union projects it, the reference's second
// projection onto the same frame returns it unchanged).  detection_world(out) yields the detection in world space, false where the
// reference throws.  A union beyond CAPE_MAP_MAX_RING / CAPE_MAP_MAX_HOLES keeps the OLD polygon (and its frame): `overflow`; `holed`
// says that the union had interior rings within an outer ring of at most CAPE_MAP_MAX_RING vertices, which `poly` no longer shows
// after an overflow.
struct PolygonStep
{
    bool ok = false, overflow = false, merged = false; // merged: what merge_union returned
    bool holed = false;
    Polygon::MergeInfo info;
};
template <class Detection>
PolygonStep polygon_step(const Polygon& mapPolygon, const vector3& xAxis, const vector3& yAxis, const vector3& center, Detection&& detection_world,
                         Polygon& poly)
{
    PolygonStep step;
    poly = mapPolygon;
    if (!(is_approx3(poly.get_center(), center) && is_approx3(poly.get_x_axis(), xAxis) && is_approx3(poly.get_y_axis(), yAxis)))
        poly = poly.project(xAxis, yAxis, center);
    Polygon detWorld;
    step.ok = is_approx3(poly.get_center(), center) && detection_world(detWorld);
    if (!step.ok)
        return step;
    Polygon merged = poly;
    step.merged = merged.merge_union(detWorld, &step.info);
    step.holed = merged.boundary().size() <= CAPE_MAP_MAX_RING && !merged.interior_rings().empty();
    bool fits = merged.boundary().size() <= CAPE_MAP_MAX_RING && merged.interior_rings().size() <= CAPE_MAP_MAX_HOLES;
    for (const auto& h : merged.interior_rings())
        fits = fits && h.size() <= CAPE_MAP_MAX_RING;
    if (fits)
        poly = merged;
    else
    {
        poly = mapPolygon;
        step.overflow = true;
    }
    return step;
}

// A pair's row of cape_map_union from the step's outcome (the map polygon had no hole; both operands within
// CAPE_MAP_UNION_MAX_RING): a union with a hole -- however many, and however long: the device does not count them -- or an
// outer ring beyond the map's limit is the host's; a served ring goes to `slab` at `used` if it fits the `capacity` pairs.
void put_union_row(cape_plane_union& row, const Polygon& poly, const PolygonStep& step, uint32_t& used, uint32_t capacity, double* slab)
{
    if (step.holed)
        row.flags = CAPE_UNION_HOST_NEW_HOLE;
    else if (step.overflow)
        row.flags = CAPE_UNION_HOST_CAPACITY;
    else if (poly.boundary().size() > capacity - used)
        row.flags = CAPE_UNION_HOST_CAPACITY;
    else
    {
        row.flags = CAPE_UNION_SERVED | (step.merged ? 0u : (uint32_t)CAPE_UNION_UNCHANGED) | (step.info.disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u);
        put3(row.x_axis, poly.get_x_axis());
        put3(row.y_axis, poly.get_y_axis());
        put3(row.center, poly.get_center());
        row.area = poly.get_area();
        row.vertex_offset = used;
        row.vertex_count = (uint32_t)poly.boundary().size();
        for (const vector2& p : poly.boundary())
        {
            slab[2 * (size_t)used] = p[0];
            slab[2 * (size_t)used + 1] = p[1];
            ++used;
        }
    }
}

// A pair's rows of cape_map_union_holes from the step's outcome (every ring of the map plane within CAPE_MAP_UNION_MAX_RING, at most
// CAPE_MAP_MAX_HOLES of them): a partly covered hole first, then the capacities the device has -- the interior rings before simplify,
// polygon_step's overflow, the slab, which takes the whole polygon or nothing.
// `cutMode` (cape_map_union_cut): a partly covered hole is no refusal -- the host class has computed its pieces -- and a served row
// says that merge_union's `cut` branch ran (CAPE_UNION_HOLE_PIECES).
void put_union_holes_rows(cape_plane_union& row, cape_plane_union_rings& rings, const Polygon& poly, const PolygonStep& step, uint32_t& used,
                          uint32_t capacity, double* slab, bool cutMode = false)
{
    size_t holeVertices = 0, total = poly.boundary().size();
    for (const auto& h : poly.interior_rings())
        holeVertices += h.size();
    total += holeVertices;
    if (step.merged)
        holeVertices = step.info.holeVertices; // (before simplify)
    if (step.info.holeCut && !cutMode)
        row.flags = CAPE_UNION_HOST_HOLE_CUT;
    else if (step.overflow || holeVertices > CAPE_MAP_UNION_HOLE_VERTICES || total > capacity - used)
        row.flags = CAPE_UNION_HOST_CAPACITY;
    else
    {
        const auto& holes = poly.interior_rings();
        row.flags = CAPE_UNION_SERVED | (step.merged ? 0u : (uint32_t)CAPE_UNION_UNCHANGED) | (step.info.disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u) |
                    (holes.empty() ? 0u : (uint32_t)CAPE_UNION_HOLES) | (step.info.holeCut ? (uint32_t)CAPE_UNION_HOLE_PIECES : 0u);
        put3(row.x_axis, poly.get_x_axis());
        put3(row.y_axis, poly.get_y_axis());
        put3(row.center, poly.get_center());
        row.area = poly.get_area();
        row.vertex_offset = used;
        row.vertex_count = (uint32_t)poly.boundary().size();
        rings.ring_count = 1 + (uint32_t)holes.size();
        rings.holes_new = step.info.holesNew;
        rings.holes_kept = step.info.holesKept;
        rings.holes_covered = step.info.holesCovered;
        for (size_t k = 0; k <= holes.size(); ++k)
        {
            const std::vector<vector2>& ring = k == 0 ? poly.boundary() : holes[k - 1];
            rings.vertex_count[k] = (uint32_t)ring.size();
            for (const vector2& p : ring)
            {
                slab[2 * (size_t)used] = p[0];
                slab[2 * (size_t)used + 1] = p[1];
                ++used;
            }
        }
    }
}

// what the device refuses before any geometry: a map plane of too many rings or with a ring it cannot hold, a detection too long
bool union_holes_operands_fit(const cape_host_map& map, const cape_map_plane& M, uint32_t detectionCount)
{
    if (M.ring_count > 1 + CAPE_MAP_MAX_HOLES || detectionCount > CAPE_MAP_UNION_MAX_RING)
        return false;
    for (uint32_t k = 0; k < M.ring_count; ++k)
        if (map.rings[M.ring_first + k].vertex_count > CAPE_MAP_UNION_MAX_RING)
            return false;
    return true;
}

} // namespace

extern "C" int cape_host_polygon(const double* points3, int n, const double* normal, const double* center, double* ring_out, int capacity,
                                 int* count_out, double* area_out, double* x_axis_out, double* y_axis_out, int* valid_out)
{
    try
    {
        std::vector<vector3> pts;
        pts.reserve(n);
        for (int i = 0; i < n; ++i)
            pts.emplace_back(points3[3 * i], points3[3 * i + 1], points3[3 * i + 2]);
        const Polygon poly(pts, vec3(normal), vec3(center));
        const auto& ring = poly.boundary();
        *count_out = static_cast<int>(ring.size());
        for (size_t i = 0; i < ring.size() && static_cast<int>(i) < capacity; ++i)
        {
            ring_out[2 * i] = ring[i][0];
            ring_out[2 * i + 1] = ring[i][1];
        }
        *area_out = poly.get_area();
        put3(x_axis_out, poly.get_x_axis());
        put3(y_axis_out, poly.get_y_axis());
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
    const Polygon a(ring_from(ring_a, na), vec3(x_a), vec3(y_a), vec3(c_a)), b(ring_from(ring_b, nb), vec3(x_b), vec3(y_b), vec3(c_b));
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
    const Polygon a(ring_from(ring_a, na), vec3(x_a), vec3(y_a), vec3(c_a)), b(ring_from(ring_b, nb), vec3(x_b), vec3(y_b), vec3(c_b));
    if (plane_in && plane_out)
        rgbd_slam::utils::plane_to_camera(plane_in, plane_in[3], world_to_camera, plane_out, plane_out + 3);
    return a.inter_area(b.to_camera_space(world_to_camera));
}

// The map matcher's host twin (cape_host_map.h).
extern "C" int cape_host_match_map(const cape_host_map* map, const cape_host_planes* detected, const double* world_to_camera,
                                   const uint32_t* skip, uint32_t flags, int32_t* match, int32_t* map_of, double* inter_area)
{
    static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double* T = world_to_camera ? world_to_camera : kIdentity;
    const double minCos = std::abs(std::cos(20.0 * M_PI / 180.0)); // parameters.hpp:92-93, shape_primitives.cpp:72-73
    const double maxDistance = 100.0;                              // parameters.hpp:94-95
    const double overlap = (flags & CAPE_MATCH_ADVANCED) ? static_cast<double>(0.4f) / 2 : static_cast<double>(0.4f);
    const int32_t n_planes = map->n_planes, n_det = detected->n;
    try
    {
        std::vector<Polygon> det;
        if (!kept_polygons(*detected, 0, det))
            return CAPE_ERR_INVALID_ARGUMENT;
        std::vector<double> detArea;
        for (int32_t i = 0; i < n_det; ++i)
            detArea.push_back(detected->areas ? detected->areas[i] : det[i].get_area());
        std::vector<char> matched(n_det, 0);
        std::fill_n(map_of, n_det, -1);
        std::fill_n(match, n_planes, -1);
        if (inter_area)
            std::fill_n(inter_area, (size_t)n_planes * n_det, -1.0);
        for (int32_t j = 0; j < n_planes; ++j)
        {
            const cape_map_plane& M = map->planes[j];
            const bool skipped = skip && ((skip[j >> 5] >> (j & 31)) & 1u); // is_moving() or not is_visible(worldToCamera): not visited
            Polygon mapPolygon;
            if (!map_polygon(*map, M, skipped ? nullptr : &mapPolygon))
                return CAPE_ERR_INVALID_ARGUMENT;
            if (skipped)
                continue;
            double pn[3], pd;
            rgbd_slam::utils::plane_to_camera(M.normal, M.d, T, pn, &pd);
            const Polygon projected = mapPolygon.to_camera_space(T);
            if (projected.get_area() <= 0.0)
                continue;
            int selected = -1;
            double greatest = 0.0;
            for (int32_t i = 0; i < n_det; ++i)
            {
                const double* dn = detected->planes + 4 * i;
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

// The twin of the consecutive-frame matchers (cape_host_map.h): the statements of cape_match_polygons_pose's three kernels in
// the order of map_primitive.cpp:91-161, frame f-1's kept planes as the map planes.
extern "C" int cape_host_match_planes(const cape_host_planes* prev, const cape_host_planes* cur, const double* prev_to_cur16, uint32_t flags,
                                      int32_t* match, double* inter_area)
{
    if (!prev || !cur || prev->n < 0 || cur->n < 0 || (prev->n > 0 && !match) || (flags & ~(uint32_t)(CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0)))
        return CAPE_ERR_INVALID_ARGUMENT;
    const double* T = prev_to_cur16;
    const double minCos = std::abs(std::cos(20.0 * M_PI / 180.0)); // parameters.hpp:92-93, shape_primitives.cpp:72-73
    const double maxDistance = 100.0;                              // parameters.hpp:94-95
    const double overlap = (flags & CAPE_MATCH_ADVANCED) ? static_cast<double>(0.4f) / 2 : static_cast<double>(0.4f);
    const int32_t n_prev = prev->n, n_cur = cur->n;
    try
    {
        std::vector<Polygon> map, det;
        if (!kept_polygons(*prev, 0, map) || !kept_polygons(*cur, 0, det))
            return CAPE_ERR_INVALID_ARGUMENT;
        std::vector<char> matched(n_cur, 0);
        std::fill_n(match, n_prev, -1);
        if (inter_area)
            std::fill_n(inter_area, (size_t)n_prev * n_cur, -1.0);
        for (int32_t j = 0; j < n_prev; ++j)
        {
            double pn[3] = {prev->planes[4 * j], prev->planes[4 * j + 1], prev->planes[4 * j + 2]}, pd = prev->planes[4 * j + 3];
            if (T)
                rgbd_slam::utils::plane_to_camera(prev->planes + 4 * j, prev->planes[4 * j + 3], T, pn, &pd);
            const Polygon projected = T ? map[j].to_camera_space(T) : map[j];
            const double projectedArea = prev->areas ? prev->areas[j] : map[j].get_area();
            int selected = -1;
            double greatest = 0.0;
            for (int32_t i = 0; i < n_cur; ++i)
            {
                const double* dn = cur->planes + 4 * i;
                const double cosAngle = (dn[0] * pn[0] + dn[1] * pn[1]) + dn[2] * pn[2];
                if (!(std::abs(dn[3] - pd) < maxDistance) || !(std::abs(cosAngle) > minCos))
                    continue;
                const double ia = det[i].inter_area(projected);
                if (inter_area)
                    inter_area[(size_t)j * n_cur + i] = ia;
                if (matched[i] || !(projectedArea > 0.0))
                    continue;
                if (ia > greatest && ia / (cur->areas ? cur->areas[i] : det[i].get_area()) >= overlap)
                {
                    selected = i;
                    greatest = ia;
                }
            }
            if (selected < 0 || (selected == 0 && !(flags & CAPE_MATCH_ALLOW_INDEX0))) // map_primitive.cpp:146
                continue;
            match[j] = selected;
            matched[selected] = 1;
        }
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}

// The visibility twin (cape_host_map.h).
extern "C" int cape_host_map_visibility(const cape_host_map* map, const double* world_to_camera, int32_t width, int32_t height, double fx, double fy,
                                        double cx, double cy, const uint32_t* moving, uint32_t* skip_out)
{
    static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!map || map->n_planes < 0 || width < 3 || height < 3 || (map->n_planes > 0 && (!skip_out || !map->planes)))
        return CAPE_ERR_INVALID_ARGUMENT;
    const double* T = world_to_camera ? world_to_camera : kIdentity;
    const int32_t n_planes = map->n_planes;
    try
    {
        std::vector<uint32_t> words((size_t)(n_planes + 31) / 32, 0u);
        for (int32_t j = 0; j < n_planes; ++j)
        {
            const bool isMoving = moving && ((moving[j >> 5] >> (j & 31)) & 1u);
            Polygon mapPolygon;
            if (!map_polygon(*map, map->planes[j], isMoving ? nullptr : &mapPolygon))
                return CAPE_ERR_INVALID_ARGUMENT;
            if (isMoving || !mapPolygon.to_camera_space(T).is_visible_in_screen_space(width, height, fx, fy, cx, cy))
                words[j >> 5] |= 1u << (j & 31);
        }
        std::copy(words.begin(), words.end(), skip_out);
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}

// One frame of a packed shard as the kept planes of the two calls around it (cape_host_map.h): the proof that what
// CAPE_GATHER_POLYGONS ships is enough to track planes on a rank that never saw the frame.
extern "C" int cape_host_shard_frame(const void* shard, uint64_t shard_bytes, const cape_gather_layout* layout,
                                     const cape_gather_polygon_layout* polygon_layout, int32_t frame, cape_host_planes* detected_out)
{
    if (!shard || !layout || !polygon_layout || !detected_out || frame < 0 || detected_out->capacity < 0 || detected_out->vertices_capacity < 0)
        return CAPE_ERR_INVALID_ARGUMENT;
    const cape_gather_layout& L = *layout;
    const cape_gather_polygon_layout& PL = *polygon_layout;
    const auto section_fits = [&](uint64_t offset, uint64_t count, uint64_t size) { return offset <= shard_bytes && count * size <= shard_bytes - offset; };
    if (shard_bytes != L.bytes_per_rank || PL.polygons_offset == 0 || L.frames_capacity < 0 || L.planes_capacity < 0 || PL.vertices_capacity < 0 ||
        PL.polygons_capacity != L.planes_capacity || !section_fits(0, 1, sizeof(cape_packed_header)) ||
        !section_fits(L.frames_offset, (uint64_t)L.frames_capacity, sizeof(cape_packed_frame)) ||
        !section_fits(L.planes_offset, (uint64_t)L.planes_capacity, sizeof(cape_packed_plane)) ||
        !section_fits(PL.polygons_offset, (uint64_t)PL.polygons_capacity, sizeof(cape_polygon)) ||
        !section_fits(PL.vertices_offset, (uint64_t)PL.vertices_capacity, 2 * sizeof(double)))
        return CAPE_ERR_INVALID_ARGUMENT;
    const unsigned char* base = static_cast<const unsigned char*>(shard);
    cape_packed_header hd;
    std::memcpy(&hd, base, sizeof(hd));
    if (hd.magic != CAPE_PACKED_MAGIC || !(hd.flags & CAPE_GATHER_POLYGONS) || frame >= hd.n_frames || hd.n_frames > L.frames_capacity ||
        (hd.overflow & (CAPE_PACKED_PLANES_DROPPED | CAPE_PACKED_VERTICES_DROPPED)))
        return CAPE_ERR_INVALID_ARGUMENT;
    cape_packed_frame fr;
    std::memcpy(&fr, base + L.frames_offset + (size_t)frame * sizeof(fr), sizeof(fr));
    if (fr.plane_offset < 0 || fr.n_planes < 0 || (int64_t)fr.plane_offset + fr.n_planes > L.planes_capacity)
        return CAPE_ERR_INVALID_ARGUMENT;
    int32_t n = 0;
    int64_t nv = 0;
    bool fits = true;
    try
    {
        for (int32_t k = fr.plane_offset; k < fr.plane_offset + fr.n_planes; ++k)
        {
            cape_polygon g;
            std::memcpy(&g, base + PL.polygons_offset + (size_t)k * sizeof(g), sizeof(g));
            if (!(g.flags & CAPE_POLY_VALID) || g.vertex_count < 3)
                continue; // Primitive_Detection drops the plane
            if ((uint64_t)g.vertex_offset + g.vertex_count > (uint64_t)PL.vertices_capacity)
                return CAPE_ERR_INVALID_ARGUMENT;
            fits = fits && n < detected_out->capacity && nv + g.vertex_count <= detected_out->vertices_capacity;
            if (fits)
            {
                cape_packed_plane pl;
                std::memcpy(&pl, base + L.planes_offset + (size_t)k * sizeof(pl), sizeof(pl));
                std::vector<double> xy(2 * (size_t)g.vertex_count);
                std::memcpy(xy.data(), base + PL.vertices_offset + (size_t)g.vertex_offset * 2 * sizeof(double), xy.size() * sizeof(double));
                const Polygon polygon(ring_from(xy.data(), g.vertex_count), vec3(g.x_axis), vec3(g.y_axis), vec3(g.center));
                if (polygon.boundary().size() != g.vertex_count)
                    return CAPE_ERR_INVALID_ARGUMENT; // (the constructor keeps an open ring as it is)
                put_kept_plane(*detected_out, n, nv, pl, g, polygon);
            }
            ++n;
            nv += g.vertex_count;
        }
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
    detected_out->n = n;
    detected_out->n_vertices = nv;
    return fits ? 0 : CAPE_ERR_CAPACITY;
}

// The host map update (cape_host_map.h).
extern "C" int cape_host_map_update(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected,
                                    const double* camera_to_world, const double* pose_covariance, uint32_t flags, uint64_t* next_id,
                                    cape_host_map* map_out, int32_t* used_out)
{
    namespace mt = rgbd_slam::map_tracking;
    if (!map || !detected || !map_out || map->n_planes < 0 || detected->n < 0 || detected->n > CAPE_MAX_PLANES || !camera_to_world ||
        !pose_covariance || !next_id || (map->n_planes > 0 && (!map->planes || !map->tracks || !match)) || (flags & ~(uint32_t)CAPE_MAP_ADD_STAGED))
        return CAPE_ERR_INVALID_ARGUMENT;
    const int32_t n_planes = map->n_planes, n_det = detected->n;
    const double *det_planes = detected->planes, *det_cov = detected->cov;
    const double* T = camera_to_world;
    if (!mt::is_covariance_valid(pose_covariance, 3))
        return CAPE_ERR_INVALID_ARGUMENT; // update_map: "The given pose covariance is invalid, map wont be update"
    try
    {
        std::vector<Polygon> det;
        if (!kept_polygons(*detected, 3, det))
            return CAPE_ERR_INVALID_ARGUMENT;
        std::vector<char> used(n_det, 0);
        std::vector<MapEntry> out;
        out.reserve(n_planes + n_det);
        for (int32_t j = 0; j < n_planes; ++j)
        {
            const cape_map_plane& M = map->planes[j];
            MapEntry e {M, map->tracks[j], Polygon()};
            if (match[j] < -1 || match[j] >= n_det || !map_polygon(*map, M, &e.polygon))
                return CAPE_ERR_INVALID_ARGUMENT;
            uint32_t result = 0;
            const bool staged = (e.track.flags & CAPE_MAP_TRACK_STAGED) != 0;
            const int32_t i = match[j];
            if (i >= 0)
            {
                result |= CAPE_MAP_RESULT_MATCHED;
                const double* dp = det_planes + 4 * i;
                double planeCov[16], worldCov[16], nw[3], dw;
                if (!mt::plane_covariance(dp, dp[3], det_cov + 9 * i, planeCov) ||
                    !mt::world_plane_covariance(dp, dp[3], T, planeCov, pose_covariance, worldCov))
                    result |= CAPE_MAP_RESULT_FAIL_DETECTION;
                else if (!mt::is_covariance_valid(e.track.covariance, 4))
                    result |= CAPE_MAP_RESULT_FAIL_STATE;
                else
                {
                    mt::plane_to_world(dp, dp[3], T, nw, &dw);
                    const double x[4] = {M.normal[0], M.normal[1], M.normal[2], M.d}, z[4] = {nw[0], nw[1], nw[2], dw};
                    double xn[4], Pn[16];
                    const mt::KalmanStatus st = mt::kalman_update(x, e.track.covariance, z, worldCov, xn, Pn);
                    if (st == mt::KALMAN_SINGULAR)
                        result |= CAPE_MAP_RESULT_FAIL_SINGULAR;
                    else if (st != mt::KALMAN_OK)
                        result |= CAPE_MAP_RESULT_FAIL_KALMAN;
                    else
                    {
                        // PlaneWorldCoordinates(vector4), its copy and the assignment each normalise the normal (plane_coordinates.hpp:19-32)
                        double n[3] = {xn[0], xn[1], xn[2]};
                        mt::normalize3(n);
                        mt::normalize3(n);
                        mt::normalize3(n);
                        std::memcpy(e.track.covariance, Pn, sizeof(Pn));
                        std::memcpy(e.plane.normal, n, sizeof(n));
                        e.plane.d = xn[3];
                        // Plane::update_boundary_polygon (plane_with_tracking.cpp:63-82)
                        const vector3 normal(n[0], n[1], n[2]), center(n[0] * -xn[3], n[1] * -xn[3], n[2] * -xn[3]);
                        bool ok = std::abs(mt::norm3(n) - 1.0) <= std::numeric_limits<double>::epsilon(); // Polygon::project's check
                        Polygon poly = e.polygon;
                        if (ok)
                        {
                            const auto axes = rgbd_slam::utils::get_plane_coordinate_system(normal);
                            const PolygonStep step = polygon_step(e.polygon, axes.first, axes.second, center,
                                                                  [&](Polygon& detWorld) { return to_world_space(det[i], T, detWorld); }, poly);
                            ok = step.ok;
                            if (ok)
                            {
                                if (step.overflow)
                                    result |= CAPE_MAP_RESULT_OVERFLOW;
                                result |= CAPE_MAP_RESULT_UPDATED;
                            }
                        }
                        if (!ok)
                            result |= CAPE_MAP_RESULT_FAIL_POLYGON;
                        e.polygon = poly;
                    }
                }
                if ((result & CAPE_MAP_RESULT_UPDATED) || staged)
                    used[i] = 1;
            }
            if (result & CAPE_MAP_RESULT_UPDATED)
            {
                e.track.failed_tracking = 0;
                ++e.track.successive_matched;
            }
            else
            {
                ++e.track.failed_tracking;
                e.track.successive_matched -= 1;
            }
            if (staged && e.track.successive_matched >= 4)
                result |= CAPE_MAP_RESULT_PROMOTE;
            else if (staged && e.track.failed_tracking >= 2)
                result |= CAPE_MAP_RESULT_DROP;
            else if (!staged && e.track.failed_tracking >= 10)
                result |= CAPE_MAP_RESULT_LOST;
            e.track.result = result;
            out.push_back(std::move(e));
        }
        uint64_t id = *next_id;
        if (flags & CAPE_MAP_ADD_STAGED)
            for (int32_t i = 0; i < n_det; ++i)
            {
                if (used[i])
                    continue;
                const double* dp = det_planes + 4 * i;
                MapEntry e {};
                double planeCov[16];
                if (!mt::plane_covariance(dp, dp[3], det_cov + 9 * i, planeCov) ||
                    !mt::world_plane_covariance(dp, dp[3], T, planeCov, pose_covariance, e.track.covariance))
                    continue;
                mt::plane_to_world(dp, dp[3], T, e.plane.normal, &e.plane.d);
                mt::normalize3(e.plane.normal); // the assignment to _parametrization
                if (!to_world_space(det[i], T, e.polygon) || !(std::abs(mt::norm3(e.plane.normal) - 1.0) <= std::numeric_limits<double>::epsilon()) ||
                    e.polygon.boundary().size() > CAPE_MAP_MAX_RING)
                    continue;
                e.track.flags = CAPE_MAP_TRACK_STAGED;
                e.track.result = CAPE_MAP_RESULT_APPENDED;
                e.track.id = id++;
                out.push_back(std::move(e));
            }
        if (!put_map(out, *map_out))
            return CAPE_ERR_CAPACITY;
        if (used_out)
            std::copy(used.begin(), used.end(), used_out);
        *next_id = id;
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}

// The twin of cape_map_kalman (cape_host_map.h): the statements of cape_host_map_update above that concern a map plane's state, the
// detection's measurement given as a row of cape_map_measure.
extern "C" int cape_host_map_kalman(const cape_host_map* map, const int32_t* match, const cape_plane_measurement* measurements, int32_t n_cur,
                                    cape_frame_map_kalman* frame_out, cape_plane_fusion* rows_out, cape_map_track_result* tracks_out)
{
    namespace mt = rgbd_slam::map_tracking;
    if (!map || map->n_planes < 0 || n_cur < 0 || n_cur > CAPE_MATCH_MAP_WIDE_MAX_PLANES || (n_cur > 0 && !measurements) ||
        (map->n_planes > 0 && (!map->planes || !map->tracks || !match)))
        return CAPE_ERR_INVALID_ARGUMENT;
    const int32_t n_planes = map->n_planes;
    for (int32_t j = 0; j < n_planes; ++j)
        if (match[j] < -1 || match[j] >= n_cur)
            return CAPE_ERR_INVALID_ARGUMENT;
    std::vector<cape_plane_fusion> rows((size_t)n_cur, cape_plane_fusion {});
    for (auto& row : rows)
        row.map_plane = -1;
    const uint32_t noDetection = CAPE_MEASURE_FAIL_PLANE_COV | CAPE_MEASURE_FAIL_WORLD_COV | CAPE_MEASURE_BAD_POSE_COV;
    bool badPose = false;
    for (int32_t i = 0; i < n_cur; ++i)
        badPose = badPose || (measurements[i].flags & CAPE_MEASURE_BAD_POSE_COV) != 0;
    int32_t nUpdated = 0;
    for (int32_t j = 0; j < n_planes; ++j)
    {
        const cape_map_plane& M = map->planes[j];
        cape_map_track track = map->tracks[j];
        uint32_t result = 0;
        const bool staged = (track.flags & CAPE_MAP_TRACK_STAGED) != 0;
        const int32_t i = match[j];
        if (i >= 0)
        {
            const cape_plane_measurement& m = measurements[i];
            cape_plane_fusion& row = rows[i];
            row.map_plane = j;
            result |= CAPE_MAP_RESULT_MATCHED;
            if (!(m.flags & CAPE_MEASURE_KEPT) || (m.flags & noDetection))
                result |= CAPE_MAP_RESULT_FAIL_DETECTION;
            else if (!mt::is_covariance_valid(track.covariance, 4))
                result |= CAPE_MAP_RESULT_FAIL_STATE;
            else
            {
                const double x[4] = {M.normal[0], M.normal[1], M.normal[2], M.d}, z[4] = {m.normal[0], m.normal[1], m.normal[2], m.d};
                double xn[4], Pn[16];
                const mt::KalmanStatus st = mt::kalman_update(x, track.covariance, z, m.covariance, xn, Pn);
                if (st == mt::KALMAN_SINGULAR)
                    result |= CAPE_MAP_RESULT_FAIL_SINGULAR;
                else if (st != mt::KALMAN_OK)
                    result |= CAPE_MAP_RESULT_FAIL_KALMAN;
                else
                {
                    double n[3] = {xn[0], xn[1], xn[2]};
                    mt::normalize3(n);
                    mt::normalize3(n);
                    mt::normalize3(n);
                    std::memcpy(row.normal, n, sizeof(n));
                    row.d = xn[3];
                    std::memcpy(row.covariance, Pn, sizeof(Pn));
                    row.flags |= CAPE_FUSION_STATE;
                    bool ok = std::abs(mt::norm3(n) - 1.0) <= std::numeric_limits<double>::epsilon(); // Polygon::project's check
                    if (ok)
                    {
                        try
                        {
                            const auto axes = rgbd_slam::utils::get_plane_coordinate_system(vector3(n[0], n[1], n[2]));
                            for (int k = 0; k < 3; ++k)
                            {
                                row.x_axis[k] = axes.first[k];
                                row.y_axis[k] = axes.second[k];
                                row.center[k] = n[k] * -xn[3];
                            }
                            row.flags |= CAPE_FUSION_FRAME;
                        }
                        catch (const std::invalid_argument&)
                        {
                            ok = false; // (its own 1e-9 norm check)
                        }
                    }
                    ok = ok && !(m.flags & CAPE_MEASURE_FAIL_POLYGON);
                    result |= ok ? CAPE_MAP_RESULT_UPDATED : CAPE_MAP_RESULT_FAIL_POLYGON;
                }
            }
            if ((result & CAPE_MAP_RESULT_UPDATED) || staged)
                row.flags |= CAPE_FUSION_USED;
        }
        if (result & CAPE_MAP_RESULT_UPDATED)
        {
            track.failed_tracking = 0;
            track.successive_matched = (int32_t)((uint32_t)track.successive_matched + 1u);
            ++nUpdated;
        }
        else
        {
            ++track.failed_tracking;
            track.successive_matched = (int32_t)((uint32_t)track.successive_matched - 1u);
        }
        if (staged && track.successive_matched >= 4)
            result |= CAPE_MAP_RESULT_PROMOTE;
        else if (staged && track.failed_tracking >= 2)
            result |= CAPE_MAP_RESULT_DROP;
        else if (!staged && track.failed_tracking >= 10)
            result |= CAPE_MAP_RESULT_LOST;
        if (tracks_out)
            tracks_out[j] = cape_map_track_result {result, track.successive_matched, track.failed_tracking, i};
    }
    if (rows_out)
        std::copy(rows.begin(), rows.end(), rows_out);
    if (frame_out)
        *frame_out = cape_frame_map_kalman {n_planes, n_cur, badPose ? (uint32_t)CAPE_KALMAN_BAD_POSE_COV : 0u, nUpdated};
    return 0;
}

// The twins of cape_map_union and cape_map_union_holes (cape_host_map.h): the polygon step above, per pair of one frame, through the
// host class itself.  rings_out NULL: the first one's rules, otherwise the second one's.
namespace {
int host_map_union(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion, const cape_plane_measurement* measurements,
                   const double* world_vertices, int32_t n_cur, cape_plane_union* rows_out, cape_plane_union_rings* rings_out, double* vertices_out,
                   bool cutMode = false)
{
    const bool holesMode = rings_out != nullptr;
    if (!map || map->n_planes < 0 || n_cur < 0 || n_cur > CAPE_MATCH_MAP_WIDE_MAX_PLANES || !rows_out || !vertices_out ||
        (n_cur > 0 && (!fusion || !measurements || !world_vertices)) || (map->n_planes > 0 && (!map->planes || !map->rings || !map->vertices)))
        return CAPE_ERR_INVALID_ARGUMENT;
    const int32_t n_planes = map->n_planes;
    try
    {
        std::vector<cape_plane_union> rows(CAPE_MATCH_MAP_WIDE_MAX_PLANES, cape_plane_union {});
        std::vector<cape_plane_union_rings> ringRows(CAPE_MATCH_MAP_WIDE_MAX_PLANES, cape_plane_union_rings {});
        std::vector<double> slab;
        slab.resize(2 * (size_t)CAPE_MAP_UNION_FRAME_VERTICES);
        uint32_t used = 0;
        size_t ringAt = 0;
        for (int32_t i = 0; i < n_cur; ++i)
        {
            const cape_plane_fusion& F = fusion[i];
            const cape_plane_measurement& m = measurements[i];
            const size_t ringFirst = ringAt;
            ringAt += m.vertex_count;
            cape_plane_union& row = rows[i];
            row.map_plane = -1;
            const int32_t j = F.map_plane;
            if (j < 0 || j >= n_planes || !(F.flags & CAPE_FUSION_FRAME) || !(m.flags & CAPE_MEASURE_KEPT) || (m.flags & CAPE_MEASURE_FAIL_POLYGON) ||
                (match && match[j] != i))
                continue;
            row.map_plane = j;
            const cape_map_plane& M = map->planes[j];
            if (!map_polygon(*map, M, nullptr))
                return CAPE_ERR_INVALID_ARGUMENT;
            if (!holesMode && M.ring_count > 1)
            {
                row.flags = CAPE_UNION_HOST_MAP_HOLES;
                continue;
            }
            if (!union_holes_operands_fit(*map, M, m.vertex_count))
            {
                row.flags = CAPE_UNION_HOST_CAPACITY;
                continue;
            }
            Polygon mapPolygon, poly;
            map_polygon(*map, M, &mapPolygon);
            const PolygonStep step = polygon_step(
                mapPolygon, vec3(F.x_axis), vec3(F.y_axis), vec3(F.center),
                [&](Polygon& detWorld) {
                    detWorld = Polygon(ring_from(world_vertices + 2 * ringFirst, m.vertex_count), {}, vec3(m.x_axis), vec3(m.y_axis), vec3(m.center));
                    return true;
                },
                poly);
            if (!step.ok) // (the centre check after a projection: not reached, the projected polygon's centre IS the target)
                continue;
            if (holesMode)
                put_union_holes_rows(row, ringRows[i], poly, step, used, CAPE_MAP_UNION_FRAME_VERTICES, slab.data(), cutMode);
            else
                put_union_row(row, poly, step, used, CAPE_MAP_UNION_FRAME_VERTICES, slab.data());
        }
        std::copy(rows.begin(), rows.end(), rows_out);
        if (holesMode)
            std::copy(ringRows.begin(), ringRows.end(), rings_out);
        std::copy(slab.begin(), slab.begin() + 2 * (size_t)used, vertices_out);
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}

// one pair given by its rings and frames: ring a with its interior rings (holesMode) against ring b
int host_pair_union(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b, const double* frames27,
                    cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out, bool cutMode = false)
{
    static const double kCanonical[27] = {1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0};
    const bool holesMode = rings_out != nullptr;
    const double* F = frames27 ? frames27 : kCanonical;
    try
    {
        cape_plane_union row {};
        cape_plane_union_rings ringRow {};
        bool fits = n_b <= CAPE_MAP_UNION_MAX_RING;
        for (int32_t k = 0; k < n_rings_a; ++k)
            fits = fits && counts_a[k] <= CAPE_MAP_UNION_MAX_RING;
        if (!fits)
            row.flags = CAPE_UNION_HOST_CAPACITY;
        else
        {
            std::vector<std::vector<vector2>> holes;
            size_t at = (size_t)counts_a[0];
            for (int32_t k = 1; k < n_rings_a; ++k)
            {
                holes.push_back(ring_from(rings_a + 2 * at, (size_t)counts_a[k]));
                at += (size_t)counts_a[k];
            }
            const Polygon a(ring_from(rings_a, (size_t)counts_a[0]), holes, vec3(F), vec3(F + 3), vec3(F + 6));
            const Polygon b(ring_from(ring_b, n_b), {}, vec3(F + 9), vec3(F + 12), vec3(F + 15));
            Polygon poly;
            const PolygonStep step = polygon_step(
                a, vec3(F + 18), vec3(F + 21), vec3(F + 24),
                [&](Polygon& detWorld) {
                    detWorld = b;
                    return true;
                },
                poly);
            uint32_t used = 0;
            if (step.ok && holesMode)
                put_union_holes_rows(row, ringRow, poly, step, used, CAPE_MAP_UNION_FRAME_VERTICES, vertices_out, cutMode);
            else if (step.ok)
                put_union_row(row, poly, step, used, CAPE_MAP_MAX_RING, vertices_out);
        }
        *row_out = row;
        if (holesMode)
            *rings_out = ringRow;
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}
} // namespace

extern "C" int cape_host_map_union(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion,
                                   const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur,
                                   cape_plane_union* rows_out, double* vertices_out)
{
    return host_map_union(map, match, fusion, measurements, world_vertices, n_cur, rows_out, nullptr, vertices_out);
}

extern "C" int cape_host_map_union_holes(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion,
                                         const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur,
                                         cape_plane_union* rows_out, cape_plane_union_rings* rings_out, double* vertices_out)
{
    if (!rings_out)
        return CAPE_ERR_INVALID_ARGUMENT;
    return host_map_union(map, match, fusion, measurements, world_vertices, n_cur, rows_out, rings_out, vertices_out);
}

extern "C" int cape_host_map_union_cut(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion,
                                       const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur,
                                       cape_plane_union* rows_out, cape_plane_union_rings* rings_out, double* vertices_out)
{
    if (!rings_out)
        return CAPE_ERR_INVALID_ARGUMENT;
    return host_map_union(map, match, fusion, measurements, world_vertices, n_cur, rows_out, rings_out, vertices_out, true);
}

// The twin of cape_map_commit (cape_host_map.h): the decisions are the plan of csrc/cape_map_commit.h, one plane after the other; the
// planes it names are then built like cape_host_map_update builds them and laid out by put_map.
extern "C" int cape_host_map_commit(const cape_host_map* map, int32_t frame, const cape_frame_map_kalman* frame_header,
                                    const cape_map_track_result* track_results, const cape_plane_fusion* fusion,
                                    const cape_plane_measurement* measurements, const double* world_vertices, const cape_plane_union* union_rows,
                                    const cape_plane_union_rings* rings, const double* slab, uint32_t flags, uint64_t* next_id,
                                    cape_host_map* map_out, cape_map_commit_result* result_out)
{
    if (!map || !frame_header || !next_id || !map_out || !result_out || frame < 0 || map->n_planes < 0 || map->n_rings < 0 || map->n_vertices < 0 ||
        (flags & ~(uint32_t)CAPE_COMMIT_ADD_STAGED) ||
        (map->n_planes > 0 && (!map->planes || !map->tracks || !map->rings || !map->vertices || !track_results)))
        return CAPE_ERR_INVALID_ARGUMENT;
    const int32_t n_planes = map->n_planes, n_cur = cape::commit_kept_planes(*frame_header);
    if (n_cur > 0 && (!fusion || !measurements || !world_vertices || !union_rows || !slab))
        return CAPE_ERR_INVALID_ARGUMENT;
    try
    {
        std::vector<cape::CommitPlanRow> plan((size_t)n_planes + cape::kCommitMaxAppended);
        const uint64_t unbounded = ~(uint64_t)0; // (the twin writes the caller's arrays: put_map checks them)
        const cape_map_commit_result result =
            cape::commit_plan_serial(map->planes, n_planes, map->rings, map->n_rings, map->n_vertices, frame, *frame_header, track_results, fusion,
                                     measurements, union_rows, rings, flags, *next_id, unbounded, unbounded, unbounded, plan.data());
        *result_out = result;
        if (!(result.flags & CAPE_COMMIT_DONE))
            return 0; // refused: map_out and next_id stay as they were
        std::vector<MapEntry> out;
        out.reserve((size_t)result.n_planes);
        for (int32_t b = 0; b < result.n_planes; ++b)
        {
            const cape::CommitPlanRow& row = plan[b];
            MapEntry e {};
            if (row.source == cape::kCommitFromMeasure)
            {
                const cape_plane_measurement& m = measurements[row.index];
                std::memcpy(e.plane.normal, m.staged_normal, sizeof(m.staged_normal));
                e.plane.d = m.d;
                std::memcpy(e.track.covariance, m.covariance, sizeof(m.covariance));
                e.polygon = Polygon(ring_from(world_vertices + 2 * (size_t)row.srcVertex, m.vertex_count), {}, vec3(m.x_axis), vec3(m.y_axis),
                                    vec3(m.center));
                e.track.flags = CAPE_MAP_TRACK_STAGED;
                e.track.result = CAPE_MAP_RESULT_APPENDED;
                e.track.id = *next_id + (uint64_t)(b - n_planes);
                out.push_back(std::move(e));
                continue;
            }
            const int32_t j = row.source == cape::kCommitFromUnion ? union_rows[row.index].map_plane : (int32_t)row.index;
            e.plane = map->planes[j];
            e.track = map->tracks[j];
            if (row.source == cape::kCommitFromUnion)
            {
                const cape_plane_fusion& F = fusion[row.index];
                const cape_plane_union& U = union_rows[row.index];
                std::memcpy(e.plane.normal, F.normal, sizeof(F.normal));
                e.plane.d = F.d;
                std::memcpy(e.track.covariance, F.covariance, sizeof(F.covariance));
                std::vector<std::vector<vector2>> polygonRings;
                size_t at = (size_t)row.srcVertex;
                for (uint32_t k = 0; k < row.ringCount; ++k)
                {
                    const uint32_t count = rings ? rings[row.index].vertex_count[k] : U.vertex_count;
                    polygonRings.push_back(ring_from(slab + 2 * at, count));
                    at += count;
                }
                e.polygon = Polygon(polygonRings[0], {polygonRings.begin() + 1, polygonRings.end()}, vec3(U.x_axis), vec3(U.y_axis), vec3(U.center));
            }
            else if (!map_polygon(*map, e.plane, &e.polygon))
                return CAPE_ERR_INVALID_ARGUMENT;
            e.track.successive_matched = track_results[j].successive_matched;
            e.track.failed_tracking = track_results[j].failed_tracking;
            e.track.result = track_results[j].result;
            out.push_back(std::move(e));
        }
        if (!put_map(out, *map_out))
            return CAPE_ERR_CAPACITY;
        *next_id = result.next_id;
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}

// The twin of cape_map_maintain (cape_host_map.h): the decisions are the plan of csrc/cape_map_maintain.h, one plane after the other,
// with the promote candidates' check made here by the host algebra; the planes it keeps or retires go through the host class and
// put_map.
extern "C" int cape_host_map_maintain(const cape_host_map* map, cape_host_map* map_out, cape_host_map* retired_out, cape_map_maintain_result* result_out)
{
    if (!map || !map_out || !retired_out || !result_out || map->n_planes < 0 || map->n_rings < 0 || map->n_vertices < 0 ||
        retired_out->n_planes < 0 || retired_out->n_rings < 0 || retired_out->n_vertices < 0 ||
        (map->n_planes > 0 && (!map->planes || !map->tracks || !map->rings || !map->vertices)))
        return CAPE_ERR_INVALID_ARGUMENT;
    namespace mt = rgbd_slam::map_tracking;
    const int32_t n_planes = map->n_planes;
    try
    {
        std::vector<uint8_t> promotable((size_t)n_planes, 0);
        for (int32_t j = 0; j < n_planes; ++j)
        {
            const cape_map_track& T = map->tracks[j];
            if (cape::maintain_promote_candidate(T.flags, T.successive_matched))
                promotable[j] = mt::is_covariance_valid(T.covariance, 4) &&
                                std::abs(mt::norm3(map->planes[j].normal) - 1.0) <= std::numeric_limits<double>::epsilon();
        }
        std::vector<cape::MaintainPlanRow> plan((size_t)n_planes);
        const uint64_t unbounded = ~(uint64_t)0; // (the twin writes the caller's arrays: put_map checks them)
        const cape::MaintainLog log {cape::MaintainCursor {retired_out->n_planes, retired_out->n_rings, retired_out->n_vertices}, unbounded, unbounded,
                                     unbounded};
        const cape_map_maintain_result result = cape::maintain_plan_serial(map->planes, n_planes, map->rings, map->n_rings, map->n_vertices, map->tracks,
                                                                           promotable.data(), unbounded, unbounded, unbounded, log, plan.data());
        *result_out = result;
        if (!(result.flags & CAPE_MAINTAIN_DONE))
            return 0; // NOTHING or refused: map_out and retired_out stay as they were
        std::vector<MapEntry> out((size_t)result.n_planes), lost;
        for (int32_t j = 0; j < n_planes; ++j)
        {
            const cape::MaintainPlanRow& row = plan[j];
            if (row.dest == cape::kMaintainToNone)
                continue;
            MapEntry e {};
            e.plane = map->planes[j];
            e.track = map->tracks[j];
            if (!map_polygon(*map, e.plane, &e.polygon))
                return CAPE_ERR_INVALID_ARGUMENT;
            if (row.edit == cape::kMaintainEditPromote)
            {
                e.track.flags &= ~(uint32_t)CAPE_MAP_TRACK_STAGED;
                e.track.failed_tracking = 0;
            }
            if (row.dest == cape::kMaintainToLog)
                lost.push_back(std::move(e)); // (in list order: the log's planes count up with j)
            else
                out[row.plane] = std::move(e);
        }
        if (result.n_planes > map_out->planes_capacity || result.n_rings > map_out->rings_capacity || result.n_vertices > map_out->vertices_capacity ||
            result.n_retired > retired_out->planes_capacity || result.n_retired_rings > retired_out->rings_capacity ||
            result.n_retired_vertices > retired_out->vertices_capacity)
            return CAPE_ERR_CAPACITY;
        if (!put_map(out, *map_out) || (!lost.empty() && !put_map(lost, *retired_out, true)))
            return CAPE_ERR_CAPACITY;
        return 0;
    }
    catch (const std::exception&)
    {
        return CAPE_ERR_INVALID_ARGUMENT;
    }
}

// The twins of cape_debug_ring_union, cape_debug_polygon_union and cape_debug_polygon_union_cut (cape_host_map.h): one pair given by
// its rings and three frames.
extern "C" int cape_host_ring_union(const double* ring_a, int32_t n_a, const double* ring_b, int32_t n_b, const double* frames27,
                                    cape_plane_union* row_out, double* vertices_out)
{
    if (!ring_a || !ring_b || !row_out || !vertices_out || n_a < 3 || n_b < 3 || n_a > 4096 || n_b > 4096)
        return CAPE_ERR_INVALID_ARGUMENT;
    return host_pair_union(ring_a, &n_a, 1, ring_b, n_b, frames27, row_out, nullptr, vertices_out);
}

// the argument checks of cape_host_polygon_union and cape_host_polygon_union_cut
static bool polygon_union_arguments_fit(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                                        const cape_plane_union* row_out, const cape_plane_union_rings* rings_out, const double* vertices_out)
{
    if (!rings_a || !counts_a || !ring_b || !row_out || !rings_out || !vertices_out || n_rings_a < 1 || n_rings_a > 1 + CAPE_MAP_MAX_HOLES || n_b < 3 ||
        n_b > 4096)
        return false;
    for (int32_t k = 0; k < n_rings_a; ++k)
        if (counts_a[k] < 3 || counts_a[k] > 4096)
            return false;
    return true;
}

extern "C" int cape_host_polygon_union(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                                       const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out)
{
    if (!polygon_union_arguments_fit(rings_a, counts_a, n_rings_a, ring_b, n_b, row_out, rings_out, vertices_out))
        return CAPE_ERR_INVALID_ARGUMENT;
    return host_pair_union(rings_a, counts_a, n_rings_a, ring_b, n_b, frames27, row_out, rings_out, vertices_out);
}

extern "C" int cape_host_polygon_union_cut(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                                           const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out,
                                           double* vertices_out)
{
    if (!polygon_union_arguments_fit(rings_a, counts_a, n_rings_a, ring_b, n_b, row_out, rings_out, vertices_out))
        return CAPE_ERR_INVALID_ARGUMENT;
    return host_pair_union(rings_a, counts_a, n_rings_a, ring_b, n_b, frames27, row_out, rings_out, vertices_out, true);
}

// Test hooks of the covariance and Kalman algebra (tests/test_map_update_host.py restates them in numpy).  Each returns 1 on
// success, 0 where the reference throws; cape_host_kalman_update returns the KalmanStatus.
extern "C" int cape_host_covariance_valid(const double* M, int n) { return (n == 3 || n == 4) && rgbd_slam::map_tracking::is_covariance_valid(M, n); }
extern "C" int cape_host_plane_covariance(const double* normal, double d, const double* cov9, double* out16)
{
    return rgbd_slam::map_tracking::plane_covariance(normal, d, cov9, out16);
}
extern "C" int cape_host_world_plane_covariance(const double* normal, double d, const double* camera_to_world, const double* plane_cov16,
                                                const double* pose_cov9, double* out16)
{
    return rgbd_slam::map_tracking::world_plane_covariance(normal, d, camera_to_world, plane_cov16, pose_cov9, out16);
}
extern "C" int cape_host_kalman_update(const double* x, const double* P, const double* z, const double* R, double* x_out, double* P_out)
{
    return rgbd_slam::map_tracking::kalman_update(x, P, z, R, x_out, P_out);
}
// get_plane_coordinate_system: out6 = x axis, y axis; 0 where it throws (the normal's norm is not 1 within 1e-9)
extern "C" int cape_host_plane_frame(const double* normal, double* out6)
{
    try
    {
        const auto axes = rgbd_slam::utils::get_plane_coordinate_system(vector3(normal[0], normal[1], normal[2]));
        for (int k = 0; k < 3; ++k)
        {
            out6[k] = axes.first[k];
            out6[3 + k] = axes.second[k];
        }
        return 1;
    }
    catch (const std::invalid_argument&)
    {
        return 0;
    }
}
// plane_to_world: out4 = (normal, d) of the plane in world coordinates, z of the Kalman step
extern "C" void cape_host_plane_to_world(const double* normal, double d, const double* camera_to_world, double* out4)
{
    rgbd_slam::map_tracking::plane_to_world(normal, d, camera_to_world, out4, out4 + 3);
}
