/* cape_host_map.h -- the host map update of libcape_primitives.so (host/polygon_capi.cpp): Feature_Map::update_map for one frame
 * on the host class, over a map in the layout of cape_map_upload (include/cape_hip.h).  Not part of libcape_hip's C ABI: no
 * function of libcape_hip takes these types. */
#ifndef CAPE_HOST_MAP_H
#define CAPE_HOST_MAP_H

#include "cape_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tracking state of one map plane, parallel to cape_map_plane: what Feature_Map::update_map (feature_map.hpp:367-384, :701-830)
 * reads and changes besides the plane and its polygon.  cape_host_map_update fuses one frame's matched planes into the map with it: MapPlane::update_with_match (map_primitive.cpp:204-251) per matched plane, the
 * counters of update_matched / update_unmatched (feature_map.hpp:112-129) for every plane, and optionally the StagedMapPlane
 * appends (map_primitive.cpp:262-285).  Promotion from staged to local, removal from staged and the loss of a local plane
 * reorder or delete entries of the ordered list: they are reported in `result` and left to the caller. */
typedef struct cape_map_track
{
    double covariance[16];      /* 4 x 4 covariance of (normal, d), row-major */
    int32_t successive_matched; /* _successivMatchedCount (may go negative) */
    uint32_t failed_tracking;   /* _failedTrackingCount */
    uint32_t flags;             /* CAPE_MAP_TRACK_* */
    uint32_t result;            /* CAPE_MAP_RESULT_* of the last update call (output) */
    uint64_t id;                /* the caller's identifier; appended planes get consecutive ids from the update's next_id */
} cape_map_track;
enum
{
    CAPE_MAP_TRACK_STAGED = 1u << 0, /* a staged plane (StagedMapPlane): a match counts the detection as used even if the update fails */
    CAPE_MAP_TRACK_MOVING = 1u << 1  /* is_moving(): informational here, the caller's skip bits of cape_match_map follow it */
};
enum
{
    CAPE_MAP_RESULT_MATCHED = 1u << 0,        /* a detected plane was matched to this map plane */
    CAPE_MAP_RESULT_UPDATED = 1u << 1,        /* update_with_match returned true */
    CAPE_MAP_RESULT_FAIL_DETECTION = 1u << 2, /* the detection's plane / world covariance is invalid: nothing changed */
    CAPE_MAP_RESULT_FAIL_STATE = 1u << 3,     /* the map plane's covariance is invalid (the reference exits): nothing changed */
    CAPE_MAP_RESULT_FAIL_SINGULAR = 1u << 4,  /* innovation determinant 0 within DBL_EPSILON, where the reference takes a
                                                 pseudo-inverse: nothing changed.  Not reached with valid covariances: the
                                                 detection's world covariance carries 0.01 on its diagonal, so the innovation's
                                                 eigenvalues are >= 0.01 */
    CAPE_MAP_RESULT_FAIL_KALMAN = 1u << 5,    /* the Kalman step produced an invalid covariance: nothing changed */
    CAPE_MAP_RESULT_FAIL_POLYGON = 1u << 6,   /* update_boundary_polygon failed: the plane and covariance ARE updated, the polygon
                                                 is the projected one or the old one.  Its isApprox centre check fails the update
                                                 like the reference; a Polygon::project or to_world_space check, which throws inside
                                                 the noexcept update_boundary_polygon there (std::terminate), fails it here too */
    CAPE_MAP_RESULT_OVERFLOW = 1u << 7,       /* the merged polygon exceeds CAPE_MAP_MAX_RING / CAPE_MAP_MAX_HOLES after simplify:
                                                 plane and covariance updated, the old polygon (and its frame) kept */
    CAPE_MAP_RESULT_PROMOTE = 1u << 8,        /* staged, should_add_to_local_map (successive_matched >= 4) */
    CAPE_MAP_RESULT_DROP = 1u << 9,           /* staged, not promoted, should_remove_from_staged (failed_tracking >= 2) */
    CAPE_MAP_RESULT_LOST = 1u << 10,          /* local, is_lost (failed_tracking >= planeUnmatchedCountToLoose = 10) */
    CAPE_MAP_RESULT_APPENDED = 1u << 11       /* a staged plane appended by this call */
};
enum
{
    CAPE_MAP_ADD_STAGED = 1u << 0 /* append every kept plane of the frame that no map plane used as a staged plane (not one whose
                                     StagedMapPlane constructor would throw, nor one whose ring exceeds CAPE_MAP_MAX_RING) */
};

int cape_host_map_update(const cape_map_plane* planes, int32_t n_planes, const cape_map_ring* rings, int32_t n_rings, const double* vertices,
                         int64_t n_vertices, const cape_map_track* tracks, const int32_t* match, int32_t n_det, const double* det_planes,
                         const double* det_cov, const double* det_frames, const double* det_vertices, const int32_t* det_counts,
                         const double* camera_to_world, const double* pose_covariance, uint32_t flags, uint64_t* next_id,
                         cape_map_plane* planes_out, int32_t planes_capacity, cape_map_ring* rings_out, int32_t rings_capacity,
                         double* vertices_out, int64_t vertices_capacity, cape_map_track* tracks_out, int32_t* n_planes_out,
                         int32_t* n_rings_out, int64_t* n_vertices_out, int32_t* used_out);

/* One frame of a packed shard -- the bytes cape_pack_primitives writes with CAPE_GATHER_POLYGONS, as they arrive from
 * cape_gather_primitives[_root] or any other transport -- as the detected planes cape_host_match_map and cape_host_map_update take: no
 * handle, no device.  `frame` counts from the shard's first frame.  The planes are those Primitive_Detection keeps (packed polygon with
 * CAPE_POLY_VALID and >= 3 vertices, primitive_detection.cpp:623-631) in order, i.e. the reference's plane_container; each goes
 * through the host class's Polygon(ring, xAxis, yAxis, center) constructor, which is where ring, axes and area come from.
 * Outputs (each may be NULL; `capacity` planes, `vertices_capacity` (x, y) pairs): det_planes n x (normal[3], d); det_cov n x 9, the
 * point-cloud covariance restated from the packed sums (the inverse of their second-moment matrix by cofactors, plane_segment.cpp:192-203:
 * cape_plane_segment.cov bit for bit); det_frames n x (x_axis, y_axis, center); det_areas; the rings one after the other in
 * det_vertices with det_counts[i] vertices each; det_segments[i] = index of the plane in the frame's segment list.
 * Returns 0; CAPE_ERR_INVALID_ARGUMENT for a buffer that is no shard of this layout (size, magic, no polygon sections, frame out of
 * range, an offset outside its section) or whose header reports dropped planes or rings (the kept-plane indices would not be the
 * reference's); CAPE_ERR_CAPACITY if an output is too small -- *n_det_out and *n_vertices_out say what the frame needs either way. */
int cape_host_shard_frame(const void* shard, uint64_t shard_bytes, const cape_gather_layout* layout, const cape_gather_polygon_layout* polygon_layout,
                          int32_t frame, int32_t capacity, int64_t vertices_capacity, double* det_planes, double* det_cov, double* det_frames,
                          double* det_areas, double* det_vertices, int32_t* det_counts, int32_t* det_segments, int32_t* n_det_out,
                          int64_t* n_vertices_out);

#ifdef __cplusplus
}
#endif

#endif /* CAPE_HOST_MAP_H */
