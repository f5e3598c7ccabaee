/* cape_host_map.h -- the host twins of libcape_primitives.so (host/polygon_capi.cpp) that track planes without the device: the map
 * matcher, the matcher of two consecutive frames, the visibility test in front of it, the map update, its halves, its commit and its list maintenance and the reader of a gathered shard, over a map in the layout of cape_map_upload (include/cape_hip.h) and a
 * frame's kept planes.  Not part of libcape_hip's C ABI: no function of libcape_hip takes these types. */
#ifndef CAPE_HOST_MAP_H
#define CAPE_HOST_MAP_H

#include "cape_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cape_map_track and its CAPE_MAP_TRACK_* / CAPE_MAP_RESULT_* enums are declared in cape_hip.h (cape_map_upload_tracks takes them). */
enum
{
    CAPE_MAP_ADD_STAGED = 1u << 0 /* append every kept plane of the frame that no map plane used as a staged plane (not one whose
                                     StagedMapPlane constructor would throw, nor one whose ring exceeds CAPE_MAP_MAX_RING) */
};

/* A map in the layout of cape_map_upload, with the tracking state parallel to the planes.  As an input the counts say what each
 * array holds, the capacities are not read, and `tracks` may be NULL where the call does not read it (cape_host_match_map).  As an
 * output (hence no const) the capacities say what each array takes, planes_capacity for `planes` and `tracks` alike, and the call
 * writes the counts: what it produced or, with CAPE_ERR_CAPACITY, what it needs. */
typedef struct cape_host_map
{
    cape_map_plane* planes;
    cape_map_ring* rings;
    double* vertices; /* (x, y) pairs */
    cape_map_track* tracks;
    int32_t n_planes, n_rings, planes_capacity, rings_capacity;
    int64_t n_vertices, vertices_capacity;
} cape_host_map;

/* A frame's kept planes: those Primitive_Detection keeps (polygon with CAPE_POLY_VALID and >= 3 vertices,
 * primitive_detection.cpp:623-631) in order, i.e. the reference's plane_container, whose indices every matcher result uses; n rows
 * per column.  As an input the capacities are not read; cape_host_match_map does not read cov, cape_host_map_update not areas,
 * neither segments.  As an output (cape_host_shard_frame) any column may be NULL, and n and n_vertices are written. */
typedef struct cape_host_planes
{
    int32_t n, capacity;
    int64_t n_vertices, vertices_capacity; /* (x, y) pairs of `vertices` */
    double* planes;                        /* (normal[3], d) */
    double* cov;                           /* 9 doubles: the point-cloud covariance (cape_plane_segment.cov) */
    double* frames;                        /* (x_axis[3], y_axis[3], center[3]) of the polygon */
    double* areas;                         /* the polygons' get_area(); as an input NULL = the area of each ring */
    double* vertices;                      /* the rings one after the other */
    int32_t* counts;                       /* the vertices of ring i */
    int32_t* segments;                     /* the index of plane i in the frame's segment list */
} cape_host_planes;

/* MapPlane::find_matches (map_primitive.cpp:91-161) as Feature_Map::get_matches drives it (feature_map.hpp:647-670), for ONE frame on
 * the host class: the twin of cape_match_map (tests/test_gpu_map_match.py compares them bit for bit) and the answer for a frame the
 * device flags CAPE_MATCH_EXACT_OVERFLOW.  world_to_camera: 16 doubles row-major (NULL = identity); skip: ceil(n_planes / 32) words
 * (NULL: none skipped); flags: CAPE_MATCH_*.  Outputs: match[n_planes], map_of[detected->n], inter_area[n_planes x detected->n]
 * (NULL: not kept) -- the area of every gated pair of a visited map plane with a positive projected area, -1 elsewhere.  Returns 0,
 * or CAPE_ERR_INVALID_ARGUMENT for a ring outside its array / of fewer than 3 vertices or a map plane without rings. */
int cape_host_match_map(const cape_host_map* map, const cape_host_planes* detected, const double* world_to_camera, const uint32_t* skip,
                        uint32_t flags, int32_t* match, int32_t* map_of, double* inter_area);

/* MapPlane::find_matches between two CONSECUTIVE frames on the host class, the kept planes of frame f-1 playing the map planes: the
 * twin of cape_match_polygons_wide and of cape_match_polygons_pose (tests/test_gpu_match_wide.py compares them bit for bit), with no
 * limit on the number of planes, and the answer for a frame either of them flags CAPE_MATCH_EXACT_OVERFLOW.  prev_to_cur16: 16
 * doubles row-major taking camera f-1's frame into camera f's; NULL = identity, for which -- like the device -- the previous
 * planes and polygons are used as they are.  flags: CAPE_MATCH_ADVANCED, CAPE_MATCH_ALLOW_INDEX0.  Per previous plane j in order:
 * the pose on the plane (plane_to_camera) and on its polygon (to_camera_space), the gates, cur's polygon i .inter_area(projected)
 * for every gated pair, the greatest area above the overlap threshold among the planes not taken yet (lowest index on a tie), the
 * `selectedIndex <= 0` quirk.  A previous plane whose own area (prev->areas, NULL: its ring's) is not positive matches nothing, its
 * areas are still reported.  Outputs: match[prev->n] and inter_area[prev->n x cur->n] (NULL: not kept; -1 for an ungated pair).
 * Returns 0, or CAPE_ERR_INVALID_ARGUMENT for a NULL argument, an unknown flag or a ring outside its array. */
int cape_host_match_planes(const cape_host_planes* prev, const cape_host_planes* cur, const double* prev_to_cur16, uint32_t flags,
                           int32_t* match, double* inter_area);

/* Feature_Map::update_map (feature_map.hpp:367-384, :701-830) for ONE frame on the host class, over the ordered list of
 * cape_map_upload (local planes first, then staged; CAPE_MAP_TRACK_STAGED tells them apart).  match[map->n_planes]: the kept plane
 * matched to map plane j (cape_host_match_map / cape_copy_map_matches) or -1; camera_to_world: 16 doubles row-major;
 * pose_covariance: 9 doubles; flags: CAPE_MAP_ADD_STAGED; next_id: the id of the first appended plane (advanced).  Per map plane in
 * list order: MapPlane::update_with_match if matched (map_primitive.cpp:204-251 with track, plane_with_tracking.cpp:15-82), then
 * update_matched / update_unmatched, the result bits of cape_map_track.  Then, with CAPE_MAP_ADD_STAGED, every kept plane that no map
 * plane used (a local plane uses its detection only on success, a staged plane either way, feature_map.hpp:790-797) becomes a
 * StagedMapPlane (map_primitive.cpp:262-285) in kept-plane order.  Outputs: map_out (every polygon as the host class stores it: outer
 * ring clockwise, holes counter-clockwise, rings plane after plane) and used_out[detected->n] (NULL: not written).  Returns 0;
 * CAPE_ERR_INVALID_ARGUMENT for a ring outside its array / of fewer than 3 vertices, a match out of range, or an invalid pose
 * covariance (update_map throws); CAPE_ERR_CAPACITY if an array of map_out is too small or NULL -- nothing is written then but the
 * three counts of map_out (next_id unchanged). */
int cape_host_map_update(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, const double* camera_to_world,
                         const double* pose_covariance, uint32_t flags, uint64_t* next_id, cape_host_map* map_out, int32_t* used_out);

/* The twin of cape_map_kalman (include/cape_hip.h) for ONE frame: the statements of cape_host_map_update above that concern a map
 * plane's state, up to but not including merge_union, with the detection's measurement given instead of derived -- so the device's own
 * z and R can be fed to it (tests/test_gpu_map_kalman.py compares the two bit for bit).  map: planes and tracks (rings and vertices
 * are not read); match[map->n_planes]: the kept plane matched to map plane j or -1; measurements: n_cur rows in KEPT-PLANE order
 * (cape_plane_measurement of cape_map_measure, or rows built from cape_host_plane_covariance / cape_host_world_plane_covariance /
 * plane_to_world).  The rules are cape_map_kalman's: a row with CAPE_MEASURE_FAIL_PLANE_COV / FAIL_WORLD_COV / BAD_POSE_COV (or
 * without CAPE_MEASURE_KEPT) is FAIL_DETECTION, a row with CAPE_MEASURE_FAIL_POLYGON has no usable polygon; the Kalman step,
 * normalize3 and get_plane_coordinate_system are those of the update.  Outputs: rows_out[n_cur] (cape_plane_fusion),
 * tracks_out[map->n_planes] (cape_map_track_result), frame_out (n_map, n_cur, CAPE_KALMAN_BAD_POSE_COV, n_updated); any may be
 * NULL.  Returns 0, or CAPE_ERR_INVALID_ARGUMENT for a NULL map, negative counts, n_cur > 128, a match out of range or a missing
 * array. */
int cape_host_map_kalman(const cape_host_map* map, const int32_t* match, const cape_plane_measurement* measurements, int32_t n_cur,
                         cape_frame_map_kalman* frame_out, cape_plane_fusion* rows_out, cape_map_track_result* tracks_out);

/* The twin of cape_map_union (include/cape_hip.h) for ONE frame, through the host class itself (Polygon::project, merge_union,
 * simplify): the very polygon step of cape_host_map_update above, so a served pair's ring, area and frame are the update's new map
 * polygon bit for bit.  map: planes, rings and vertices (tracks are not read); match[map->n_planes] (NULL: not checked): a pair needs
 * match[j] == i; fusion: n_cur rows of cape_map_kalman / cape_host_map_kalman in kept-plane order; measurements: n_cur rows of
 * cape_map_measure in kept-plane order (frame, vertex_count and flags are read); world_vertices: the world rings of kept planes
 * 0 .. n_cur - 1 back to back, ring i of measurements[i].vertex_count (x, y) pairs (vertex_offset is not read).  A pair exists where
 * the fusion row has map_plane = j >= 0 and CAPE_FUSION_FRAME and the measurement row has CAPE_MEASURE_KEPT and lacks
 * CAPE_MEASURE_FAIL_POLYGON.  Sets
 * CAPE_UNION_SERVED / UNCHANGED / DISJOINT / HOST_MAP_HOLES / HOST_NEW_HOLE; of CAPE_UNION_HOST_CAPACITY it knows the ring-length rule
 * (an operand of more than CAPE_MAP_UNION_MAX_RING vertices), the frame's slab and a union whose outer ring exceeds
 * CAPE_MAP_MAX_RING.  A union with interior rings is HOST_NEW_HOLE however many or how long they are, like the device's, which meets
 * holes but does not count them -- also where cape_host_map_update reports CAPE_MAP_RESULT_OVERFLOW for more than CAPE_MAP_MAX_HOLES
 * of them.  It never sets HOST_AMBIGUOUS, and n_nodes stays 0.  Outputs: rows_out[128] (zero beyond n_cur) and
 * vertices_out (room for CAPE_MAP_UNION_FRAME_VERTICES pairs; only the served rings are written).  Returns 0, or
 * CAPE_ERR_INVALID_ARGUMENT for a NULL argument, negative counts, n_cur > 128 or a map ring outside its array. */
int cape_host_map_union(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion, const cape_plane_measurement* measurements,
                        const double* world_vertices, int32_t n_cur, cape_plane_union* rows_out, double* vertices_out);

/* The twin of cape_debug_ring_union: one pair, ring_a the map plane's outer ring, ring_b the detection's, frames27 = (x, y, centre) of
 * ring a's frame, ring b's frame and the target frame (NULL: the canonical frame for all three).  row_out: one row (map_plane 0);
 * vertices_out: room for CAPE_MAP_MAX_RING pairs.  CAPE_ERR_INVALID_ARGUMENT: a NULL ring or output, n_a or n_b outside [3, 4096]. */
int cape_host_ring_union(const double* ring_a, int32_t n_a, const double* ring_b, int32_t n_b, const double* frames27, cape_plane_union* row_out,
                         double* vertices_out);

/* The twins of cape_map_union_holes and cape_debug_polygon_union (include/cape_hip.h): the arguments of the two calls above plus the
 * rings output (rings_out[128], zero beyond n_cur; one row for a pair), through the same polygon step, for a map plane with interior
 * rings and / or a union that creates some.  rings_a: ring a's outer ring and its interior rings back to back, counts_a[n_rings_a]
 * their lengths, n_rings_a in [1, 1 + CAPE_MAP_MAX_HOLES], every count and n_b in [3, 4096].  A served polygon's rings go to
 * vertices_out back to back, the outer ring first (room for CAPE_MAP_UNION_FRAME_VERTICES pairs in both calls); row.area is
 * Polygon::_area.  They never set HOST_MAP_HOLES or HOST_NEW_HOLE.  CAPE_UNION_HOST_HOLE_CUT where merge_union met a partly covered
 * hole, before every capacity.  Of CAPE_UNION_HOST_CAPACITY they know the rules that follow from inputs and results: a map plane of
 * more than 1 + CAPE_MAP_MAX_HOLES rings, a ring of the map plane or a detection of more than CAPE_MAP_UNION_MAX_RING vertices, more
 * than CAPE_MAP_UNION_HOLE_VERTICES vertices in the interior rings before simplify(), the update's own overflow (CAPE_MAP_MAX_RING,
 * CAPE_MAP_MAX_HOLES) and a polygon that does not fit the rest of the slab as a whole.  They never set HOST_AMBIGUOUS, and n_nodes
 * stays 0.  CAPE_ERR_INVALID_ARGUMENT as above, and for a NULL rings_out. */
int cape_host_map_union_holes(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion,
                              const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur, cape_plane_union* rows_out,
                              cape_plane_union_rings* rings_out, double* vertices_out);
int cape_host_polygon_union(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                            const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out);

/* The twins of cape_map_union_cut and cape_debug_polygon_union_cut: the signatures, outputs and capacity rules of the two above, for
 * a map plane whose hole the detection covers in part as well.  The host class computes the pieces of such a hole itself
 * (merge_union's carry_hole), so these never set CAPE_UNION_HOST_HOLE_CUT: the pair is served like any other, with
 * CAPE_UNION_HOLE_PIECES beside CAPE_UNION_SERVED where merge_union's `cut` branch ran (MergeInfo::holeCut), whatever became of the
 * pieces; rings.holes_covered counts the wholly covered holes only.  A pair without a partly covered hole has the rows of the twins
 * above.  Of the device's CAPE_UNION_HOST_CAPACITY they do not know the second arrangement's own limits (its cuts, nodes, degrees and
 * walks): such a pair is served here. */
int cape_host_map_union_cut(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion,
                            const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur, cape_plane_union* rows_out,
                            cape_plane_union_rings* rings_out, double* vertices_out);
int cape_host_polygon_union_cut(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                                const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out);

/* The twin of cape_map_commit (include/cape_hip.h) for ONE frame, and its reference byte for byte: the map after the frame from the
 * results of the calls before it, with no arithmetic of its own.  map: planes, rings, vertices and tracks; frame: goes into the result
 * only; frame_header and track_results[map->n_planes]: cape_map_kalman's (or cape_host_map_kalman's) for the frame; fusion,
 * measurements and world_vertices: n_cur rows in kept-plane order and the world rings back to back (ring i of
 * measurements[i].vertex_count pairs; vertex_offset is not read), as cape_host_map_union takes them, n_cur being frame_header->n_cur
 * (0 for a frame flagged CAPE_MATCH_EXACT_OVERFLOW, at most 128); union_rows[128], rings[128] (NULL: the rows are a plain
 * cape_map_union's, one ring per pair) and slab (CAPE_MAP_UNION_FRAME_VERTICES pairs): the frame's union results; flags:
 * CAPE_COMMIT_ADD_STAGED; next_id: the id of the first appended plane (advanced if DONE).  The rules are cape_map_commit's, written
 * once in csrc/cape_map_commit.h; the planes go through the host class and put_map like those of cape_host_map_update, which this
 * call equals where the rows come from the host algebra and every pair is served.  result_out is always written.  Returns 0 for a
 * DONE and for a refused frame alike -- a refused one (result_out->flags lacks CAPE_COMMIT_DONE) leaves map_out and next_id
 * untouched; CAPE_ERR_INVALID_ARGUMENT for a NULL argument the frame needs, a negative count or frame, an unknown flag;
 * CAPE_ERR_CAPACITY if an array of map_out is too small or NULL -- nothing is written then but the three counts of map_out. */
int cape_host_map_commit(const cape_host_map* map, int32_t frame, const cape_frame_map_kalman* frame_header,
                         const cape_map_track_result* track_results, const cape_plane_fusion* fusion, const cape_plane_measurement* measurements,
                         const double* world_vertices, const cape_plane_union* union_rows, const cape_plane_union_rings* rings, const double* slab,
                         uint32_t flags, uint64_t* next_id, cape_host_map* map_out, cape_map_commit_result* result_out);

/* The twin of cape_map_maintain (include/cape_hip.h), and its reference byte for byte: PROMOTE, DROP and LOST executed on `map`
 * (planes, rings, vertices and tracks) -- the decisions are cape_map_maintain's, written once in csrc/cape_map_maintain.h and taken
 * one plane after the other (maintain_plan_serial); a promote candidate is promotable where mt::is_covariance_valid of its 4 x 4
 * covariance and |normal| = 1 within DBL_EPSILON hold; the planes then go through the host class and put_map like those of
 * cape_host_map_commit.  map_out: the new map, a stable partition of the survivors (not staged first, then staged).  retired_out: the
 * retired log, an INPUT AND an output -- its counts say what it holds on entry (they, not the arrays, decide
 * CAPE_MAINTAIN_LOG_FULL against CAPE_MAP_RETIRED_MAX_PLANES), the lost planes are appended behind that with ring_first and
 * vertex_offset relative to the log's own arrays, and the counts are advanced.  result_out is always written.  Returns 0 for DONE,
 * NOTHING and a refusal alike -- only DONE writes map_out and retired_out; CAPE_ERR_INVALID_ARGUMENT for a NULL argument, a negative
 * count or a map plane without a polygon; CAPE_ERR_CAPACITY if an array of map_out or retired_out is too small or NULL (the old map's
 * sizes, and the log's plus the old map's, always suffice) -- nothing is written then. */
int cape_host_map_maintain(const cape_host_map* map, cape_host_map* map_out, cape_host_map* retired_out, cape_map_maintain_result* result_out);

/* One frame of a packed shard -- the bytes cape_pack_primitives writes with CAPE_GATHER_POLYGONS, as they arrive from
 * cape_gather_primitives[_root] or any other transport -- as the kept planes the two calls above take: no handle, no device.
 * `frame` counts from the shard's first frame.  Each plane goes through the host class's Polygon(ring, xAxis, yAxis, center)
 * constructor, which is where ring, axes and area come from; cov is restated from the packed sums (the inverse of their
 * second-moment matrix by cofactors, plane_segment.cpp:192-203: cape_plane_segment.cov bit for bit).  Returns 0;
 * CAPE_ERR_INVALID_ARGUMENT for a buffer that is no shard of this layout (size, magic, no polygon sections, frame out of range, an
 * offset outside its section) or whose header reports dropped planes or rings (the kept-plane indices would not be the
 * reference's); CAPE_ERR_CAPACITY if detected_out is too small -- its n and n_vertices say what the frame needs either way. */
int cape_host_shard_frame(const void* shard, uint64_t shard_bytes, const cape_gather_layout* layout, const cape_gather_polygon_layout* polygon_layout,
                          int32_t frame, cape_host_planes* detected_out);

/* The skip words of ONE frame on the host class: bit j = bit j of `moving` is set, or MapPlane::is_visible(world_to_camera) is false
 * (map_primitive.cpp:186-189: to_camera_space, then Polygon::is_visible_in_screen_space of host/boundary_polygon.hpp with the given
 * image size and intrinsics).  The twin of cape_map_visibility (tests/test_gpu_map_visibility.py compares them bit for bit; the
 * device takes a bounding-box shortcut, this function none) and the answer for a caller without a device.  world_to_camera: 16
 * doubles row-major (NULL = identity); moving: ceil(n_planes / 32) words, one bit per map plane (NULL: none); skip_out:
 * ceil(n_planes / 32) words, the bits beyond n_planes in the last word 0.  Returns 0, or CAPE_ERR_INVALID_ARGUMENT for a NULL map or
 * skip_out (with n_planes > 0), a negative n_planes, a width or height below 3, a ring outside its array / of fewer than 3 vertices
 * or a map plane without rings (nothing is written then). */
int cape_host_map_visibility(const cape_host_map* map, const double* world_to_camera, int32_t width, int32_t height, double fx, double fy,
                             double cx, double cy, const uint32_t* moving, uint32_t* skip_out);

/* The twin of cape_map_pose_score (include/cape_hip.h) for ONE frame (host/pose_score.cpp), on the rules of csrc/cape_pose_score.h
 * that the kernels compile too: the plane cost function of the pose solver -- PlaneOptimizationFeature's is_inlier, get_distance and
 * get_score (map_primitive.cpp:15-85) -- for n_hypotheses poses.  map: planes and tracks (covariance and id; rings and vertices are not
 * read); match[map->n_planes]: the kept plane matched to map plane j or -1 (cape_copy_map_matches_wide's row of the frame);
 * detected: the frame's kept planes, of which `planes` (normal[3], d) is read; frame_flags: the frame's flags of the wide match
 * (CAPE_MATCH_EXACT_OVERFLOW: the frame reports that flag, n_pairs = 0 and zeros); world_to_camera: n_hypotheses x 16 doubles
 * row-major.  The map plane goes through utils::plane_to_camera.  Outputs, any may be NULL: scores_out[n_hypotheses],
 * features_out[128] (zero beyond n_pairs), residuals_out[n_hypotheses x 128 x 7] (signed[4] then reduced[3], zero beyond n_pairs).
 * Everything equals the device bit for bit except the three angle parts of `signed`, which are this host's libm's (and what follows
 * from a part within a few ulp of its threshold).  Returns 0, or CAPE_ERR_INVALID_ARGUMENT for a NULL map, detected or poses, negative
 * counts, more than 128 kept planes, n_hypotheses < 1, an unknown frame flag, a match out of range or a missing array. */
int cape_host_pose_score(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                         int32_t n_hypotheses, const double* world_to_camera, cape_pose_score* scores_out, cape_pose_feature* features_out,
                         double* residuals_out);

/* The twin of cape_map_pose_solve (include/cape_hip.h) for ONE frame (host/pose_solve.cpp), on the rules of csrc/cape_pose_solve.h that
 * the kernel compiles too: MINPACK's lmstr driver over forward differences on the frame's pairs, problem after problem.  map, match,
 * detected, frame_flags: as cape_host_pose_score takes them (its pairs and feature rows are used).  x0: n_problems x 6 doubles;
 * subsets: n_problems x 4 words (bit i: the pair of kept plane i takes part); or, with `selection` given, n_problems = 1 and the
 * problem comes from its x and inlier_words (CAPE_POSE_SOLVE_FROM_SELECTION; a selection without a best gives
 * CAPE_POSE_SOLVE_NO_SELECTION).  params: NULL = the defaults.  Outputs, any may be NULL: solutions_out[n_problems],
 * world_to_camera_out[n_problems x 16], n_rank_deficient_out: the problems in which the pivoted qrfac ran
 * (CAPE_POSE_SOLVE_RANK_DEFICIENT), for the tests.  Everything equals the device bit for bit.  Returns 0, or
 * CAPE_ERR_INVALID_ARGUMENT for what cape_host_pose_score refuses, a missing input or a parameter out of range. */
int cape_host_pose_solve(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                         int32_t n_problems, const double* x0, const uint32_t* subsets, const cape_pose_selection* selection,
                         const cape_pose_solve_params* params, cape_pose_solution* solutions_out, double* world_to_camera_out,
                         int32_t* n_rank_deficient_out);
/* The twin of cape_map_pose_select for ONE frame: pose_select_frame over the frame's n_hypotheses score rows and solution rows. */
int cape_host_pose_select(int32_t n_hypotheses, const cape_pose_score* scores, const cape_pose_solution* solutions,
                          cape_pose_selection* selection_out);

/* The twin of cape_map_pose_covariance (include/cape_hip.h) for ONE frame (host/pose_covariance.cpp), on the rules of
 * csrc/cape_pose_covariance.h that the kernels compile too: vary, a minimisation per iteration, the reduction.  map, match, detected,
 * frame_flags: as cape_host_pose_score takes them.  x: 6 doubles and subset: 4 words; or, with `solution` and `selection` given (both or
 * neither), the refit's row and the selection it came from (CAPE_POSE_COVARIANCE_FROM_SOLUTION).  deviates: the table
 * [n_iterations][128][4], or NULL for Philox keyed by `seed` at frame index `frame_index` (= frame_base + the frame of the device's call).
 * Outputs, any may be NULL: row_out, samples_out[n_iterations] (the solution rows; 0 for a refused frame), vectors_out[n_iterations x 6]
 * (the pose vectors the reduction reads).  With a table everything equals the device bit for bit except the three Euler angles of a
 * vector and what the reduction makes of them, which are this host's libm's.  Returns 0, or CAPE_ERR_INVALID_ARGUMENT. */
int cape_host_pose_covariance(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                              int32_t n_iterations, const double* x, const uint32_t* subset, const cape_pose_solution* solution,
                              const cape_pose_selection* selection, const double* deviates, uint64_t seed, uint32_t frame_index,
                              const cape_pose_solve_params* params, cape_pose_covariance* row_out, cape_pose_solution* samples_out,
                              double* vectors_out);
/* The twin of cape_pose_draw_deviates: the table [n_iterations][128][4] of frame index `frame`; flags: 0 or CAPE_POSE_DRAW_UNIFORMS.  The
 * uniforms equal the device's bit for bit; the normals go through this host's log, cos and sin. */
int cape_host_pose_draw_deviates(uint64_t seed, uint32_t frame, int32_t n_iterations, double* out, uint32_t flags);
/* Single statements of csrc/cape_pose_covariance.h, for the tests: a Philox4x32-10 block; the variation of a map plane; the pose vector
 * of x (and, if asked for, the rotation matrix its angles are taken of); Eigen's eulerAngles(0, 1, 2) of a row-major rotation. */
void cape_host_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4);
void cape_host_pose_vary_plane(const double* map_plane4, const double* stddev4, const double* z4, double* out4);
void cape_host_pose_vector(const double* x6, double* vector6_out, double* rotation9_out);
void cape_host_euler_angles_012(const double* rotation9, double* angles3_out);

#ifdef __cplusplus
}
#endif

#endif /* CAPE_HOST_MAP_H */
