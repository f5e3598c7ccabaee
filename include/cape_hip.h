/*
 * cape_hip.h -- C ABI of the MI355X-native CAPE plane/cylinder extractor (libcape_hip.so).
 *
 * This is the drop-in boundary for ONE path of BaptisteHudyma/RGB-D-SLAM: the `primitives` library
 * (reference CMakeLists.txt:117-123), i.e. Depth_Map_Transformation::get_organized_cloud_array +
 * Primitive_Detection::find_primitives.  The reference has no FFI layer; the functions below are what a
 * binding for that library would call.  Each entry point cites the reference interface it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the reference-side shim.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns CAPE_OK (0) or a negative
 * cape_status and never throws, exits or logs to stdout (the reference's exit(-1)/terminate paths,
 * histogram.hpp:105-109, become error codes).  A handle is not thread-safe; distinct handles are.
 * All device work of a call is enqueued on the caller's HIP stream (`stream` is a hipStream_t passed as
 * void*; NULL = the null stream).
 *
 * Streams: ONE stream is in flight per handle -- the per-handle scratch and result buffers carry no per-buffer events.
 * A call made with another stream than the previous call's is ordered behind the handle's earlier work ON THE DEVICE
 * (hipStreamWaitEvent on a handle-owned event recorded behind every enqueue): it neither blocks the host nor touches
 * the previous stream, which the caller may destroy as soon as it has no further use for it.  The stream of the LAST
 * call must stay alive until that work has been waited for (cape_copy_results / cape_host_results / a stream
 * synchronisation of the caller's) -- the usual HIP rule for any enqueued work.
 */
#ifndef CAPE_HIP_H
#define CAPE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI number of this header: bumped whenever a struct below changes size or meaning (cape_abi_version() returns the library's;
 * a binding built against another number must not call it).  2 = round 6: cape_frame_header grew by next_record / segment_base
 * (frames of more than 64 plane segments continue in spill records), cape_config by spill_records, cape_timings holds the
 * reference's five buckets (12 fields), the frame status carries bit 7 and a count in bits 8..15. */
#define CAPE_ABI_VERSION 2

#define CAPE_CELL_SIZE 20          /* parameters::detection::depthMapPatchSize_px, src/parameters.hpp:79-80 */
#define CAPE_MAX_PLANES 64         /* plane segments ONE RECORD holds.  _planeSegments is an unbounded std::vector in the reference
                                      (primitive_detection.hpp:206): a frame with more continues in spill records, see
                                      cape_frame_header.next_record.  Frames with up to 32 segments run entirely in the fast
                                      kernels, up to 64 in a 64-segment instance, the others in the general instance */
#define CAPE_MAX_CYLINDERS 64      /* cylinder labels one record holds (cylinder2regionMap, likewise unbounded: same chain) */

typedef enum cape_status
{
    CAPE_OK = 0,
    CAPE_ERR_INVALID_ARGUMENT = -1,
    CAPE_ERR_NO_DEVICE = -2,       /* no HIP device / runtime error at create: the product has NO CPU fallback */
    CAPE_ERR_HIP = -3,             /* a HIP runtime call failed; cape_last_error() has the text */
    CAPE_ERR_CAPACITY = -4,        /* n_frames > max_batch */
    CAPE_ERR_UNSUPPORTED = -5
} cape_status;

enum
{
    CAPE_FLAG_CYLINDERS = 1u << 0, /* run cylinder RANSAC on low-score regions (primitive_detection.cpp:385-388);
                                      cleared = "plane-only" mode of BASELINE.json configs[0..1] */
    CAPE_FLAG_ASYNC_SECOND_PASS = 1u << 1, /* batches with cylinders: the second pass of stage B (the frames that reach a cylinder
                                      candidate; it lasts as long as its slowest frame) runs on a stream of the handle's own and
                                      cape_extract's caller stream does NOT wait for it.  Every later entry point on the handle
                                      (the next cape_extract, cape_copy_results, cape_pack_primitives, ...) orders itself behind
                                      it; a consumer of the raw cape_device_results pointers calls cape_sync_results first.
                                      Meant for TWO handles fed alternately: one's streaming kernels run under the other's tail */
};

/* per-frame status bits (cape_frame_header.status) */
enum
{
    CAPE_FRAME_PLANE_OVERFLOW = 1u << 0,    /* the handle's pool of spill records (cape_config.spill_records) ran out while this frame
                                               needed one more: the frame is truncated at the records it got */
    CAPE_FRAME_BOUNDARY_OVERFLOW = 1u << 1, /* boundary point capacity exceeded */
    CAPE_FRAME_CYL_OVERFLOW = 1u << 2,
    CAPE_FRAME_BIN_NEAR_EDGE = 1u << 3,     /* a cell's histogram angle fell within 1e-9 of a bin edge (libm tie risk) */
    CAPE_FRAME_INORDER_CELLS = 1u << 4,     /* >=1 cell took the in-order accumulation path (exactness guard) */
    CAPE_FRAME_RNG_EXHAUSTED = 1u << 5,     /* RANSAC asked for more draws than the precomputed mt19937 table */
    CAPE_FRAME_SEED_LIMIT = 1u << 6,        /* the seed loop hit its iteration guard (4 * cells + 1024; provably unreachable) */
    CAPE_FRAME_INVALID_SEED = 1u << 7       /* the seed loop ended on "Could not find a single plane segment: invalid seed"
                                               (log_warning, primitive_detection.cpp:299-304) */
};
/* bits 8..15 of the status: how many times the frame logged "Plane segment is not planar after merge" (primitive_detection.cpp:374
 * for a grown region, :497 for a cylinder sub-segment), saturating at 255 */
#define CAPE_FRAME_NOT_PLANAR_SHIFT 8
#define CAPE_FRAME_NOT_PLANAR_COUNT(status) (((status) >> CAPE_FRAME_NOT_PLANAR_SHIFT) & 0xFFu)

/*
 * Replaces: Depth_Map_Transformation(width,height,cellSize) + Primitive_Detection(width,height) constructors
 * (src/rgbd_slam.cpp:48-57) and the process-global camera intrinsics they read lazily
 * (Parameters::get_camera_1_intrinsics, src/parameters.hpp:144-149).
 */
typedef struct cape_config
{
    int32_t width;      /* multiple of 20; at most 256 cells wide (5120 px) and 65 535 cells in all -- grids of up to 128 x 64 cells */
    int32_t height;     /* multiple of 20     (2560 x 1280 px) run in the fast kernels, larger ones in the general instance      */
    double fx, fy, cx, cy;
    uint32_t flags;     /* CAPE_FLAG_* */
    int32_t device;     /* HIP device ordinal */
    int32_t max_batch;  /* frames per cape_extract call (sizes the per-frame scratch and result buffers) */
    int32_t boundary_capacity; /* boundary points per frame; 0 = 2 * cells */
    int32_t sub_batches; /* 0/1: the whole batch runs kernel after kernel on the caller's stream.  k > 1: the batch is
                            cut in k sub-batches that alternate between two internal streams (forked from / joined
                            into the caller's stream), so the latency-bound grow kernel of one sub-batch overlaps
                            the streaming cell kernel of the next */
    int32_t spill_records; /* records (each with its own boundary slab) in the handle's spill pool, shared by the frames of a batch
                            that hold more than 64 plane segments or cylinder labels; 0 = max(8, max_batch / 8).  A frame needs
                            ceil(n / 64) - 1 of them; at most cells / max(1, min(6, uint(0.0065 cells))) segments can exist */
} cape_config;

typedef struct cape_handle_s* cape_handle;

/* One plane segment of a frame = one element of Primitive_Detection::_planeSegments after merge_planes()
 * (primitive_detection.cpp:503-560) plus what Plane(planeSeg, polygon) derives from it
 * (shape_primitives.cpp:48-56).  Field names follow Plane_Segment (plane_segment.hpp:122-139). */
typedef struct cape_plane_segment
{
    double normal[3];       /* PlaneCoordinates::_normal of the segment */
    double d;
    double centroid[3];
    double mse;
    double score;
    double sums[9];         /* Sx Sy Sz Sxs Sys Szs Sxy Syz Szx */
    double out_normal[3];   /* Plane::_parametrization normal (one more normalisation) ; valid if is_output */
    double cov[9];          /* Plane_Segment::get_point_cloud_covariance(), row-major ; valid if is_output */
    uint32_t point_count;
    uint32_t merge_label;   /* planeMergeLabels[i]: index in the FRAME's segment list (may point into an earlier record of the chain) */
    uint32_t planar;
    uint32_t is_output;     /* root of its merge group, planar and >= 3 boundary points: becomes a `Plane` */
    uint32_t boundary_offset; /* first point in the boundary slab of the record that holds this segment */
    uint32_t boundary_count;
} cape_plane_segment;

typedef struct cape_cylinder
{
    double axis[3];         /* Cylinder::_normal */
    double radius;          /* NaN, as in the reference (shape_primitives.cpp:17-24 over a copy with 0 segments) */
    uint32_t kept;          /* survived add_cylinders_to_primitives (primitive_detection.cpp:705-734) */
    uint32_t region;        /* cylinder2regionMap[i].first */
} cape_cylinder;

typedef struct cape_frame_header
{
    int32_t n_plane_segments; /* _planeSegments.size() -- counted FROM THIS RECORD ON: the frame's first record holds the whole
                                 frame's count, the record itself the first min(64, n) of them, the rest follow next_record */
    int32_t n_planes;         /* number of segments with is_output (= planeContainer.size() before polygon tests), from this record on */
    int32_t n_cylinder_labels;/* cylinder2regionMap.size(), from this record on (the record holds the first min(64, n)) */
    int32_t n_cylinders;      /* cylinderContainer.size(), from this record on */
    int32_t n_boundary_points;/* points in THIS record's boundary slab */
    int32_t n_seeds;          /* iterations of the seed loop (debug) */
    uint32_t status;          /* CAPE_FRAME_* */
    int32_t n_planar_cells;
    int32_t next_record;      /* -1, or the index in the handle's record array (>= max_batch: a spill record) of the record that
                                 continues this frame: segments / cylinders 64.. of it, with its own boundary slab, polygons, vertices */
    int32_t segment_base;     /* index of segments[0] (and cylinders[0]) of this record in the frame's lists: 0, 64, 128, ... */
} cape_frame_header;

/* Fixed-capacity record (stays on the producing GPU / goes to its host; the multi-GPU gather ships the packed lists below).
 * The handle's record array holds max_batch records -- record f is frame f of the batch -- followed by the spill pool
 * (cape_config.spill_records).  A frame with more than 64 plane segments (a checkerboard of small facets) or cylinder labels is a
 * CHAIN of records linked by header.next_record; every record of the chain owns a boundary slab, a polygon row and a vertex slab
 * at its own index, so whatever consumes "record i" (polygons, the host conversion) works on spill records unchanged. */
typedef struct cape_frame_record
{
    cape_frame_header header;
    cape_plane_segment segments[CAPE_MAX_PLANES];
    cape_cylinder cylinders[CAPE_MAX_CYLINDERS];
} cape_frame_record;

/*
 * Multi-GPU exchange (BASELINE.json configs[3], [4]).  Frames shard by contiguous blocks, one GPU per
 * block, no collective inside a frame; once per batch the ranks all-gather what plane_container / cylinder_container
 * hold after find_primitives (shape_primitives.hpp:129-130), optionally with the two label grids.  The lists are ragged,
 * so each rank PACKS its shard on the device into one buffer of a fixed byte count (what ncclAllGather needs):
 *
 *   cape_packed_header | frames_capacity x cape_packed_frame | planes_capacity x cape_packed_plane |
 *   cylinders_capacity x cape_packed_cylinder | [frames_capacity x cells u8 plane labels | same, cylinder labels] |
 *   [cape_packed_polygon_header | polygons_capacity x cape_polygon | vertices_capacity x 2 doubles]
 *
 * planes_capacity = frames_capacity x planes_per_frame is a budget for the whole shard, not per frame: nothing is
 * truncated unless the shard's TOTAL exceeds it, which the header reports (planes_per_frame = CAPE_MAX_PLANES can never
 * overflow).  Sections start on 16-byte boundaries; cape_gather_layout has the offsets.
 *
 * The label grids travel with CAPE_GATHER_LABELS.  The last three sections travel with CAPE_GATHER_POLYGONS (they come last,
 * behind the label grids when both flags are set; every other section keeps the offset and the bytes it has without the flag):
 * the boundary polygon of every packed plane as cape_build_polygons built it, so that a receiver can tell which planes the
 * reference keeps (CAPE_POLY_VALID and >= 3 vertices: the indices of its plane_container) and hand the rings to find_matches /
 * the map update.  polygons_capacity = planes_capacity: polygon k belongs to plane k of the planes section, so
 * cape_packed_frame.plane_offset / n_planes index both.  A packed cape_polygon is the record cape_copy_polygons shows for that
 * segment, bit for bit, except that `segment` is the index in the FRAME's segment list (= cape_packed_plane.segment) and
 * `vertex_offset` counts from the start of the shard's vertex section.  The rings lie in that section in plane order, without
 * gaps.  vertices_capacity = frames_capacity x vertices_per_frame is a budget for the shard like planes_capacity, and a ring
 * travels whole or not at all: the rings that travel are exactly the longest prefix, in packed-plane order, of the rings whose
 * vertices fit the budget together.  A ring beyond it leaves its polygon with vertex_count = 0 and vertex_offset = UINT32_MAX
 * (flags, axes, centre and area are kept), and the header says CAPE_PACKED_VERTICES_DROPPED.  A polygon that has no ring on the
 * producing GPU either (CAPE_POLY_OVERFLOW, CAPE_POLY_REJECTED) has vertex_count = 0 and vertex_offset = 0.  A plane that was
 * dropped itself (CAPE_PACKED_PLANES_DROPPED) has no polygon.  vertices_per_frame = boundary_capacity can never overflow for
 * frames of one record (a ring's vertices are boundary points of its record's slab); a frame that continues in spill records
 * holds at most boundary_capacity vertices per record of its chain, so boundary_capacity x (1 + spill_records) per frame --
 * or, for the shard, boundary_capacity x (frames_capacity + spill_records) vertices in all -- can never overflow.
 */
#define CAPE_PACKED_MAGIC 0x43415045u /* "CAPE" */
enum
{
    CAPE_GATHER_LABELS = 1u << 0, /* also ship _gridPlaneSegmentMap / _gridCylinderSegMap, one byte per cell each */
    CAPE_GATHER_POLYGONS = 1u << 1 /* also ship the boundary polygon of every packed plane (cape_build_polygons of the batch first) */
};
/* vertices_per_frame when none is asked for (0, or cape_gather_configure with CAPE_GATHER_POLYGONS).  Measured with
 * cape_count_polygon_vertices on 640 x 480 batches (profiles/r08_gather_polygons.txt): 32.5 vertices per frame on the 4 096-frame
 * room batch (at most 102 in one frame), 8.0 on the tunnel batch (51), 57.3 on the 2 048-frame TUM-like stream (156).  The default
 * covers the largest of the three means with 25 % headroom, ceil(1.25 x 57.34) = 72 -- the rule INTEGRATION.md gives for
 * planes_per_frame; a caller with other scenes sizes the budget from its own previous batch the same way. */
#define CAPE_GATHER_DEFAULT_VERTICES_PER_FRAME 72
enum
{
    CAPE_PACKED_PLANES_DROPPED = 1u << 0,   /* cape_packed_header.overflow */
    CAPE_PACKED_CYLINDERS_DROPPED = 1u << 1,
    CAPE_PACKED_LABELS_CLIPPED = 1u << 2,   /* a frame of the shard holds more than 255 plane segments / cylinder labels: its label
                                               grids (one byte per cell on the wire) read 255 where the label is larger */
    CAPE_PACKED_VERTICES_DROPPED = 1u << 3  /* CAPE_GATHER_POLYGONS: the rings of the shard hold more vertices than vertices_capacity;
                                               the longest prefix of rings that fits travels, the others have vertex_count = 0 */
};
typedef struct cape_packed_header
{
    uint32_t magic;             /* CAPE_PACKED_MAGIC */
    int32_t n_frames;           /* frames of this shard */
    int32_t first_frame;        /* index of the shard's first frame in the whole batch (caller supplied) */
    int32_t n_planes_total;     /* planes found in the shard; only min(total, capacity) are listed */
    int32_t n_cylinders_total;
    int32_t planes_capacity;
    int32_t cylinders_capacity;
    uint32_t overflow;          /* CAPE_PACKED_*_DROPPED */
    uint32_t status_or;         /* OR of the frames' CAPE_FRAME_* flag bits (bits 0..7; the count in bits 8..15 of a frame's status is not folded) */
    int32_t cells;
    int32_t frames_capacity;
    uint32_t flags;             /* CAPE_GATHER_* */
} cape_packed_header;
typedef struct cape_packed_frame
{
    int32_t plane_offset;       /* first plane of the frame in the planes section */
    int32_t n_planes;           /* planeContainer.size() before the polygon validity test (primitive_detection.cpp:623-631); with
                                   CAPE_GATHER_POLYGONS the planes the reference keeps are those whose packed polygon has
                                   CAPE_POLY_VALID and >= 3 vertices, in this order */
    int32_t cylinder_offset;
    int32_t n_cylinders;        /* cylinderContainer.size() */
    uint32_t status;            /* CAPE_FRAME_* */
    int32_t n_plane_segments;
} cape_packed_frame;
typedef struct cape_packed_plane /* SURVEY.md 8e record: the planeSeg of Plane(planeSeg, polygon); the polygon is entry k of the
                                    polygons section for plane k with CAPE_GATHER_POLYGONS, and does not travel without it */
{
    double normal[3];           /* Plane::get_normal() */
    double d;                   /* Plane::get_d() */
    double centroid[3];
    double mse;
    double score;
    double sums[9];             /* Sx Sy Sz Sxs Sys Szs Sxy Syz Szx: get_point_cloud_covariance() follows from them */
    uint32_t point_count;
    uint32_t segment;           /* index of the segment in the producing frame's record */
} cape_packed_plane;
typedef struct cape_packed_cylinder
{
    double axis[3];
    double radius;              /* NaN, as in the reference */
} cape_packed_cylinder;

typedef struct cape_gather_config
{
    int32_t frames_capacity;     /* largest shard (frames per rank) this handle will pack; <= max_batch */
    int32_t planes_per_frame;    /* budget: planes_capacity = frames_capacity x planes_per_frame; 0 = 16; <= 4096 */
    int32_t cylinders_per_frame; /* 0 = 8 */
    uint32_t flags;              /* CAPE_GATHER_LABELS | CAPE_GATHER_POLYGONS */
} cape_gather_config;
typedef struct cape_gather_layout
{
    uint64_t bytes_per_rank;
    uint64_t frames_offset, planes_offset, cylinders_offset, plane_labels_offset, cyl_labels_offset; /* labels: 0 if absent */
    int32_t frames_capacity, planes_capacity, cylinders_capacity, cells;
} cape_gather_layout;
/* the sections CAPE_GATHER_POLYGONS appends (cape_gather_configure_polygons) */
typedef struct cape_packed_polygon_header
{
    int64_t n_vertices_total;   /* vertices of the rings of every plane found in the shard (= cape_count_polygon_vertices); only the
                                   rings of the longest prefix that fits vertices_capacity are listed */
    int32_t vertices_capacity;
    int32_t n_polygons_valid;   /* planes found in the shard that the reference keeps (CAPE_POLY_VALID and >= 3 vertices) */
} cape_packed_polygon_header;
typedef struct cape_gather_polygon_layout
{
    uint64_t polygon_header_offset, polygons_offset, vertices_offset;
    int32_t polygons_capacity;  /* = planes_capacity */
    int32_t vertices_capacity;  /* = frames_capacity x vertices_per_frame */
} cape_gather_polygon_layout;

/* Per-cell statistics (debug / parity access to Primitive_Detection::_planeGrid, _cellDistanceTols,
 * Histogram::_bins; primitive_detection.hpp:205-218).  One struct per cell, cell-row-major. */
typedef struct cape_cell_stats
{
    double sums[9];
    double normal[3];
    double d;
    double centroid[3];
    double mse;
    double score;
    float tol;
    uint32_t point_count;
    int32_t bin;            /* histogram bin right after init_histogram, -1 if not planar */
    uint32_t planar;
    uint32_t inorder;       /* 1 if the exactness guard sent this cell through the in-order path */
    uint32_t pad;
} cape_cell_stats;

typedef struct cape_timings
{
    /* mirrors the reference's stage buckets (primitive_detection.hpp:233-239), from HIP events, seconds,
     * accumulated over calls made with CAPE timing enabled */
    double cell_fit_s;      /* _initTime : back-projection + per-cell PCA (stage A = the two kernels below) */
    double cell_moments_s;  /*   A1 cape_cell_moments_kernel (streaming pass over the depth image) */
    double cell_plane_s;    /*   A2 cape_cell_plane_kernel (per-cell plane fit, tolerance, histogram bin) */
    double grow_s;          /* _growTime + _mergeTime + _refineTime : stage B kernel */
    double total_s;
    uint64_t frames;
    uint64_t calls;         /* number of cape_extract calls folded into the sums (= launches of each kernel) */
    /* The reference's five buckets, one to one (find_primitives, primitive_detection.cpp:126-160; show_statistics :69-117):
     *   reset_s       _resetTime : reset_data().  Nothing persists between frames here (row A14) and the hand-over counters are
     *                 cleared by a thread of stage A2: there is no reset pass to time, the bucket is 0 by construction
     *   init_s        _initTime  : init_planar_cell_fitting + init_histogram = kernels A1 + A2 (= cell_fit_s; the histogram's
     *                 bins are A2's, its counting is the first microseconds of the grow kernel)
     *   grow_phase_s  _growTime  : grow_planes_and_cylinders (seed loop, region growing, cylinder_fitting)
     *   merge_s       _mergeTime : merge_planes
     *   refine_s      _refineTime: add_planes_to_primitives + add_cylinders_to_primitives WITHOUT the boundary polygon (that is
     *                 cape_build_polygons or the host class; the overlay adds its own clock for it)
     * grow / merge / refine share the stage-B kernels: every frame's wave books the shader-clock ticks it spends in each of the
     * three (three atomics per frame, only while timing is on) and grow_s -- the kernels' HIP-event time -- is split in those
     * proportions: grow_phase_s + merge_s + refine_s == grow_s.  The split is an ESTIMATE weighted by wave occupancy, not three wall
     * times: a frame that is redone books its grow ticks in both passes, the workgroup finisher books one of its four waves, and only
     * the SUM of the three is measured (the HIP events). */
    double reset_s, init_s, grow_phase_s, merge_s, refine_s;
} cape_timings;

typedef struct cape_layout
{
    int32_t h_cells, v_cells, cells;
    int32_t boundary_capacity;
    uint64_t frame_record_bytes;  /* sizeof(cape_frame_record) */
    int32_t compute_units;        /* CUs of the handle's device */
    int32_t grow_frames_per_cu;   /* frames (one wavefront each) the grow kernel keeps in flight per CU (occupancy API) */
    uint32_t effective_flags;     /* the CAPE_FLAG_* bits that are ACTIVE on this handle: CAPE_FLAG_ASYNC_SECOND_PASS is
                                     cleared here when the handle cannot overlap (cylinders off, max_batch <= 8 or
                                     sub_batches > 1), so a caller can tell whether the mode it asked for is in force */
    uint32_t reserved;
} cape_layout;

/* Number of HIP devices this process sees (0 and CAPE_ERR_NO_DEVICE without a GPU): what a host-side batch API shards
 * over (one handle per device). */
int cape_device_count(int32_t* count_out);

/* Depth_Map_Transformation / Primitive_Detection constructors (src/rgbd_slam.cpp:48-57). */
int cape_create(const cape_config* cfg, cape_handle* out);
void cape_destroy(cape_handle h);
int cape_get_layout(cape_handle h, cape_layout* out);

/*
 * Replaces, for a batch of frames: get_organized_cloud_array (depth_map_transformation.hpp:36-39) followed by
 * find_primitives (primitive_detection.hpp:41-44).  `depth_dev` is a DEVICE pointer to n_frames row-major
 * float32 images in millimetres (0 = invalid), already resident in HBM, 16-byte aligned.  Asynchronous on `stream`.
 * Results stay on the device until fetched (cape_copy_results) or gathered (cape_device_results).
 */
int cape_extract(cape_handle h, const float* depth_dev, int32_t n_frames, void* stream);

/* Same path fed with the raw 16-bit sensor image (what the depth PNGs of the TUM / CAPE datasets hold): the device
 * converts exactly like the reference's host-side cv::Mat::convertTo(CV_32F, scale) (examples/main_TUM.cpp:221,242
 * with scale = 1/5 ; examples/main_CAPE.cpp:58-59 with scale = 1): z = float(raw) * scale, 0 = invalid.  Halves the
 * bytes read per frame ("next" row N4 of SURVEY.md 8f). */
int cape_extract_u16(cape_handle h, const uint16_t* depth_dev, float scale, int32_t n_frames, void* stream);

/* "Next" row N3: Depth_Map_Transformation::rectify_depth (depth_map_transformation.hpp:29, .cpp:23-87) for a batch --
 * registers the depth camera's image to the colour camera.  `cam2_to_cam1` is the row-major 4x4 matrix
 * Parameters::get_camera_2_to_camera_1_transformation() (host pointer, 16 doubles; the last row is ignored).  Both
 * images are device pointers, n_frames x H x W float32, not in place.  Collisions keep the last source pixel in
 * row-major order, which is what the reference's MAKE_DETERMINISTIC loop does.  The intrinsics are the handle's
 * (the reference also uses camera 1's for both directions, depth_map_transformation.cpp:156 / point_coordinates.cpp:90). */
int cape_rectify_depth(cape_handle h, const float* depth_dev, float* rectified_dev, int32_t n_frames,
                       const double* cam2_to_cam1, void* stream);

/* Same with host images (H2D copy, rectify, D2H copy, synchronous): the host boundary of the reference signature. */
int cape_rectify_depth_host(cape_handle h, const float* depth_host, float* rectified_host, int32_t n_frames,
                            const double* cam2_to_cam1);

/* "Next" row N2, device part: a cell-mask pre-filter for MapPlane::find_matches
 * (src/map_management/map_features/map_primitive.cpp:91-161) between CONSECUTIVE frames of the last cape_extract batch.
 * For frame f >= 1 the planes of frame f-1 play the map planes ("projected" with the identity pose) and the planes of
 * frame f the detected ones; plane i = i-th segment with is_output, its mask = the cells whose label belongs to its
 * merge group (the mask add_planes_to_primitives builds, primitive_detection.cpp:586-594).  Areas are counted in
 * cells instead of polygon mm^2; everything else follows the reference: |d_i - d_j| < 100 mm and |n_i . n_j| >
 * |cos 20 deg| (shape_primitives.cpp:70-86), inter > best so far and inter / area(detected) >= 0.4f (0.2 with
 * CAPE_MATCH_ADVANCED), previous planes visited in order with the is-matched flags updated between them
 * (feature_map.hpp:651-669), and the `selectedIndex <= 0` quirk that never returns detected plane 0
 * (map_primitive.cpp:146) unless CAPE_MATCH_ALLOW_INDEX0 is set.  Frame 0 of a batch has no predecessor (n_prev = 0).
 * A frame that continues in spill records (more than 64 plane segments) takes part with the planes of its FIRST record only: this
 * pre-filter has no reference counterpart and its tables hold 64 planes; the polygon matcher below flags such a frame instead. */
enum
{
    CAPE_MATCH_ADVANCED = 1u << 0,
    CAPE_MATCH_ALLOW_INDEX0 = 1u << 1
};
typedef struct cape_frame_match
{
    int32_t n_prev;                      /* planes of frame f-1 */
    int32_t n_cur;                       /* planes of frame f */
    int32_t match[CAPE_MAX_PLANES];      /* per previous plane j: matched plane of this frame, or -1 */
    uint16_t area_prev[CAPE_MAX_PLANES]; /* cells */
    uint16_t area_cur[CAPE_MAX_PLANES];
    uint16_t inter[CAPE_MAX_PLANES][CAPE_MAX_PLANES]; /* inter[j][i]: cells shared by previous plane j and plane i */
} cape_frame_match;
/* Asynchronous on `stream`; reads the device results of the last cape_extract (n_frames <= that batch). */
int cape_match_consecutive(cape_handle h, int32_t n_frames, uint32_t flags, void* stream);
/* Device pointer to / synchronous copy of the n_frames x cape_frame_match written by cape_match_consecutive. */
int cape_device_matches(cape_handle h, void** matches);
int cape_copy_matches(cape_handle h, int32_t n_frames, cape_frame_match* out);

/* "Next" row N1 on the device: the boundary polygon of every output plane of the last cape_extract batch -- what the
 * reference builds on the host right after the boundary candidates, `utils::Polygon(points, normal, center)`
 * (primitive_detection.cpp:622 -> src/utils/polygon.cpp:168-229: plane frame :74-115, projection :125-144, concave hull
 * :283-318 with the convex hull :268-281 as fallback, area :453-461, simplify :578-601), one wavefront per plane.
 * A polygon is a ring of 2-D vertices in the plane frame (x_axis, y_axis, center), clockwise, first vertex not repeated:
 * exactly the arguments of the reference's Polygon(ring, xAxis, yAxis, center) constructor (polygon.cpp:236-266), which is
 * how the overlay turns a record into a CameraPolygon without running a hull on the host.  The vertices are bit-identical
 * to this repo's host class (rgb-d-slam_amd/host/boundary_polygon.cpp; the reference's own vertices are not reproducible:
 * FLANN's randomized kd-trees over a nondeterministically ordered point list). */
enum
{
    CAPE_POLY_VALID = 1u << 0,           /* simple ring of >= 3 vertices: Primitive_Detection keeps the plane (:623-631) */
    CAPE_POLY_CONVEX_FALLBACK = 1u << 1, /* no concave hull on the k ladder: compute_convex_hull was used */
    CAPE_POLY_SIMPLIFIED = 1u << 2,      /* simplify() replaced the ring (area stayed above 75 %) */
    CAPE_POLY_OVERFLOW = 1u << 3,        /* more than 1024 boundary points: not built, left to the host class */
    CAPE_POLY_REJECTED = 1u << 4,        /* the host constructor would throw (fewer than 3 points / normal not unit) */
    CAPE_POLY_DISSOLVED = 1u << 5        /* the walk's hull crossed itself (the reference's Intersects misses crossings with axis-parallel
                                            edges) and was cut apart at its crossings like correct_boost_polygon.hpp does; the ring may
                                            hold vertices that are no boundary candidates (the crossing points) */
};
typedef struct cape_polygon
{
    double x_axis[3], y_axis[3]; /* get_plane_coordinate_system(segment normal) */
    double center[3];            /* Plane_Segment::get_center() = normal * (-d) (plane_coordinates.hpp:52), like primitive_detection.cpp:622 */
    double area;                 /* Polygon::_area after simplify */
    uint32_t vertex_offset;      /* first vertex in the frame's vertex array (= the segment's boundary_offset) */
    uint32_t vertex_count;
    uint32_t flags;              /* CAPE_POLY_* ; 0 for a segment that is not an output plane */
    uint32_t segment;            /* index of the segment in the frame record */
} cape_polygon;
/* Builds the polygons of frames [0, n_frames) of the last cape_extract; asynchronous on `stream`. */
int cape_build_polygons(cape_handle h, int32_t n_frames, void* stream);
/* Device pointers: polygons = n_frames x CAPE_MAX_PLANES cape_polygon (indexed by segment), vertices = n_frames x
 * boundary_capacity x 2 doubles.  Valid until the next cape_build_polygons / destroy.  CAPE_ERR_CAPACITY when no
 * cape_build_polygons has run since the last cape_extract (the arrays would describe the PREVIOUS batch); the copy calls
 * below likewise refuse more frames than the last cape_build_polygons / cape_match_polygons of the current batch covered. */
int cape_device_polygons(cape_handle h, cape_polygon** polygons, double** vertices);
/* Synchronous D2H copy of both arrays (either pointer may be NULL). */
int cape_copy_polygons(cape_handle h, int32_t n_frames, cape_polygon* polygons, double* vertices);

/* Debug / parity: the device polygon of an arbitrary point set (host pointers; n <= boundary_capacity points x 3 doubles,
 * unit normal, centre) -- one launch of the same kernel over a one-plane record.  `vertices_out` takes up to n x 2 doubles.
 * Synchronous; does not disturb the results of the last cape_extract. */
int cape_debug_polygon(cape_handle h, const double* points3, int32_t n, const double* normal, const double* center,
                       cape_polygon* polygon_out, double* vertices_out);

/* Row N2 with the reference's own area measure: the selection of MapPlane::find_matches (map_primitive.cpp:91-161) between
 * consecutive frames on the boundary polygons of cape_build_polygons -- `detectedPolygon.inter_area(projectedPolygon)` in mm^2
 * (map_primitive.cpp:137; the previous frame's polygon projected into the detected plane's frame, Polygon::project,
 * polygon.cpp:338-382) divided by the detected polygon's area -- instead of the shared cells cape_match_consecutive counts.
 * Plane indices count the planes Primitive_Detection KEEPS (output plane with a valid polygon of >= 3 vertices,
 * primitive_detection.cpp:623-631), i.e. the indices of the reference's plane_container.  Needs cape_build_polygons of the
 * same batch first.  The areas are bit-identical to this repo's host class (Polygon::inter_area). */
#define CAPE_MATCH_MAX_PLANES 16
enum
{
    CAPE_MATCH_EXACT_OVERFLOW = 1u << 0 /* more than 16 kept planes in one of the two frames, a frame that continues in spill records
                                           (cape_frame_header.next_record), an output plane of either frame
                                           whose polygon was left to the host class (CAPE_POLY_OVERFLOW: the host may keep it,
                                           so the kept-plane indices are not known here), or a polygon pair beyond the
                                           kernel's capacities (512 vertices per ring, 2 048 slab boundaries, 32 edges of a
                                           ring over one slab): no match is reported for the frame -- use the host class */
    ,
    CAPE_MATCH_EXACT_HOST = 1u << 1     /* never set by the library: the C++ overlay marks the entries its host class computed (frame
                                           pairs across a chunk / shard boundary, frames the device flagged); match[] is filled,
                                           seg_prev / seg_cur / inter_area are not */
    ,
    CAPE_MATCH_EXACT_BAD_SHARD = 1u << 3 /* cape_match_map_shards only, next to CAPE_MATCH_EXACT_OVERFLOW: the shard's header or the frame's
                                           indices do not fit the layout the caller gave; nothing of it was read (bit 2 is taken by the
                                           INPUT flag CAPE_MATCH_MAP_AREAS) */
};
typedef struct cape_frame_match_exact
{
    int32_t n_prev, n_cur;                    /* kept planes of frame f-1 / f */
    int32_t match[CAPE_MATCH_MAX_PLANES];     /* per previous plane j: matched plane of this frame, or -1 */
    int32_t seg_prev[CAPE_MATCH_MAX_PLANES];  /* segment index of previous plane j (-1 beyond n_prev) */
    int32_t seg_cur[CAPE_MATCH_MAX_PLANES];
    uint32_t flags;                           /* CAPE_MATCH_EXACT_* */
    uint32_t pad;
    double inter_area[CAPE_MATCH_MAX_PLANES][CAPE_MATCH_MAX_PLANES]; /* [j][i] mm^2 ; -1 where the distance / normal gates
                                                 failed (the reference does not intersect those), NaN: capacity exceeded */
} cape_frame_match_exact;
/* flags: CAPE_MATCH_ADVANCED, CAPE_MATCH_ALLOW_INDEX0 as for cape_match_consecutive.  Asynchronous on `stream`. */
int cape_match_polygons(cape_handle h, int32_t n_frames, uint32_t flags, void* stream);
/* The same with the camera motion between consecutive frames -- what the reference does before its gates: the map plane goes
 * through PlaneWorldCoordinates::to_camera_coordinates (map_primitive.cpp:100-101, plane_coordinates.cpp:20-24 with the plane
 * matrix of camera_transformation.cpp:53-71) and its polygon through WorldPolygon::to_camera_space (map_primitive.cpp:103,
 * polygon_coordinates.cpp:135-165) with `worldToCamera`.  Here the map is frame f-1: prev_to_cur = n_frames x 16 doubles in
 * HOST memory (read before the call returns), row-major 4x4 [R t; 0 0 0 1], entry f taking a point of camera f-1's frame into
 * camera f's; entry 0 is not read.  NULL = the identity = cape_match_polygons (a static camera). */
int cape_match_polygons_pose(cape_handle h, int32_t n_frames, const double* prev_to_cur, uint32_t flags, void* stream);
int cape_copy_polygon_matches(cape_handle h, int32_t n_frames, cape_frame_match_exact* out);

/* cape_match_polygons_pose without its two limits: frames of up to 128 kept planes, counted in record order over the frame's whole
 * record chain (cape_frame_header.next_record), with result buffers of its own -- cape_match_polygons and its results are not
 * touched.  Per pair and per frame the statements are cape_match_polygons_pose's: the pose on the previous plane and its polygon,
 * the gates, Polygon::project into the detected plane's frame, the slab intersection, the overlap threshold, the lowest index on a
 * tie, the `selectedIndex <= 0` quirk and the is-matched flags carried from previous plane j to j + 1; a frame both calls serve
 * gets the same matches and bit-identical areas from either.  prev_to_cur as for cape_match_polygons_pose (n_frames x 16 doubles in
 * HOST memory, read before the call returns, entry 0 not read, NULL = identity).  flags: CAPE_MATCH_ADVANCED,
 * CAPE_MATCH_ALLOW_INDEX0, CAPE_MATCH_MAP_AREAS, which keeps the dense area table (CAPE_ERR_CAPACITY if it would exceed 1 GiB), and
 * CAPE_MATCH_CARRY (below: frame 0's predecessor is the handle's carried frame, and entry 0 is read).
 * A frame is flagged CAPE_MATCH_EXACT_OVERFLOW, with all its matches -1, only if it or its predecessor keeps more than 128 planes,
 * an output plane of either chain has CAPE_POLY_OVERFLOW, a pair is beyond the largest intersection tier, or the frame's pairs do
 * not fit the work list (4 194 304 gated pairs per call): cape_host_match_planes (host/cape_host_map.h) answers for it.  Needs
 * cape_build_polygons of the same batch first.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, negative n_frames, unknown flag;
 * CAPE_ERR_CAPACITY: more frames than the last cape_build_polygons covered, the area table beyond 1 GiB.  Asynchronous on `stream`. */
#define CAPE_MATCH_WIDE_MAX_PLANES 128
typedef struct cape_frame_match_wide
{
    int32_t n_prev, n_cur;   /* kept planes of frame f-1 / f over their whole record chains */
    uint32_t flags;          /* CAPE_MATCH_EXACT_OVERFLOW */
    int32_t n_matched;
} cape_frame_match_wide;
int cape_match_polygons_wide(cape_handle h, int32_t n_frames, const double* prev_to_cur, uint32_t flags, void* stream);
/* Synchronous copy of the last cape_match_polygons_wide, row-major with 128 entries per frame: match[f][j] = the kept plane of frame
 * f taken by previous kept plane j, or -1; seg_prev[f][j] / seg_cur[f][i] = the plane's position in its frame's concatenated segment
 * list (the chain's records one after the other), -1 beyond the count; inter_area[f][j][i] in mm^2, -1 for an ungated pair, NaN for
 * a pair beyond capacity (the call must have had CAPE_MATCH_MAP_AREAS).  Any of the four arrays may be NULL.  CAPE_ERR_CAPACITY:
 * more frames than that call covered. */
int cape_copy_polygon_matches_wide(cape_handle h, int32_t n_frames, cape_frame_match_wide* frames, int32_t* match, int32_t* seg_prev,
                                   int32_t* seg_cur, double* inter_area);

/* The CARRIED FRAME of a handle: a compact, handle-owned device copy of what cape_match_polygons_wide reads of ONE frame when that
 * frame plays the previous frame, so that a depth stream cut into batches (or served one frame per call on a one-frame handle) loses
 * no frame pair at the cuts.  With CAPE_MATCH_CARRY the predecessor of frame 0 is the carried frame: prev_to_cur entry 0 IS read (it
 * takes the carried frame's camera into frame 0's; NULL is still the identity for every frame), and frame 0 reports n_prev,
 * seg_prev[0][j] (the position in the carried frame's segment list), match[0][j] and inter_area[0][j][i] exactly as it would as
 * frame k of a batch that held both frames -- gates, to_camera_space and project, tiers, selection, the `selectedIndex <= 0` quirk
 * and the is-matched flags are the same statements.  The carry is read, not consumed.  CAPE_ERR_CAPACITY when no frame is carried.
 * Only cape_match_polygons_wide takes the bit: the 16-plane calls and the map matchers reject it as an unknown flag, and a pair whose
 * frames live on different handles (a shard boundary) stays with cape_host_match_planes.
 *
 * Order of use for a stream: cape_extract -> cape_build_polygons -> cape_match_polygons_wide(CAPE_MATCH_CARRY) ->
 * cape_match_carry_save(last frame) -> the next batch; the handle's one-stream rule orders the save behind the match and ahead of
 * the next cape_extract. */
enum
{
    CAPE_MATCH_CARRY = 1u << 5 /* cape_match_polygons_wide only */
};
typedef struct cape_match_carry_info_t
{
    int32_t valid;      /* 1: a frame is carried */
    int32_t n_kept;     /* its kept planes over the whole record chain (the TRUE count, may exceed 128) */
    uint32_t flags;     /* CAPE_MATCH_EXACT_OVERFLOW: more than 128 kept planes or an output plane with CAPE_POLY_OVERFLOW -- the frame
                           that follows it is flagged, cape_host_match_planes answers */
    int32_t n_vertices; /* ring vertices held (0 for a flagged carry: its rings are never read) */
} cape_match_carry_info_t;
/* Copies the kept planes of frame `frame` of the last cape_build_polygons, in kept-plane order over the frame's whole record chain:
 * per kept plane out_normal and d, its position in the frame's concatenated segment list, its cape_polygon and its ring -- into
 * buffers no other call writes, allocated on the first save.  The copy survives any later call on the handle (cape_extract,
 * cape_build_polygons, any matcher) until the next save, cape_match_carry_clear or cape_destroy.  A frame that keeps more than 128
 * planes, or has an output plane with CAPE_POLY_OVERFLOW, is carried as flagged: n_kept is the true count and the first 128 segment
 * positions are kept, which is what the matcher keeps of such a predecessor inside a batch.
 * The vertex store holds 128 x min(1024, boundary_capacity) vertices (16 bytes each, 2 MiB at most): at most 128 planes are carried,
 * and a served ring has at most min(1024, boundary_capacity) vertices -- they are boundary points of its record's slab, and a plane of
 * more than 1 024 boundary points is CAPE_POLY_OVERFLOW and has no ring.  No frame the matcher would serve is refused.
 * Asynchronous on `stream`.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, negative frame; CAPE_ERR_CAPACITY: `frame` is not covered by
 * the last cape_build_polygons of the current batch (the rule of cape_device_polygons). */
int cape_match_carry_save(cape_handle h, int32_t frame, void* stream);
/* Forgets the carried frame (the buffers stay allocated). */
int cape_match_carry_clear(cape_handle h);
/* Synchronous: waits for the handle's work and describes the carried frame (all zero when none is carried). */
int cape_match_carry_info(cape_handle h, cape_match_carry_info_t* out);

/* Row N2 against a persistent MAP (Feature_Map::get_matches, feature_map.hpp:638-697): which detected plane of each frame
 * belongs to which map plane.  The map planes live in world coordinates; their boundary polygons (grown over many frames by
 * merge_union, so they may be large and have holes) stay on the device from cape_map_upload until the next upload or destroy.
 * The map is ONE ordered list: the local map's planes first, then the staged map's, sharing one is-matched vector. */
#define CAPE_MAP_MAX_PLANES 1024 /* map planes per upload */
#define CAPE_MAP_MAX_RING 512    /* vertices of one map ring (the largest capacity tier of the intersection kernel) */
#define CAPE_MAP_MAX_HOLES 8     /* interior rings per map plane */
typedef struct cape_map_ring
{
    uint32_t vertex_offset, vertex_count; /* into the upload's vertex array (pairs of doubles), open ring (no repeated closing vertex) */
} cape_map_ring;
typedef struct cape_map_plane
{
    double normal[3], d;                    /* PlaneWorldCoordinates: unit normal, d in mm */
    double x_axis[3], y_axis[3], center[3]; /* the WorldPolygon's frame (unit axes) */
    uint32_t ring_first, ring_count;        /* rings[ring_first] = outer ring, the next ring_count - 1 = holes, in order */
} cape_map_plane;
typedef struct cape_frame_map_match
{
    int32_t n_map, n_cur;                 /* map planes of the call / kept planes of the frame */
    uint32_t flags;                       /* CAPE_MATCH_EXACT_OVERFLOW: no match is reported for the frame, use the host class
                                             (+ CAPE_MATCH_EXACT_BAD_SHARD from cape_match_map_shards) */
    int32_t n_matched;                    /* map planes that took a plane of this frame */
    int32_t seg_cur[CAPE_MAX_PLANES];     /* segment index of kept plane i, -1 beyond n_cur */
    int32_t map_of[CAPE_MAX_PLANES];      /* map plane that took kept plane i, or -1 */
} cape_frame_map_match;
enum
{
    CAPE_MATCH_MAP_AREAS = 1u << 2 /* cape_match_map: also keep the dense inter-area table (tests, diagnostics) */
};
/* Copies the map to the device (host pointers; synchronous).  planes: n_planes entries; rings: n_rings; vertices: n_vertices
 * (x, y) pairs in the planes' own frames.  The rings are re-oriented like the host class does (outer ring clockwise, holes
 * counter-clockwise).  Waits for a cape_match_map still running on the previous map.  CAPE_ERR_INVALID_ARGUMENT: a ring of
 * fewer than 3 vertices, an offset outside the arrays, ring_count == 0, a normal or axis whose norm is not 1 within DBL_EPSILON
 * (what to_camera_space requires); CAPE_ERR_CAPACITY: beyond CAPE_MAP_MAX_* (simplify the polygon first).  n_planes == 0 is an
 * empty map. */
int cape_map_upload(cape_handle h, const cape_map_plane* planes, int32_t n_planes, const cape_map_ring* rings, int32_t n_rings,
                    const double* vertices, int64_t n_vertices);
/* MapPlane::find_matches (map_primitive.cpp:91-161) for map planes j = 0 .. n_map-1 in order against the kept planes of frames
 * [0, n_frames) of the last cape_build_polygons (all kept planes of the frame's first record, up to CAPE_MAX_PLANES).  Per frame f:
 * the map plane goes through plane_to_camera and its polygon (holes included) through to_camera_space with
 * world_to_camera[f] (n_frames x 16 doubles in HOST memory, read before the call returns, row-major [R t; 0 0 0 1]; NULL =
 * identity); a projected area <= 0 matches nothing; the gates |delta d| < 100 mm, |cos| > cos 20 deg come before any
 * intersection; inter = I(detected, outer) - I(detected, hole_k) in order, clamped at 0; the greatest inter with
 * inter / area(detected) >= 0.4f (halved with CAPE_MATCH_ADVANCED) wins, the lowest index on a tie, the `selectedIndex <= 0`
 * quirk unless CAPE_MATCH_ALLOW_INDEX0, and a detected plane taken by map plane j is skipped by j+1 ...
 * skip: NULL or n_frames x ceil(n_map / 32) words in HOST memory; bit j of frame f set = map plane j is not visited (the caller's
 * `is_moving() or not is_visible(worldToCamera)`, feature_map.hpp:658, :683).  A frame is flagged CAPE_MATCH_EXACT_OVERFLOW
 * (no match reported) if it continues in spill records, one of its output planes has CAPE_POLY_OVERFLOW, a pair exceeds the
 * intersection kernel's capacities or its pairs do not fit the work list.  flags: CAPE_MATCH_ADVANCED, CAPE_MATCH_ALLOW_INDEX0,
 * CAPE_MATCH_MAP_AREAS (CAPE_ERR_CAPACITY if the table would exceed 1 GiB).  Asynchronous on `stream`. */
int cape_match_map(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, uint32_t flags, void* stream);
/* Synchronous copy of the last cape_match_map: frames (n_frames entries), match (n_frames x n_map, n_map being the map size of
 * that cape_match_map call -- not of a map uploaded since: detected kept-plane index matched to map plane j, or -1) and, if the call
 * kept it, inter_area (n_frames x n_map x CAPE_MAX_PLANES doubles, [f][j][i]
 * mm^2; -1 where the pair was not gated or the map plane was skipped / has no positive projected area, NaN: capacity).  Either
 * of match / inter_area may be NULL.  Refuses more frames than the last cape_match_map covered. */
int cape_copy_map_matches(cape_handle h, int32_t n_frames, cape_frame_map_match* frames, int32_t* match, double* inter_area);

/* cape_match_map without its limit on the frame: the detected planes are the frame's kept planes in record order over its whole
 * record chain (cape_frame_header.next_record), up to 128 -- the frames of more than 64 plane segments the general grow instance
 * leaves in spill records, which cape_match_map flags.  Per pair and per frame the statements are cape_match_map's
 * (MapPlane::find_matches, map_primitive.cpp:91-161, for map planes j = 0 .. n_map-1 in order, feature_map.hpp:638-697):
 * plane_to_camera (plane_coordinates.cpp:20-24) and to_camera_space with holes (polygon_coordinates.cpp:135-165) through
 * world_to_camera[f]; a projected area <= 0 matches nothing (map_primitive.cpp:105-106); the gates |delta d| < 100 mm,
 * |cos| > cos 20 deg (shape_primitives.cpp:66-86) before any intersection; inter = I(detected, outer) - I(detected, hole_k) in order,
 * clamped at 0; inter / area(detected) >= 0.4f, halved with CAPE_MATCH_ADVANCED (map_primitive.cpp:137-143); the lowest index on a
 * tie; the `selectedIndex <= 0` quirk (map_primitive.cpp:146) unless CAPE_MATCH_ALLOW_INDEX0; the is-matched flags carried from map
 * plane j to j + 1.  A frame both calls serve gets the same decisions and bit-identical areas from either.
 * world_to_camera (n_frames x 16 doubles) and skip (n_frames x ceil(n_map / 32) words) as for cape_match_map: HOST memory, read
 * before the call returns, NULL = identity / none skipped.  flags: CAPE_MATCH_ADVANCED, CAPE_MATCH_ALLOW_INDEX0,
 * CAPE_MATCH_MAP_AREAS (the dense table [f][j][i] with 128 entries per map plane; CAPE_ERR_CAPACITY if n_frames x n_map x 128 x 8
 * bytes would exceed 1 GiB) and CAPE_MATCH_MAP_DEVICE_SKIP (the words of the last cape_map_visibility; skip must be NULL).
 * A frame is flagged CAPE_MATCH_EXACT_OVERFLOW -- no match reported, n_cur the true count -- only if its chain keeps more than 128
 * planes, an output plane of the chain has CAPE_POLY_OVERFLOW, a pair exceeds the largest intersection tier, or its pairs do not fit
 * the work list (16 777 216 gated pairs per call): cape_host_match_map (host/cape_host_map.h) answers for it.
 * Needs cape_build_polygons of the same batch first.  The results live in buffers of the handle's own: cape_match_map /
 * cape_copy_map_matches and this pair do not disturb each other's results; a cape_map_upload waits for a call in flight.
 * CAPE_ERR_INVALID_ARGUMENT: NULL handle, negative n_frames, unknown flag, no map uploaded, a non-NULL skip together with
 * CAPE_MATCH_MAP_DEVICE_SKIP; CAPE_ERR_CAPACITY: more frames than the last cape_build_polygons covered, the area table beyond 1 GiB,
 * CAPE_MATCH_MAP_DEVICE_SKIP without a cape_map_visibility since the last cape_map_upload that covers n_frames.  An empty map
 * succeeds with n_matched = 0.  Asynchronous on `stream`. */
#define CAPE_MATCH_MAP_WIDE_MAX_PLANES CAPE_MATCH_WIDE_MAX_PLANES
typedef struct cape_frame_map_match_wide
{
    int32_t n_map, n_cur;    /* map planes of the call / kept planes of the frame over its whole record chain */
    uint32_t flags;          /* CAPE_MATCH_EXACT_OVERFLOW */
    int32_t n_matched;       /* map planes that took a plane of this frame */
} cape_frame_map_match_wide;
int cape_match_map_wide(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, uint32_t flags, void* stream);
/* Synchronous copy of the last cape_match_map_wide: frames (n_frames entries); match (n_frames x n_map, n_map being the map size of
 * that call -- not of a map uploaded since): the kept plane matched to map plane j, or -1; seg_cur and map_of (n_frames x 128): kept
 * plane i's position in the frame's concatenated segment list (the chain's records one after the other) and the map plane that took
 * it, both -1 beyond n_cur; inter_area (n_frames x n_map x 128, [f][j][i] mm^2; -1 where the pair was not gated or the map plane was
 * skipped / has no positive projected area, NaN: capacity; the call must have had CAPE_MATCH_MAP_AREAS, else
 * CAPE_ERR_INVALID_ARGUMENT).  Any array may be NULL.  CAPE_ERR_CAPACITY: more frames than that call covered. */
int cape_copy_map_matches_wide(cape_handle h, int32_t n_frames, cape_frame_map_match_wide* frames, int32_t* match, int32_t* seg_cur,
                               int32_t* map_of, double* inter_area);

/* cape_match_map for the frames of GATHERED SHARDS: what the rank that owns the map does with the world x bytes_per_rank bytes a
 * gather left in its device memory, without a host read of them.  shards_dev: n_shards shards of layout->bytes_per_rank bytes, rank
 * after rank, packed with CAPE_GATHER_POLYGONS -- the recv_dev of cape_gather_primitives[_root], or the slot cape_pack_primitives
 * returns (n_shards = 1); 16-byte aligned.  layout / polygon_layout: what cape_gather_configure_polygons reported on the PRODUCERS;
 * this handle needs no gather configuration of its own, need never have run cape_extract and may have any max_batch: the call uses
 * the map of cape_map_upload and nothing else of the handle.
 * Results, world_to_camera (n_slots x 16 doubles) and skip (n_slots x ceil(n_map / 32) words; both HOST memory, read before the call
 * returns, NULL as for cape_match_map) are indexed by SLOT s = shard x frames_capacity + k, n_slots = n_shards x frames_capacity:
 * how many frames a shard holds is known on the device only.  A slot with k >= the shard's n_frames is EMPTY: n_map set, n_cur = 0,
 * n_matched = 0, flags = 0, its match row all -1.
 * Per served slot the semantics are cape_match_map's (gates, projected-area rule, tiers, selection, flags, CAPE_MATCH_MAP_AREAS with
 * its 1 GiB cap).  Kept plane i of a frame is the i-th of its packed planes whose packed polygon has CAPE_POLY_VALID and >= 3
 * vertices; seg_cur[i] is that plane's cape_packed_plane.segment, the index in the FRAME's segment list (>= 64 in a frame that
 * continued in spill records on its producer: the packed lists follow the chain, so such a frame is served here whenever it keeps at
 * most 64 planes).  A slot is flagged CAPE_MATCH_EXACT_OVERFLOW, and reports no match, when its frame keeps more than 64 planes,
 * holds a polygon with CAPE_POLY_OVERFLOW, has planes beyond planes_capacity (CAPE_PACKED_PLANES_DROPPED) or a polygon whose ring
 * did not travel (vertex_offset == UINT32_MAX: with vertex_count = 0 the kept rule cannot be evaluated), or exceeds the intersection
 * capacities / the work list as in cape_match_map.  The frames of a shard that dropped rings which lie wholly before the first
 * dropped ring are served -- cape_host_shard_frame (host/cape_host_map.h), the answer for a flagged slot, refuses that whole shard.
 * The shard bytes come from another process: every index read from a shard is checked against its section before it is used and
 * the kernels never read outside n_shards x bytes_per_rank.  All slots of a shard are flagged CAPE_MATCH_EXACT_BAD_SHARD |
 * CAPE_MATCH_EXACT_OVERFLOW, and nothing beyond the header is read, when its header has a wrong magic, no CAPE_GATHER_POLYGONS,
 * frames_capacity / planes_capacity / cells or the polygon header's vertices_capacity other than the layouts', or n_frames outside
 * [0, frames_capacity]; one frame is flagged the same way, and not read, when its plane_offset / n_planes lie outside the plane
 * section (without the header's CAPE_PACKED_PLANES_DROPPED) or one of its rings ends beyond vertices_capacity.
 * CAPE_ERR_INVALID_ARGUMENT: a NULL handle / shards / layout, n_shards < 1, an unknown flag, no map uploaded, a layout whose
 * sections do not fit bytes_per_rank, overlap or are not 16-byte aligned; CAPE_ERR_CAPACITY: more than INT32_MAX slots, the area table beyond
 * 1 GiB.  Asynchronous on `stream`; the shard memory is the caller's and must stay untouched until that work has been waited for.
 * Behind a gather the caller orders the call with cape_gather_wait(h, stream, 0) first.
 * The results live in buffers of their own, sized by the call's slots: cape_match_map / cape_copy_map_matches and this pair do not
 * disturb each other's results, and a cape_extract does not invalidate these. */
int cape_match_map_shards(cape_handle h, const void* shards_dev, int32_t n_shards, const cape_gather_layout* layout,
                          const cape_gather_polygon_layout* polygon_layout, const double* world_to_camera, const uint32_t* skip,
                          uint32_t flags, void* stream);
/* Synchronous copy of the last cape_match_map_shards, slots [0, n_slots): the arrays of cape_copy_map_matches, indexed by slot.
 * CAPE_ERR_CAPACITY: more slots than that call covered. */
int cape_copy_shard_map_matches(cape_handle h, int32_t n_slots, cape_frame_map_match* frames, int32_t* match, double* inter_area);

/* The skip words of cape_match_map / cape_match_map_shards, decided on the device: bit j of frame f = map plane j is not visited,
 * i.e. bit j of `moving` is set or MapPlane::is_visible(world_to_camera[f]) is false (map_primitive.cpp:186-189) -- the first
 * statement of the get_matches loop (feature_map.hpp:658, :683).  n_frames counts frames or, for cape_match_map_shards, slots; the
 * call uses the map of cape_map_upload and the handle's width, height, fx, fy, cx, cy and nothing else of the handle (no cape_extract
 * is needed, max_batch does not bound n_frames).  world_to_camera: n_frames x 16 doubles in HOST memory, read before the call
 * returns, NULL = identity; moving: ceil(n_map / 32) words in HOST memory, one bit per MAP PLANE (the caller's is_moving()), NULL =
 * none.  Per pair: the map polygon goes through to_camera_space as in cape_match_map, every vertex (a, b) of its OUTER ring (holes
 * are not read, as in to_screen_space) becomes the camera point centre + a xAxis + b yAxis and the screen point
 * u = (1 / Z) (fx X + cx Z), v = (1 / Z) (fy Y + cy Z); the plane is visible when the ring intersection of the matchers gives
 * area(screen ring n rectangle (1, 1) .. (W-1, H-1)) > 0, both rings oriented like the host class orients an outer ring.  Stated
 * differences to the reference: a ring with a NaN or INFINITE screen coordinate is not visible (the reference drops NaN only and hands
 * Boost an invalid polygon on infinity); a ring with vertices behind the camera goes through the same statements without clipping
 * (the reference has a TODO there) and the answer is cape_host_map_visibility's (host/cape_host_map.h), not Boost's; a pair beyond
 * the intersection kernel's capacities is not decided and counts as VISIBLE.  The words are the host twin's bit for bit.
 * They live in a buffer of the handle's own that no other call writes; a cape_map_upload discards them (and waits for a call in
 * flight).  Asynchronous on `stream`.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, n_frames < 1, no map uploaded; CAPE_ERR_CAPACITY:
 * n_frames x n_map work-list entries would exceed 1 GiB.  An empty map succeeds and writes nothing. */
int cape_map_visibility(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* moving, void* stream);
/* Synchronous copy of the last cape_map_visibility: skip_out (n_frames x ceil(n_map / 32) words; the bits beyond n_map in a frame's
 * last word are 0) and n_undecided (pairs of that call that exceeded the capacities and count as visible); either may be NULL.
 * CAPE_ERR_CAPACITY: more frames than that call covered, or none since the last cape_map_upload. */
int cape_copy_map_visibility(cape_handle h, int32_t n_frames, uint32_t* skip_out, int64_t* n_undecided);
enum
{
    CAPE_MATCH_MAP_DEVICE_SKIP = 1u << 4 /* cape_match_map / cape_match_map_shards: the skip words are those of the last
                                            cape_map_visibility (frame or slot f of this call = frame f of that one; the poses are
                                            still passed to this call).  `skip` must be NULL (CAPE_ERR_INVALID_ARGUMENT);
                                            CAPE_ERR_CAPACITY if no cape_map_visibility has run since the last cape_map_upload or it
                                            covered fewer frames / slots than this call */
};

/* The MEASUREMENT half of the map update on the device: what MapPlane::update_with_match computes of a matched detection before
 * its Kalman step, and the StagedMapPlane constructor of an unmatched one (host: cape_host_map_update, host/polygon_capi.cpp) --
 * per kept plane of frames [0, n_frames) of the last cape_build_polygons, over each frame's whole record chain and without a limit
 * on the planes of a frame: plane_covariance of the detection (out_normal, d, the segment's cov), world_plane_covariance with the
 * frame's pose T = camera_to_world[f] and pose covariance S = pose_covariance[f], the plane in world coordinates (plane_to_world),
 * the polygon's frame and ring in world space (to_world_space's checks, then to_camera_space with T).  It reads neither the map nor
 * a match and changes neither: the Kalman step and the counters are cape_map_kalman's (below), merge_union stays with cape_host_map_update.
 * A segment is a kept plane when it is an output plane whose polygon has CAPE_POLY_VALID and >= 3 vertices (a CAPE_POLY_OVERFLOW
 * polygon is not kept; the frame's other planes are served).  The rows are indexed like the polygon rows, [record][segment], the
 * batch's records followed by the spill pool's; the world ring of a kept plane lies in the record's world-vertex slab at the
 * cape_polygon's vertex_offset / vertex_count.  A row whose segment is not kept is all zero.  For a kept plane that fails a step,
 * the flags name the first failing step and the fields that step and the later ones would have produced are 0 (its ring too).
 * The world plane, the polygon frame and the ring are the host twin's bit for bit; the two covariances pass through pow(s, 3 / 2)
 * (ocml's on the device, the C library's on the host) and agree to rounding (1e-12 relative in the tests). */
enum
{
    CAPE_MEASURE_KEPT = 1u << 0,           /* the segment is a kept plane: the row is filled */
    CAPE_MEASURE_STAGEABLE = 1u << 1,      /* every check passed and the ring has <= CAPE_MAP_MAX_RING vertices: cape_host_map_update
                                              with CAPE_MAP_ADD_STAGED would append it */
    CAPE_MEASURE_FAIL_PLANE_COV = 1u << 2, /* plane_covariance of the detection is false */
    CAPE_MEASURE_FAIL_WORLD_COV = 1u << 3, /* world_plane_covariance is false */
    CAPE_MEASURE_FAIL_POLYGON = 1u << 4,   /* to_world_space's checks, or staged_normal not unit */
    CAPE_MEASURE_RING_TOO_LONG = 1u << 5,  /* more than CAPE_MAP_MAX_RING vertices: a measurement, not a map plane */
    CAPE_MEASURE_BAD_POSE_COV = 1u << 6    /* the frame's pose covariance is not valid */
};
typedef struct cape_plane_measurement
{
    double normal[3], d;                    /* world plane = z of the Kalman step */
    double staged_normal[3];                /* normal through one more normalisation: the staged plane's */
    double covariance[16];                  /* world plane covariance, row-major = R of the Kalman step / the staged plane's covariance */
    double x_axis[3], y_axis[3], center[3]; /* the world polygon's frame; its ring: the record's world-vertex slab at the
                                               cape_polygon's vertex_offset / vertex_count */
    uint32_t vertex_offset, vertex_count;   /* ... repeated here once the polygon step has passed (0 otherwise), so that the rows and
                                               the world-vertex slabs can be read without the polygon rows */
    uint32_t flags, pad;
} cape_plane_measurement;                   /* 32 doubles + 16 bytes = 272 bytes */
/* camera_to_world: n_frames x 16 doubles in HOST memory (row-major [R t; 0 0 0 1]), read before the call returns, NULL = identity;
 * pose_covariance: n_frames x 9 doubles in HOST memory, required (the zero matrix is not a valid covariance).  A frame whose pose
 * covariance is not valid (is_covariance_valid, as cape_host_map_update refuses it) has CAPE_MEASURE_KEPT | CAPE_MEASURE_BAD_POSE_COV
 * on every kept plane and nothing else.  Needs cape_build_polygons of the same batch and no map.  Asynchronous on `stream`.  The
 * results live in buffers of the handle's own (allocated on the first call) that no other call writes; a later cape_extract or
 * cape_build_polygons invalidates them.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, negative n_frames, NULL pose_covariance;
 * CAPE_ERR_CAPACITY: more frames than the last cape_build_polygons of the current batch covered. */
int cape_map_measure(cape_handle h, int32_t n_frames, const double* camera_to_world, const double* pose_covariance, void* stream);
/* Device pointers: rows = (max_batch + spill records) x CAPE_MAX_PLANES cape_plane_measurement, world_vertices = as many slabs of
 * boundary_capacity x 2 doubles.  Either may be NULL.  CAPE_ERR_CAPACITY when no cape_map_measure has run on the current batch. */
int cape_device_map_measurements(cape_handle h, cape_plane_measurement** rows, double** world_vertices);
/* Synchronous copies, like cape_copy_polygons and cape_copy_spill_polygons (either pointer may be NULL): the rows and slabs of
 * frames [0, n_frames) -- CAPE_ERR_CAPACITY beyond what the last cape_map_measure of the current batch covered -- and of spill
 * records [first, first + count) -- CAPE_ERR_CAPACITY when no cape_map_measure has run on the current batch. */
int cape_copy_map_measurements(cape_handle h, int32_t n_frames, cape_plane_measurement* rows, double* world_vertices);
int cape_copy_spill_measurements(cape_handle h, int32_t first, int32_t count, cape_plane_measurement* rows, double* world_vertices);

/* Tracking state of one map plane, parallel to cape_map_plane: what Feature_Map::update_map (feature_map.hpp:367-384, :701-830)
 * reads and changes besides the plane and its polygon.  Promotion from staged to local, removal from staged and the loss of a local
 * plane reorder or delete entries of the ordered list: cape_host_map_update (host/cape_host_map.h) and cape_map_kalman report them
 * in `result` and leave them to the caller; cape_map_maintain (below) executes them on the device map. */
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
    CAPE_MAP_TRACK_MOVING = 1u << 1  /* is_moving(): cape_map_step_visible skips the plane; every other matcher takes the caller's skip bits */
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

/* The STATE half of the map update on the device, up to but not including the polygon union: per frame f of [0, n_frames) -- every
 * frame against the uploaded map and the uploaded tracks, independently of the other frames, like cape_match_map_wide -- and per map
 * plane j, the statements of cape_host_map_update (host/polygon_capi.cpp) that concern the plane's state, on the match of the last
 * cape_match_map_wide and the rows of the last cape_map_measure.  Nothing is written into the map, the tracks, the matches or the
 * measurements.  For a matched pair (j, i = match[f][j] >= 0), in the host's order and with its early exits:
 *   CAPE_MAP_RESULT_MATCHED;
 *   FAIL_DETECTION if kept plane i's measurement row carries CAPE_MEASURE_FAIL_PLANE_COV, CAPE_MEASURE_FAIL_WORLD_COV or
 *     CAPE_MEASURE_BAD_POSE_COV (or is no kept plane's row).  The host refuses a whole frame with an invalid pose covariance; here
 *     each of its matched planes fails this way and the frame's header carries CAPE_KALMAN_BAD_POSE_COV;
 *   FAIL_STATE if is_covariance_valid of the track's covariance is false;
 *   kalman_update (host/map_tracking.cpp) with x = the map plane's (normal, d), P = the track's covariance, z, R = the row's
 *     (normal, d), covariance: FAIL_SINGULAR / FAIL_KALMAN as the host maps the status;
 *   the new normal through normalize3 three times, the new d = x'[3], the new covariance;
 *   the frame update_boundary_polygon projects into: | |n| - 1 | <= DBL_EPSILON, the axes of get_plane_coordinate_system(n) (whose
 *     own 1e-9 norm check throws on the host and fails the polygon step here), the centre n x (-d);
 *   the detection's polygon is usable iff the row lacks CAPE_MEASURE_FAIL_POLYGON -- the one rule that is coarser than
 *     to_world_space's alone (the row's bit also covers the staged normal's unit check and a ring outside its slab);
 *   with both CAPE_MAP_RESULT_UPDATED, otherwise FAIL_POLYGON; plane and covariance are the updated ones either way.
 * merge_union never decides UPDATED on the host, so the bit is set without the union: merge_union, simplify and
 * CAPE_MAP_RESULT_OVERFLOW stay with the host, which needs the fusion rows, the world rings of cape_map_measure and the map polygon
 * for them.  For every map plane, matched or not: the counters after this frame (failed_tracking = 0, ++successive_matched on
 * UPDATED, else ++failed_tracking, --successive_matched) and PROMOTE / DROP / LOST by the thresholds 4 / 2 / 10.  For every kept
 * plane: used = matched and (UPDATED or the map plane is staged).
 * Everything on this path is + - x / sqrt in the order of the host twin cape_host_map_kalman (host/cape_host_map.h), which it equals
 * bit for bit when fed the same measurement rows. */
enum
{
    CAPE_KALMAN_BAD_POSE_COV = 1u << 8 /* cape_frame_map_kalman.flags: a kept plane of the frame carries CAPE_MEASURE_BAD_POSE_COV */
};
enum
{
    CAPE_FUSION_USED = 1u << 0,  /* a map plane used this detection: an update with CAPE_MAP_ADD_STAGED does not append it */
    CAPE_FUSION_STATE = 1u << 1, /* normal, d and covariance hold the matched map plane's new state (the Kalman step passed) */
    CAPE_FUSION_FRAME = 1u << 2  /* x_axis, y_axis and center hold the frame the polygon step projects into */
};
typedef struct cape_frame_map_kalman
{
    int32_t n_map, n_cur; /* map planes of the call / kept planes of the frame (the wide match's) */
    uint32_t flags;       /* CAPE_MATCH_EXACT_OVERFLOW of the wide match: the frame reports nothing, all its rows and track results are
                             0 and cape_host_map_update answers; CAPE_KALMAN_BAD_POSE_COV */
    int32_t n_updated;    /* map planes with CAPE_MAP_RESULT_UPDATED */
} cape_frame_map_kalman;
/* One row per kept plane i < 128 of a frame, all zero beyond n_cur.  A pair that failed a step keeps zeros in the fields that step
 * and the later ones would have produced: without CAPE_FUSION_STATE normal, d, covariance and the frame are 0, without
 * CAPE_FUSION_FRAME the frame is 0.  An unmatched kept plane has map_plane = -1 and nothing else. */
typedef struct cape_plane_fusion
{
    double normal[3], d;                    /* the map plane's new parametrisation */
    double covariance[16];                  /* ... and covariance, row-major */
    double x_axis[3], y_axis[3], center[3]; /* the frame the map polygon and the detection are projected into before the union */
    int32_t map_plane;                      /* the map plane that took this kept plane, or -1 */
    uint32_t flags;                         /* CAPE_FUSION_* */
} cape_plane_fusion;                        /* 29 doubles + 8 bytes = 240 bytes */
typedef struct cape_map_track_result
{
    uint32_t result;            /* CAPE_MAP_RESULT_* without OVERFLOW and APPENDED */
    int32_t successive_matched; /* the counters after this frame */
    uint32_t failed_tracking;
    int32_t kept_plane;         /* match[f][j]: the kept plane map plane j took, or -1 */
} cape_map_track_result;
/* What cape_map_kalman reads of the tracks, parallel to the planes of the last cape_map_upload: covariance, successive_matched,
 * failed_tracking, flags; `result` and `id` are kept beside them for cape_map_commit and cape_map_download.  Host pointer, synchronous.  n must equal the uploaded map's plane count.  A cape_map_upload discards the
 * tracks (and waits for a call in flight).  CAPE_ERR_INVALID_ARGUMENT: NULL handle, no map uploaded, n other than the map's plane
 * count, NULL tracks with n > 0. */
int cape_map_upload_tracks(cape_handle h, const cape_map_track* tracks, int32_t n);
/* Needs, on the current batch and covering n_frames: a cape_match_map_wide since the last cape_map_upload, a cape_map_measure, and
 * the uploaded tracks -- otherwise CAPE_ERR_CAPACITY.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, n_frames < 0.  An empty map succeeds
 * and writes frame headers only.  Kept plane i of frame f is resolved to its measurement row through the kept-plane table the wide
 * match left on the handle; every index taken from it is checked against the row buffer before use.  Asynchronous on `stream`.  The
 * results live in buffers of the handle's own, grown on demand, that no other call writes; a later cape_extract,
 * cape_build_polygons, cape_map_upload, cape_match_map_wide or cape_map_measure invalidates them. */
int cape_map_kalman(cape_handle h, int32_t n_frames, void* stream);
/* Synchronous copy of the last cape_map_kalman: frames (n_frames entries), rows (n_frames x 128), track_results (n_frames x n_map,
 * n_map being the map size of that call).  Any pointer may be NULL.  CAPE_ERR_CAPACITY beyond what the call covered. */
int cape_copy_map_kalman(cape_handle h, int32_t n_frames, cape_frame_map_kalman* frames, cape_plane_fusion* rows,
                         cape_map_track_result* track_results);
/* Device pointers of the same arrays (rows: frames x 128; track_results: frames x n_map of the call).  Any may be NULL.
 * CAPE_ERR_CAPACITY when no cape_map_kalman has run on the current batch, map and measurements. */
int cape_device_map_kalman(cape_handle h, cape_frame_map_kalman** frames, cape_plane_fusion** rows, cape_map_track_result** track_results);

/* The POLYGON half of the map update on the device, for the case a running map consists of almost entirely: a map plane without
 * holes whose union with the detection creates no hole.  Per frame f of [0, n_frames) and per pair cape_map_kalman reports as
 * UPDATED -- the fusion row of kept plane i has map_plane = j >= 0 and CAPE_FUSION_FRAME, the measurement row has CAPE_MEASURE_KEPT and
 * lacks CAPE_MEASURE_FAIL_POLYGON, and match[j] == i -- the polygon step of cape_host_map_update (host/polygon_capi.cpp) in the host's order and with its
 * early exits: the map plane's outer ring, projected into the fusion frame unless Polygon::project's isApprox shortcut holds, the
 * detection's world ring of cape_map_measure projected into the map polygon's frame, merge_union (the arrangement of the two rings,
 * the outer face, every other face with its probe point, drop_collinear, the disjoint rule, ring_is_simple) and simplify().  Every
 * frame sees the same uploaded map and every pair is independent: nothing is written into the map, the tracks, the matches, the
 * measurements or the fusion rows.  A served ring is the host class's bit for bit (vertex coordinates are + - x / only); sqrt, hypot
 * and atan2 feed comparisons only, and an angle comparison of the face walk inside a guard band of 1e-10 rad hands the pair to the
 * host.  Everything else is reported as the host's, per pair: cape_host_map_update remains the answer for those pairs. */
#define CAPE_MAP_UNION_MAX_RING 128        /* vertices of either operand's outer ring the device serves */
#define CAPE_MAP_UNION_MAX_NODES 512       /* nodes of the arrangement of the two rings */
#define CAPE_MAP_UNION_FRAME_VERTICES 2048 /* result vertices of one frame's pairs */
enum
{
    CAPE_UNION_SERVED = 1u << 0,         /* frame, area and ring are the new map polygon's; no OVERFLOW is possible (<= 512 vertices, no hole) */
    CAPE_UNION_UNCHANGED = 1u << 1,      /* with SERVED: merge_union returned false, the ring is the PROJECTED map ring, not simplified */
    CAPE_UNION_DISJOINT = 1u << 2,       /* with SERVED: the operands are two disjoint pieces and the ring is the bigger one's -- chosen by
                                            merge_union's disjoint rule, or because the outer face walked from the leftmost node already
                                            is the bigger piece (no vertex of the other operand lies inside or on it) */
    CAPE_UNION_HOST_MAP_HOLES = 1u << 3, /* the map plane has interior rings */
    CAPE_UNION_HOST_NEW_HOLE = 1u << 4,  /* the union encloses a face merge_union would add as a hole: one or many -- more than
                                            CAPE_MAP_MAX_HOLES of them too, which the update reports as CAPE_MAP_RESULT_OVERFLOW */
    CAPE_UNION_HOST_CAPACITY = 1u << 5,  /* an operand > MAX_RING, nodes > MAX_NODES, a node of more than 8 neighbours, a walk that
                                            reaches its guard or outgrows CAPE_MAP_MAX_RING, or the frame's vertex slab is full; never
                                            the number of holes */
    CAPE_UNION_HOST_AMBIGUOUS = 1u << 6, /* an angle comparison of the face walk lies inside the guard band */
    CAPE_UNION_HOLES = 1u << 7,          /* with SERVED: the polygon has interior rings, see cape_plane_union_rings */
    CAPE_UNION_HOST_HOLE_CUT = 1u << 8,  /* a hole of the map plane is partly covered by the detection */
    CAPE_UNION_HOLE_PIECES = 1u << 9     /* with SERVED, cape_map_union_cut only: a hole of the map plane was partly covered and
                                            merge_union's `cut` branch ran -- also where every piece was then dropped */
};
/* One row per kept plane i < 128 of a frame, like the fusion rows.  A pair with a CAPE_UNION_HOST_* bit carries no ring:
 * vertex_count = 0 and area = 0.  The frame is the new map polygon's: the fusion row's, except where the isApprox shortcut kept the
 * map polygon's own frame (equal to it within 1e-12). */
typedef struct cape_plane_union
{
    double x_axis[3], y_axis[3], center[3]; /* the fusion row's frame, repeated -- or the map polygon's own frame where the isApprox
                                               shortcut kept it */
    double area;                            /* Polygon::_area after the step */
    uint32_t vertex_offset, vertex_count;   /* in the frame's slab of CAPE_MAP_UNION_FRAME_VERTICES (x, y) pairs */
    int32_t map_plane;                      /* -1: no pair for this kept plane, row otherwise zero */
    uint32_t flags;
    uint32_t n_nodes, pad;                  /* arrangement nodes of a served pair (diagnostic) */
} cape_plane_union;
/* Needs a cape_map_kalman on the current batch, map, tracks and measurements covering n_frames -- otherwise CAPE_ERR_CAPACITY.
 * CAPE_ERR_INVALID_ARGUMENT: NULL handle, n_frames < 0.  A frame the wide match flagged CAPE_MATCH_EXACT_OVERFLOW writes zeros.  The
 * wave of a frame walks its pairs in kept-plane order and appends each served ring to the frame's slab, so the offsets are
 * deterministic; a ring that does not fit the rest of the slab is CAPE_UNION_HOST_CAPACITY.  Every count read from the map, a row or
 * a table is checked against its buffer before use.  Asynchronous on `stream`.  The results live in buffers of the handle's own,
 * grown on demand, that no other call writes; whatever invalidates cape_map_kalman's results, and cape_map_kalman itself,
 * invalidates them. */
int cape_map_union(cape_handle h, int32_t n_frames, void* stream);
/* Synchronous copy of the last cape_map_union: rows (n_frames x 128), vertices (n_frames x CAPE_MAP_UNION_FRAME_VERTICES x 2
 * doubles).  Of a frame's slab only the first sum-of-vertex_count vertices are defined: the call writes the served rings back to back
 * and nothing behind them.  Either pointer may be NULL.  CAPE_ERR_CAPACITY beyond what the call covered. */
int cape_copy_map_union(cape_handle h, int32_t n_frames, cape_plane_union* rows /* n_frames x 128 */, double* vertices);
/* Device pointers of the same arrays.  Either may be NULL.  CAPE_ERR_CAPACITY when no cape_map_union has run on the current batch,
 * map, match, measurements and Kalman results. */
int cape_device_map_union(cape_handle h, cape_plane_union** rows, double** vertices);

/* The same half for a pair whose map plane HAS interior rings and / or whose union creates some: cape_map_union with the hole
 * statements of the host class restated as well (cape_map_union itself and its results are unchanged; bits 3 and 4 are never set
 * here).  Polygon::project re-projects every interior ring and add_hole orients it; every bounded face of the arrangement that lies
 * inside neither operand becomes a hole after drop_collinear if it has >= 3 vertices and is simple, in face-walk order; the disjoint
 * rule simplifies the projected map polygon WITH its holes where it is the bigger piece, and drops them where the detection is; a
 * hole of the map plane is then kept (the detection covers at most 1e-12 of the bigger operand's area of it), dropped (the detection
 * covers all of it) or -- partly covered -- hands the pair to the host as CAPE_UNION_HOST_HOLE_CUT, which wins over every capacity
 * below; simplify() takes its tolerance and its 75 % rule from the area without the holes and replaces all rings or none.  A served
 * polygon's rings lie back to back in the frame's slab from row.vertex_offset: the outer ring (row.vertex_count vertices), then the
 * interior rings in the host's order (the new ones, then the kept ones in the map's order); row.area is Polygon::_area, the outer
 * ring minus the holes; a polygon that does not fit the rest of the slab as a whole is CAPE_UNION_HOST_CAPACITY.  So is: a map plane
 * of more than 1 + CAPE_MAP_MAX_HOLES rings, an interior ring of the map plane of more than CAPE_MAP_UNION_MAX_RING vertices, more
 * than CAPE_MAP_UNION_HOLE_VERTICES vertices in the interior rings of the polygon before simplify(), more than CAPE_MAP_MAX_HOLES
 * interior rings (the update reports CAPE_MAP_RESULT_OVERFLOW and keeps the old polygon) and a hole against a detection beyond the
 * intersection's slab capacities (1024 slab boundaries, 16 edges of a ring over one slab). */
#define CAPE_MAP_UNION_HOLE_VERTICES 512 /* vertices of all interior rings of a merged polygon before simplify() */
typedef struct cape_plane_union_rings            /* 56 bytes, one per kept plane i < 128, parallel to cape_plane_union */
{
    uint32_t ring_count;                           /* 0 unless SERVED; 1 + interior rings */
    uint32_t vertex_count[1 + CAPE_MAP_MAX_HOLES]; /* ring k's vertices; the rings lie back to back from row.vertex_offset */
    uint32_t holes_new, holes_kept, holes_covered; /* what merge_union did (0 on the disjoint / unchanged paths) */
    uint32_t pad;
} cape_plane_union_rings;
/* Preconditions and error codes of cape_map_union.  Writes the same row and slab buffers -- cape_copy_map_union and
 * cape_device_map_union return them -- plus the rings table below.  A later cape_map_union overwrites the rows; the rings table is
 * then no longer current, and the two calls below return CAPE_ERR_CAPACITY, as after anything that invalidates the union results. */
int cape_map_union_holes(cape_handle h, int32_t n_frames, void* stream);
/* Synchronous copy / device pointer of the rings table of the last cape_map_union_holes (n_frames x 128). */
int cape_copy_map_union_rings(cape_handle h, int32_t n_frames, cape_plane_union_rings* rings /* n_frames x 128 */);
int cape_device_map_union_rings(cape_handle h, cape_plane_union_rings** rings);

/* cape_map_union_holes for a map plane whose hole the detection covers in part as well: instead of CAPE_UNION_HOST_HOLE_CUT the
 * pieces of (hole minus detection) become interior rings, as carry_hole's rings_union_outer(hole, detection, &pieces, 1) computes
 * them.  The arrangement of the hole (as the projected map polygon holds it) and the detection's ring is built a second time inside
 * the pair, with its own eps, cuts, nodes and start node; its outer face is walked only to mark its edges; every other bounded face
 * whose probe point lies in or on the hole and not in or on the detection is a piece after drop_collinear if it has >= 3 vertices,
 * is simple and its area exceeds 1e-12 of the bigger operand's (of the FIRST pair of operands).  The interior rings of a served
 * polygon stand in the host's order: the new ones, then per hole of the map plane, in the map's order, the kept hole itself, nothing
 * for a covered one, or the cut hole's pieces in face-walk order.  Such a pair is served with CAPE_UNION_HOLE_PIECES; holes_covered
 * counts the wholly covered holes only.  Never sets CAPE_UNION_HOST_HOLE_CUT, HOST_MAP_HOLES or HOST_NEW_HOLE.
 * CAPE_UNION_HOST_CAPACITY as for cape_map_union_holes -- the limits on interior rings and their vertices count the pieces -- and
 * for the second arrangement's own limits: more than 1024 cuts, more than CAPE_MAP_UNION_MAX_NODES nodes, a node of more than 8
 * neighbours, a walk that reaches its guard or outgrows CAPE_MAP_MAX_RING.  CAPE_UNION_HOST_AMBIGUOUS also for an angle comparison of
 * the second walk.  A pair without a partly covered hole has the rows, rings and vertices of cape_map_union_holes bit for bit.
 * Preconditions and error codes of cape_map_union_holes.  Writes the same row buffer, slab and rings table: the copy and device-pointer
 * calls of both return its results; a later cape_map_union makes the rings table stale, a later cape_map_union_holes overwrites
 * everything with its own rows (and the other way round). */
int cape_map_union_cut(cape_handle h, int32_t n_frames, void* stream);

/* The COMMIT of the map update on the device: the uploaded map M and frame `frame` of the last cape_map_union, cape_map_union_holes or
 * cape_map_union_cut -- which must be current on the batch, map, match, measurements and Kalman results -- become the map_out of
 * cape_host_map_update for that frame, in the device's map and track buffers.  Pure data movement (no floating-point statement):
 * the new map is the host twin's cape_host_map_commit (host/cape_host_map.h) on the same rows byte for byte.  The list order is
 * unchanged; PROMOTE, DROP and LOST are reported in the track's `result` and left to the caller, as the host update leaves them.
 * Per map plane j in order:
 *   no pair (cape_map_track_result.kept_plane < 0), or a pair whose fusion row lacks CAPE_FUSION_STATE: plane, frame, rings and
 *     covariance are M's;
 *   CAPE_FUSION_STATE and a union row of this pair with CAPE_UNION_SERVED: normal, d and covariance of the fusion row; x_axis, y_axis
 *     and center of the union row; the rings from the frame's slab at vertex_offset, split by the rings table (ring_count,
 *     vertex_count[]) -- one ring of row.vertex_count vertices after a plain cape_map_union -- copied as they lie (they are in the
 *     host class's orientation);
 *   CAPE_FUSION_STATE otherwise: the frame is refused, CAPE_COMMIT_HOST_PAIR where the union row carries a CAPE_UNION_HOST_* bit,
 *     CAPE_COMMIT_FAIL_POLYGON where there is no union pair (or one that neither served nor handed over);
 *   every plane: successive_matched, failed_tracking and result of cape_map_track_result; flags and id are kept.
 * Then, with CAPE_COMMIT_ADD_STAGED, every kept plane of the frame's whole record chain whose fusion row lacks CAPE_FUSION_USED and
 * whose measurement row has CAPE_MEASURE_STAGEABLE is appended in kept-plane order: the plane (staged_normal, d), covariance and frame
 * of the measurement row, one ring, its world ring; flags CAPE_MAP_TRACK_STAGED, counters 0, result CAPE_MAP_RESULT_APPENDED, id
 * (*next_id)++.  Kept plane i is resolved through the kept-plane table of the wide match, as cape_map_kalman does, and every index is
 * checked against its buffer.  Rings and vertices are laid out plane after plane, back to back, as cape_map_upload lays them out.
 * A refused frame (any flag but CAPE_COMMIT_DONE) changes nothing: map, tracks, every result buffer and *next_id stay as they were, and
 * the caller downloads the map, runs cape_host_map_update and uploads.  n_updated, n_appended, n_host_pairs and n_fail_polygon are
 * what the plan counted either way.
 * The work is enqueued on `stream` behind the union; the call RETURNS once the result header has come back through pinned memory --
 * one small read that tells the host the new plane count for the next launch: the sequential step of a tracking loop.
 * A DONE commit invalidates what cape_map_upload invalidates (visibility words, map matches, Kalman and union results) but not the
 * tracks, which are now the committed ones: a following cape_match_map_wide + cape_map_kalman needs no cape_map_upload_tracks, and
 * cape_map_measure's rows stay valid.  CAPE_ERR_CAPACITY: no union result is current, or `frame` is outside what it covered;
 * CAPE_ERR_INVALID_ARGUMENT: NULL handle, out or next_id, unknown flags, a negative frame. */
enum
{
    CAPE_COMMIT_ADD_STAGED = 1u << 0 /* flags of the call */
};
enum /* cape_map_commit_result.flags */
{
    CAPE_COMMIT_DONE = 1u << 0,           /* the map and the tracks are the new ones */
    CAPE_COMMIT_FRAME_OVERFLOW = 1u << 1, /* the wide match flagged the frame CAPE_MATCH_EXACT_OVERFLOW */
    CAPE_COMMIT_BAD_POSE_COV = 1u << 2,   /* CAPE_KALMAN_BAD_POSE_COV: the host refuses the whole frame */
    CAPE_COMMIT_HOST_PAIR = 1u << 3,      /* a pair with CAPE_FUSION_STATE whose union row carries a CAPE_UNION_HOST_* bit */
    CAPE_COMMIT_FAIL_POLYGON = 1u << 4,   /* a pair with CAPE_FUSION_STATE and no union pair (FAIL_POLYGON on the host: the polygon
                                             would be the projected or the old one, which the device does not hold) */
    CAPE_COMMIT_CAPACITY = 1u << 5        /* the new map exceeds CAPE_MAP_MAX_PLANES or a uint32 offset */
};
typedef struct cape_map_commit_result
{
    uint32_t flags;
    int32_t frame;
    int32_t n_planes, n_rings; /* of the map after the call (the old map's if not DONE) */
    int64_t n_vertices;
    int32_t n_updated, n_appended, n_host_pairs, n_fail_polygon;
    uint64_t next_id; /* after the call */
} cape_map_commit_result;
int cape_map_commit(cape_handle h, int32_t frame, uint32_t flags, uint64_t* next_id, cape_map_commit_result* out, void* stream);
/* The sizes of the device map as it stands, after a cape_map_upload or a commit.  Any pointer may be NULL.  Synchronous.
 * CAPE_ERR_INVALID_ARGUMENT: NULL handle, no map. */
int cape_map_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices);
/* Synchronous copy of the device map and tracks as they stand: after cape_map_upload the upload with the rings re-oriented and laid
 * out plane after plane, after a DONE commit the committed map.  tracks (planes_capacity entries, may be NULL): what
 * cape_map_upload_tracks or the commit left, `result` and `id` included; the zero track per plane if none were uploaded for this map.
 * CAPE_ERR_INVALID_ARGUMENT: NULL handle, no map, a negative capacity, a NULL array the map needs; CAPE_ERR_CAPACITY: an array is too
 * small (cape_map_info tells the sizes). */
int cape_map_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, int32_t rings_capacity,
                      double* vertices, int64_t vertices_capacity, cape_map_track* tracks /* planes_capacity, may be NULL */);

/* The LIST MAINTENANCE of the map update on the device: PROMOTE, DROP and LOST executed on the device map and tracks as they stand --
 * after a DONE cape_map_commit, or after cape_map_upload + cape_map_upload_tracks -- with a RETIRED LOG on the device that receives the
 * lost planes.  It is what Feature_Map::update_local_map (feature_map.hpp:748-762) and update_staged_map (:805-830) do to their two
 * containers, with the constructor LocalMapPlane(const StagedMapPlane&) (map_primitive.cpp:286-318), on this project's ONE ordered
 * list.  The host twin cape_host_map_maintain (host/cape_host_map.h) gives the same bytes.  Per map plane j, decided from the
 * track's counters and flags (not from `result`; after a commit the two agree):
 *   staged (CAPE_MAP_TRACK_STAGED), in this order:
 *     successive_matched >= 4: PROMOTE.  The constructor throws unless is_covariance_valid of the 4 x 4 covariance and
 *       double_equal(|normal|, 1) (threshold DBL_EPSILON) hold.  Where both hold the plane stays in the list with
 *       CAPE_MAP_TRACK_STAGED cleared and failed_tracking = 0; successive_matched, id, result, CAPE_MAP_TRACK_MOVING, covariance,
 *       plane, frame and rings are kept.  Where one fails the plane stays staged and unchanged and is counted in n_promote_refused;
 *       it is not dropped either (the reference's `else if` is not reached; there the iterator does not advance at all);
 *     else failed_tracking >= 2: DROP.  The plane is removed and not logged;
 *     else the plane is kept as it is;
 *   local: failed_tracking >= 10: LOST.  The plane is removed and appended to the retired log -- the plane, all its rings and
 *     vertices and the whole cape_map_track, id and CAPE_MAP_TRACK_MOVING included; the caller applies the reference's
 *     `if (not is_moving()) write_to_file` (feature_map.hpp:750-754).  Else the plane is kept.
 * The new list is a STABLE PARTITION of the survivors: first those that are not staged after the step, in list order, then those
 * that are staged, in list order -- so a promoted plane goes behind the last local plane of a list that has its local planes first,
 * everything else keeps its relative order, and the commit's later appends still land at the end.  Rings and vertices are laid out
 * plane after plane, back to back, as cape_map_upload lays them out.  The call is idempotent.
 * out->flags is exactly one of:
 *   CAPE_MAINTAIN_DONE: map, tracks and log are the new ones.  It invalidates what a DONE commit invalidates (visibility words, map
 *     matches, Kalman and union results), not the tracks and not cape_map_measure's rows;
 *   CAPE_MAINTAIN_NOTHING: no plane is promoted, dropped or lost.  Nothing is written, swapped or invalidated;
 *   a refusal, which changes nothing, log included: CAPE_MAINTAIN_CAPACITY, a map plane whose rings do not lie in the map's buffers;
 *     CAPE_MAINTAIN_LOG_FULL, the lost planes of this call do not fit the log's CAPE_MAP_RETIRED_MAX_PLANES (both bits may be set).
 * The class counts are what the plan counted either way; the sizes are the old ones unless DONE.
 * Like the commit, the work (a plan kernel and a copy kernel) is enqueued on `stream` and the call RETURNS once the result header has
 * come back through pinned memory.  CAPE_ERR_INVALID_ARGUMENT: NULL handle or out, non-zero flags, no map; CAPE_ERR_CAPACITY: no
 * tracks are current for the map (cape_map_upload_tracks, or a DONE commit). */
#define CAPE_MAP_RETIRED_MAX_PLANES 4096 /* planes the retired log holds until cape_map_retired_clear */
enum /* cape_map_maintain_result.flags */
{
    CAPE_MAINTAIN_DONE = 1u << 0,     /* the map, the tracks and the log are the new ones */
    CAPE_MAINTAIN_NOTHING = 1u << 1,  /* nothing was due: nothing written, swapped or invalidated */
    CAPE_MAINTAIN_CAPACITY = 1u << 2, /* a map plane whose rings do not lie in the map's buffers */
    CAPE_MAINTAIN_LOG_FULL = 1u << 3  /* the lost planes of this call do not fit the retired log */
};
typedef struct cape_map_maintain_result
{
    uint32_t flags;
    int32_t n_planes, n_rings; /* of the map after the call */
    int32_t n_local;           /* survivors that are not staged after the step: the first n_local planes of a DONE call's list */
    int64_t n_vertices;
    int32_t n_staged; /* survivors that are staged after the step */
    int32_t n_promoted, n_promote_refused, n_dropped, n_lost;
    int32_t n_retired, n_retired_rings; /* of the retired log after the call */
    uint32_t pad;
    int64_t n_retired_vertices;
} cape_map_maintain_result;
int cape_map_maintain(cape_handle h, uint32_t flags /* must be 0 */, cape_map_maintain_result* out, void* stream);
/* The RETIRED LOG: the lost planes of every DONE cape_map_maintain since the handle was created or the log was cleared, in the order
 * they were lost, in the layout of a map -- planes, rings, vertices, tracks -- whose ring_first and vertex_offset are relative to the
 * log's own arrays.  It survives cape_map_upload, commits and further maintains.  cape_map_retired_info: its sizes (any pointer may be
 * NULL).  cape_map_retired_download: a synchronous copy under the rules of cape_map_download (tracks may be NULL).
 * cape_map_retired_clear: the log is empty afterwards (it waits for a call in flight).  CAPE_ERR_INVALID_ARGUMENT: NULL handle, a
 * negative capacity, a NULL array the log needs; CAPE_ERR_CAPACITY: an array is too small. */
int cape_map_retired_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices);
int cape_map_retired_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, int32_t rings_capacity,
                              double* vertices, int64_t vertices_capacity, cape_map_track* tracks /* planes_capacity, may be NULL */);
int cape_map_retired_clear(cape_handle h);

/* ONE FRAME THROUGH THE DEVICE MAP: the sequential step of a tracker, frame `frame` of the current batch against the map the frame
 * before left.  The call enqueues on `stream`, for that frame alone: the wide match against the device map (cape_match_map_wide's
 * kernels on one frame; world_to_camera: 16 doubles, this frame's; skip: (n_map + 31) / 32 words of this frame, may be NULL), the
 * Kalman step, the union in cut mode, the commit and -- decided on the device from the commit's header, only if it says
 * CAPE_COMMIT_DONE -- the maintenance of the committed map.  It waits ONCE, for both headers.  Afterwards the device map, tracks,
 * ids, retired log and *next_id hold, byte for byte, what cape_match_map_wide(n), cape_map_kalman(n), cape_map_union_cut(n),
 * cape_map_commit(frame, commit_flags) and, behind a DONE commit, cape_map_maintain(0) leave on the same map, tracks and log, for
 * any n > frame; out->commit and out->maintain are what those two calls report (maintain all zero, flags 0, where the commit is
 * not DONE: the maintenance has not run).
 *   commit refused:                   nothing changes, *next_id included;
 *   DONE, maintenance NOTHING:        the committed map;
 *   DONE, maintenance DONE:           the maintained map, and the log;
 *   DONE, maintenance refused:        the committed map, the log unchanged.
 * It needs a map with current tracks (cape_map_upload + cape_map_upload_tracks, or a DONE commit, maintenance or step: the next
 * step needs no upload) and the cape_build_polygons and cape_map_measure of the batch covering `frame`.  match_flags:
 * CAPE_MATCH_ADVANCED and CAPE_MATCH_ALLOW_INDEX0 (CAPE_MATCH_MAP_AREAS and CAPE_MATCH_MAP_DEVICE_SKIP are refused: the
 * visibility words do not survive a commit); commit_flags: cape_map_commit's.  The step works in the buffers of
 * cape_match_map_wide, cape_map_kalman and cape_map_union*: whatever its outcome their batch-wide results are NOT current
 * afterwards (their cape_copy_* / cape_device_* readers refuse as after a DONE commit); cape_map_measure's rows stay valid; the
 * visibility words are invalidated when the commit is DONE.  cape_map_info, cape_map_download and cape_map_retired_* read what the
 * step left.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, out, next_id or pose, a negative frame, an unknown or refused flag, no map;
 * CAPE_ERR_CAPACITY: no tracks are current for the map, no cape_map_measure covers the frame, the frame lies beyond the polygons. */
typedef struct cape_map_step_result
{
    cape_map_commit_result commit;     /* as cape_map_commit would report for this frame */
    cape_map_maintain_result maintain; /* as cape_map_maintain behind a DONE commit; all zero (flags 0) where the commit is not DONE */
} cape_map_step_result;
int cape_map_step(cape_handle h, int32_t frame, const double* world_to_camera /* 16, this frame's */,
                  const uint32_t* skip /* (n_map+31)/32 words of this frame, may be NULL */, uint32_t match_flags, uint32_t commit_flags,
                  uint64_t* next_id, cape_map_step_result* out, void* stream);

/* THE SAME STEP WITH THE FRAME'S SKIP WORDS DECIDED ON THE DEVICE, in the same call and behind the same single wait: the first
 * statement of the loop the step stands for, `if (mapFeature.is_moving() or not mapFeature.is_visible(worldToCamera)) continue;`.
 * Ahead of the match the call decides, for the map as it finds it (n_map planes, BEFORE the step), bit j = the device track j has
 * CAPE_MAP_TRACK_MOVING, or map plane j is not visible from world_to_camera -- a one-frame classify kernel that reads the moving
 * bit from the device tracks, then cape_map_visibility's intersection kernels -- and the match reads those words on the device.
 * Afterwards the device map, tracks, ids, retired log, *next_id and out->step are byte for byte what this route leaves on the same
 * map, tracks and log:  moving = the tracks' CAPE_MAP_TRACK_MOVING bits;  cape_map_visibility(1, world_to_camera, moving);
 * cape_copy_map_visibility(1, words, &und);  cape_map_step(frame, world_to_camera, words, match_flags, commit_flags, &id, &r).
 * The words are those of that route (cape_host_map_visibility's bit for bit, the bits beyond n_map in the last word 0) and
 * out->n_undecided == und.  An empty map runs no visibility kernel and has no words (n_map = 0); the step proceeds, so that it can
 * append.  match_flags, commit_flags, the preconditions and the error list are cape_map_step's (CAPE_MATCH_MAP_AREAS and
 * CAPE_MATCH_MAP_DEVICE_SKIP are refused), and so is what the call does to the results of other calls.  The words live in a buffer
 * of the step's own: the words of cape_map_visibility are neither read nor written (cape_copy_map_visibility behaves as after a
 * cape_map_step: it refuses once the commit is DONE).
 * cape_map_step_skip_words: a synchronous copy of the words of the last cape_map_step_visible, (n_map + 31) / 32 of them for the
 * map as it was BEFORE that step, whatever the step's outcome (a refused commit included); valid until the next
 * cape_map_step_visible or cape_map_upload.  *n_map (may be NULL) is that map's plane count.  CAPE_ERR_CAPACITY: no such step since
 * the last cape_map_upload, or words_capacity is too small (*n_map is still reported); CAPE_ERR_INVALID_ARGUMENT: NULL handle, a
 * negative capacity, NULL words with n_map > 0. */
typedef struct cape_map_step_visible_result
{
    cape_map_step_result step; /* exactly what cape_map_step reports */
    int32_t n_map;             /* planes of the map the words were decided against (the map BEFORE the step) */
    int32_t n_moving;          /* of them, CAPE_MAP_TRACK_MOVING in the device track */
    int32_t n_listed;          /* not moving and not ruled out by the classify: handed to the ring intersection */
    int32_t pad;
    int64_t n_undecided;       /* pairs beyond the intersection capacities: they count as visible, as in cape_map_visibility */
} cape_map_step_visible_result;
int cape_map_step_visible(cape_handle h, int32_t frame, const double* world_to_camera /* 16, this frame's */, uint32_t match_flags,
                          uint32_t commit_flags, uint64_t* next_id, cape_map_step_visible_result* out, void* stream);
int cape_map_step_skip_words(cape_handle h, uint32_t* words, int32_t words_capacity, int32_t* n_map);

/* THE PLANE COST FUNCTION OF THE POSE SOLVER, for a batch of pose hypotheses per frame: the stage between the match and the update
 * (find matches -> optimise the pose -> update -> maintain).  The solver itself (RANSAC over hypotheses, Levenberg-Marquardt) is
 * cape_map_pose_solve / cape_map_pose_select below; what it evaluates thousands of times per frame -- PlaneOptimizationFeature::is_inlier / get_distance
 * (map_primitive.cpp:15-85), called by Pose_Optimization::get_features_inliers_outliers (pose_optimization.cpp:40-75) and the LM
 * functor (levenberg_marquardt_functors.cpp:154-166) -- runs here on data that is already on the device.
 * Frame f's PAIRS are the map planes j = 0 .. n_map-1 in ascending order with i = match[f][j] >= 0 of the last cape_match_map_wide,
 * at most 128.  The k-th pair's feature row: matched = (out_normal, d) of the segment the wide match's kept-plane table names for
 * kept plane i (every index taken from that table is checked against the record buffer before use; one that fails gives NaN, i.e. an
 * invalid feature and an outlier), map_plane = the map plane's (normal, d), stddev[c] = sqrt(covariance[5 c]) of the device track,
 * map_id = the track's id.  For hypothesis T = world_to_camera[f][h], with (qn, qd) = plane_to_camera(T, map plane):
 *   signed[c] = atan2(sin(cn[c] - qn[c]), cos(cn[c] - qn[c])) for c < 3 (get_signed_distance, plane_coordinates.cpp:26-37, through
 *     angle_distance, distance_utils.cpp:6-9: the reference feeds normal components to an angle function), signed[3] = cd - qd;
 *   inlier = |signed[c]| <= (double)0.2f for c < 3 and |signed[3]| <= (double)50.0f (parameters.hpp:27-30; a NaN is an outlier);
 *   reduced[c] = cd cn[c] - qd qn[c] (get_reduced_signed_distance, plane_coordinates.cpp:49-56);
 *   r[c] = reduced[c] * 1.0 / 3.0 and sum_sq += r[c] r[c], c ascending within k, k ascending;  score += 1.0 / 3 per inlier in pair
 *     order (get_score, map_primitive.cpp:27-31).
 * A pair is VALID (is_valid, map_primitive.cpp:79-83) when matched, map_plane and stddev hold no NaN and no stddev is negative.  An
 * invalid pair is still scored; it is counted in n_invalid and every row of the frame carries CAPE_POSE_SCORE_INVALID_FEATURE (the
 * reference abandons the optimisation there, pose_optimization.cpp:270-280: the caller decides).
 * Everything but the three atan2(sin, cos) values is + - x / sqrt and equals the host twin cape_host_pose_score
 * (host/cape_host_map.h) bit for bit; the three angle parts are the device math library's and may differ from the host's libm in
 * the last places.  Every sum belongs to one (frame, hypothesis) and is taken in pair order: no result depends on the other
 * hypotheses of the call. */
enum /* flags of cape_map_pose_score */
{
    CAPE_POSE_SCORE_DEVICE_POSES = 1u << 0, /* world_to_camera is DEVICE memory, read in place when the kernel runs */
    CAPE_POSE_SCORE_RESIDUALS = 1u << 1     /* also keep signed[4] and reduced[3] of every (frame, hypothesis, pair) */
};
enum /* cape_pose_score.flags, beside CAPE_MATCH_EXACT_OVERFLOW */
{
    CAPE_POSE_SCORE_INVALID_FEATURE = 1u << 8 /* a pair of the frame fails is_valid (n_invalid > 0) */
};
typedef struct cape_pose_score /* 48 bytes, one per (frame, hypothesis) */
{
    int32_t n_pairs, n_inliers, n_invalid;
    uint32_t flags;            /* CAPE_MATCH_EXACT_OVERFLOW of the wide match (n_pairs = 0, everything else 0), CAPE_POSE_SCORE_INVALID_FEATURE */
    double score, sum_sq;      /* n_inliers times 1.0 / 3 added in pair order; the sum of the squared LM residuals */
    uint32_t inlier_words[4];  /* bit i set: kept plane i is matched and an inlier */
} cape_pose_score;
typedef struct cape_pose_feature /* 112 bytes, one per pair k < 128 of a frame, all zero beyond n_pairs: the constructor arguments of
                                    PlaneOptimizationFeature */
{
    double matched[4];   /* the detected plane (cn, cd), camera coordinates */
    double map_plane[4]; /* the map plane (normal, d), world coordinates */
    double stddev[4];    /* sqrt of the track covariance's diagonal */
    uint64_t map_id;     /* the track's id */
    int32_t map_index, kept_plane; /* j and i of the pair */
} cape_pose_feature;
/* world_to_camera: n_frames x n_hypotheses x 16 doubles, row-major [R t; 0 0 0 1] -- HOST memory read before the call returns, or,
 * with CAPE_POSE_SCORE_DEVICE_POSES, device memory that must stay unchanged until the call's work on `stream` is done.
 * CAPE_POSE_SCORE_RESIDUALS keeps the table [f][h][k][7] (CAPE_ERR_CAPACITY if n_frames x n_hypotheses x 128 x 7 x 8 bytes would
 * exceed 1 GiB).  Needs, on the current batch and covering n_frames, a cape_match_map_wide since the last cape_map_upload, and tracks
 * current for the map -- otherwise CAPE_ERR_CAPACITY.  CAPE_ERR_INVALID_ARGUMENT: NULL handle or poses, n_frames < 0,
 * n_hypotheses < 1, unknown flag.  A frame the wide match flagged CAPE_MATCH_EXACT_OVERFLOW reports that flag, n_pairs = 0 and zeros;
 * an empty map succeeds with n_pairs = 0 everywhere.  Nothing is written into the map, the tracks, the matches or any other call's
 * results: the buffers are the handle's own, grown on demand.  The feature rows are shared with cape_map_pose_solve and
 * cape_map_pose_covariance: whichever of the three runs first on a batch, map, tracks and match builds them, a call over more frames
 * builds them again in place with the bytes they hold, and their address (cape_pose_score_device) never changes.  What invalidates cape_map_kalman's results -- a later cape_extract,
 * cape_build_polygons, cape_map_upload, cape_map_upload_tracks, cape_match_map_wide, cape_map_measure, or a cape_map_commit,
 * cape_map_maintain or cape_map_step[_visible] that changes the map -- invalidates these.  Asynchronous on `stream`. */
int cape_map_pose_score(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double* world_to_camera, uint32_t flags, void* stream);
/* Synchronous copy of the last cape_map_pose_score: scores (n_frames x n_hypotheses of that call), features (n_frames x 128),
 * residuals (n_frames x n_hypotheses x 128 x 7: signed[4] then reduced[3], zeros beyond n_pairs; the call must have had
 * CAPE_POSE_SCORE_RESIDUALS, else CAPE_ERR_INVALID_ARGUMENT).  Any pointer may be NULL.  CAPE_ERR_CAPACITY: more frames than that call
 * covered, or its results are no longer current. */
int cape_copy_pose_scores(cape_handle h, int32_t n_frames, cape_pose_score* scores, cape_pose_feature* features, double* residuals);
/* Device pointers of the score rows (frames x n_hypotheses of the call) and the feature rows (frames x 128), for a caller that
 * selects the best hypothesis with a kernel of its own on the stream of the scoring call.  Either may be NULL.  CAPE_ERR_CAPACITY
 * when no cape_map_pose_score is current. */
int cape_pose_score_device(cape_handle h, const cape_pose_score** scores, const cape_pose_feature** features);

/* THE POSE SOLVER ITSELF on the same pairs: Levenberg-Marquardt per (frame, hypothesis), the RANSAC bookkeeping over a frame's scored
 * hypotheses and the final re-optimisation on the chosen inliers (Pose_Optimization::compute_pose_with_ransac and
 * compute_optimized_global_pose, pose_optimization.cpp:90-350).  The chain, on one stream without a host wait in between:
 *   cape_match_map_wide -> cape_map_pose_solve(subsets) -> cape_map_pose_score(CAPE_POSE_SCORE_DEVICE_POSES = the solve's poses) ->
 *   cape_map_pose_select -> cape_map_pose_solve(CAPE_POSE_SOLVE_FROM_SELECTION);  the host only draws the random subsets.
 * A PROBLEM (f, h) minimises the sum of r^2 over the pairs of frame f (those of cape_map_pose_score, in its order) that the subset
 * names: r = reduced[c] * 1.0 / 3.0 for c < 3, pair after pair (the LM functor, levenberg_marquardt_functors.cpp:154-166), the map
 * plane seen through the pose of x.  x[6] = the position, then the three coefficients of get_optimization_coefficients_from_quaternion;
 * the pose of x: the quaternion of the coefficients (levenberg_marquardt_functors.cpp:29-38), normalised (pose.cpp:20), its rotation
 * matrix R, camera-to-world [C R | C p] with the camera basis C of the parameters, world-to-camera its rigid inverse.  The minimiser is
 * MINPACK's lmstr driver with a forward-difference Jacobian (rules and departures from the reference: csrc/cape_pose_solve.h).
 * Everything is + - x / sqrt in one order and equals the host twin cape_host_pose_solve (host/cape_host_map.h) bit for bit; no
 * result of a problem depends on the other problems of the call. */
enum /* flags of cape_map_pose_solve */
{
    CAPE_POSE_SOLVE_DEVICE_INPUT = 1u << 0,  /* x0 and subsets are DEVICE memory, read in place when the kernel runs */
    CAPE_POSE_SOLVE_FROM_SELECTION = 1u << 1 /* one problem per frame from x and inlier_words of the last cape_map_pose_select */
};
enum /* cape_pose_solution.status: MINPACK's info 1..8 when the minimiser ran, or why the problem was refused (x = x0 then) */
{
    CAPE_POSE_SOLVE_TOO_FEW_PAIRS = -1,   /* 3 x pairs <= 6 (pose_optimization.cpp:322-331) */
    CAPE_POSE_SOLVE_LOW_SCORE = -2,       /* the subset's score, 1.0 / 3 added per pair in order, is below 1.0 (same lines) */
    CAPE_POSE_SOLVE_INVALID_FEATURE = -3, /* the frame has n_invalid > 0 (pose_optimization.cpp:270-282) */
    CAPE_POSE_SOLVE_OVERFLOW = -4,        /* the wide match flagged the frame CAPE_MATCH_EXACT_OVERFLOW */
    CAPE_POSE_SOLVE_BAD_START = -5,       /* a NaN or an infinity in x0 */
    CAPE_POSE_SOLVE_NOT_FINITE = -6,      /* a NaN or an infinity in x or in a residual during the run: x is the last accepted point */
    CAPE_POSE_SOLVE_NO_SELECTION = -7     /* CAPE_POSE_SOLVE_FROM_SELECTION on a frame whose selection has no best hypothesis */
};
enum /* cape_pose_solution.flags, beside CAPE_MATCH_EXACT_OVERFLOW and CAPE_POSE_SCORE_INVALID_FEATURE of the frame */
{
    CAPE_POSE_SOLVE_RANK_DEFICIENT = 1u << 9 /* a diagonal entry of R was 0 at least once: the pivoted qrfac ran */
};
enum /* cape_pose_selection.flags */
{
    CAPE_POSE_SELECT_NO_CONSENSUS = 1u << 0, /* no hypothesis was taken: best = -1 */
    CAPE_POSE_SELECT_EARLY_STOP = 1u << 1    /* the scan ended before the last hypothesis (pose_optimization.cpp:225-229) */
};
typedef struct cape_pose_solve_params /* NULL = the defaults of Eigen::LevenbergMarquardt and the identity basis */
{
    double ftol, xtol;       /* sqrt(DBL_EPSILON) */
    double gtol;             /* 0 */
    double factor;           /* 100 */
    double epsfcn;           /* 0: the difference step is sqrt(max(epsfcn, DBL_EPSILON)) |x_j|, or that factor alone where x_j = 0 */
    int32_t maxfev;          /* 400; a Jacobian counts 6 */
    int32_t mode;            /* 1: the columns' norms scale the variables (internal scaling); 2: no scaling */
    double camera_basis[9];  /* C, row-major: the reference's constant CameraToWorld rotation (camera_transformation.cpp:11-18) */
} cape_pose_solve_params;
typedef struct cape_pose_solution /* 96 bytes, one per problem */
{
    double x[6];           /* where the minimiser ended (the start for a refused problem) */
    double fnorm0, fnorm;  /* the residuals' norm at the start and at x (0 for a refused problem) */
    int32_t status;        /* > 0: MINPACK's info; < 0: CAPE_POSE_SOLVE_* */
    int32_t nfev;          /* evaluations of the residual vector, the Jacobians' included */
    int32_t iterations;    /* accepted steps */
    int32_t n_pairs_used;  /* pairs of the frame that the subset names */
    uint32_t flags;
    uint32_t reserved[3];
} cape_pose_solution;
typedef struct cape_pose_selection /* 96 bytes, one per frame */
{
    int32_t best;             /* the chosen hypothesis, -1: none (CAPE_POSE_SELECT_NO_CONSENSUS) */
    int32_t n_scanned;        /* hypotheses the scan looked at before it stopped */
    int32_t n_inliers;        /* of the chosen hypothesis */
    uint32_t flags;           /* CAPE_POSE_SELECT_* */
    double score;             /* of the chosen hypothesis (1.0 when none) */
    double reserved;
    uint32_t inlier_words[4]; /* its cape_pose_score.inlier_words: a subset for CAPE_POSE_SOLVE_FROM_SELECTION */
    double x[6];              /* its cape_pose_solution.x */
} cape_pose_selection;
/* n_frames x n_hypotheses problems.  x0: 6 doubles per problem; subsets: 4 uint32 per problem, bit i = the pair of kept plane i takes
 * part (the indexing of cape_pose_score.inlier_words; bits of unmatched kept planes are ignored) -- HOST memory read before the call
 * returns, or with CAPE_POSE_SOLVE_DEVICE_INPUT device memory that must stay unchanged until the call's work on `stream` is done.  With
 * CAPE_POSE_SOLVE_FROM_SELECTION n_hypotheses must be 1, x0 and subsets are not read, and a current cape_map_pose_select covering
 * n_frames is needed (CAPE_ERR_CAPACITY otherwise).  Per problem a cape_pose_solution and the pose of its x as 16 doubles row-major
 * [R t; 0 0 0 1]: the layout cape_map_pose_score takes with CAPE_POSE_SCORE_DEVICE_POSES.  Needs what cape_map_pose_score needs and is
 * invalidated by what invalidates it; a later cape_map_pose_solve replaces the rows.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, NULL x0
 * or subsets without CAPE_POSE_SOLVE_FROM_SELECTION, n_frames < 0, n_hypotheses < 1, unknown flag, a parameter that is NaN or negative,
 * maxfev < 1, a mode other than 1 and 2.  Nothing but the call's own buffers is written, and, where they do not cover n_frames yet,
 * the feature rows it shares with cape_map_pose_score -- with the bytes that call gives them.  Asynchronous on `stream`. */
int cape_map_pose_solve(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double* x0, const uint32_t* subsets,
                        const cape_pose_solve_params* params, uint32_t flags, void* stream);
/* Synchronous copy of the last cape_map_pose_solve: solutions (n_frames x n_hypotheses of that call) and poses (x 16 doubles).  Either
 * may be NULL.  CAPE_ERR_CAPACITY: more frames than that call covered, or its results are no longer current. */
int cape_copy_pose_solutions(cape_handle h, int32_t n_frames, cape_pose_solution* solutions, double* world_to_camera);
/* Device pointers of the solution rows and of the pose buffer.  Either may be NULL.  CAPE_ERR_CAPACITY when no solve is current. */
int cape_pose_solve_device(cape_handle h, const cape_pose_solution** solutions, const double** world_to_camera);
/* The RANSAC bookkeeping of pose_optimization.cpp:190-235 per frame over the current score rows and solution rows, hypotheses in
 * ascending order: maxScore = 1.0, bestInliers = 0; h is SKIPPED when its solve status is <= 0 or its score < 1.0; it is TAKEN when
 * score > maxScore, or |score - maxScore| <= 0.1 and bestInliers < n_inliers; after a hypothesis that was not skipped the scan stops
 * when h >= 3 and bestInliers > ceil(n_pairs x (double)0.80f).  Needs a current cape_map_pose_solve (not FROM_SELECTION) and a current
 * cape_map_pose_score with the same n_hypotheses, both covering n_frames: CAPE_ERR_CAPACITY otherwise.  Asynchronous on `stream`. */
int cape_map_pose_select(cape_handle h, int32_t n_frames, void* stream);
/* Synchronous copy of the last cape_map_pose_select (n_frames rows).  CAPE_ERR_CAPACITY: more frames than it covered, or not current. */
int cape_copy_pose_selection(cape_handle h, int32_t n_frames, cape_pose_selection* selection);

/* THE POSE'S COVARIANCE after the refit: Pose_Optimization::compute_pose_variance (pose_optimization.cpp:361-437), the statement that
 * makes a pose usable (local_map.hpp:118 refuses the map update without a valid pose covariance; CAPE_MEASURE_BAD_POSE_COV here).  The
 * chain goes on, on the same stream without a host wait:
 *   ... -> cape_map_pose_solve(CAPE_POSE_SOLVE_FROM_SELECTION) -> cape_map_pose_covariance(CAPE_POSE_COVARIANCE_FROM_SOLUTION).
 * Per frame and iteration i < n_iterations every pair of the subset gets its map plane varied by four standard-normal deviates z times
 * the feature row's stddev (n' = n + z[0..2] stddev[0..2], divided by its norm where that is > 0; d' = d + z[3] stddev[3]), and the
 * problem is minimised again from x on the varied planes with cape_map_pose_solve's minimiser, parameters and guards.  A sample counts
 * when its status is > 0 and its x holds no NaN.  The pose vector of a sample is x[0..2] followed by Eigen's eulerAngles(0, 1, 2) of
 * the rotation of the three coefficients, the first angle in [0, pi] (the reference's own fold: samples that straddle 0 land near 0
 * and near pi).  Over the successes in ascending iteration order: mean = sum / n_ok; covariance = sum (v - mean)(v - mean)^T /
 * (n_ok - 1) + 0.001 I, then is_covariance_valid.  n_ok = 1 divides by zero as the reference does: CAPE_POSE_COVARIANCE_INVALID.
 * The deviates are Philox4x32-10 words keyed by `seed` at the counter (frame + frame_base, iteration, pair slot, block 0 / 1), turned
 * into four uniforms in (0, 1] and two Box-Muller pairs -- NOT the reference's mt19937 stream, which its own tbb::parallel_for leaves
 * unordered -- or, with CAPE_POSE_COVARIANCE_TABLE, the caller's table [n_iterations][128 pair slots][4] shared by all frames of the
 * call.  Rules: csrc/cape_pose_covariance.h; host twin: cape_host_pose_covariance (host/cape_host_map.h).  With a table everything
 * up to a sample's x is + - x / sqrt and equals the twin bit for bit; the three angles go through atan2, sin and cos.
 * covariance[0..2][0..2], the position block, is what cape_map_measure takes as pose_covariance. */
enum /* flags of cape_map_pose_covariance (DEVICE_INPUT also of cape_pose_draw_deviates: `out` is device memory) */
{
    CAPE_POSE_COVARIANCE_DEVICE_INPUT = 1u << 0,  /* x, subsets and deviates are DEVICE memory, read in place when the kernels run */
    CAPE_POSE_COVARIANCE_FROM_SOLUTION = 1u << 1, /* x of the last cape_map_pose_solve(CAPE_POSE_SOLVE_FROM_SELECTION) and the subset of
                                                     that selection's inlier_words, both read in device memory when the kernels run */
    CAPE_POSE_COVARIANCE_TABLE = 1u << 2,         /* read `deviates`; otherwise Philox */
    CAPE_POSE_COVARIANCE_KEEP_SAMPLES = 1u << 3,  /* keep every sample's solution row for cape_copy_pose_covariance_samples:
                                                     CAPE_ERR_CAPACITY beyond CAPE_POSE_COVARIANCE_MAX_KEPT rows */
    CAPE_POSE_DRAW_UNIFORMS = 1u << 4             /* cape_pose_draw_deviates only: the four uniforms instead of the four normals */
};
enum /* cape_pose_covariance.status */
{
    CAPE_POSE_COVARIANCE_VALID = 1,
    /* -1 .. -7: the CAPE_POSE_SOLVE_* refusal of the frame (its pairs, its flags, its x; with FROM_SOLUTION the refit's own status):
       no sample ran, mean and covariance are 0 */
    CAPE_POSE_COVARIANCE_TOO_MANY_FAILED = -16, /* n_ok < n_iterations / 2 (integer division): mean and covariance are 0 */
    CAPE_POSE_COVARIANCE_INVALID = -17,         /* is_covariance_valid refused the matrix, which is reported as computed */
    CAPE_POSE_COVARIANCE_NO_SOLUTION = -18      /* FROM_SOLUTION on a refit row whose status is 0 */
};
#define CAPE_POSE_COVARIANCE_MAX_KEPT (1 << 22)             /* sample rows (96 bytes each) a call may keep */
#define CAPE_POSE_COVARIANCE_DEFAULT_BUDGET (256ull << 20)  /* bytes of the varied-plane slab: 4096 x n_iterations per frame */
typedef struct cape_pose_covariance /* 368 bytes, one per frame */
{
    double mean[6];        /* position, then the three Euler angles */
    double covariance[36]; /* row-major */
    int32_t n_ok;          /* samples that count */
    int32_t n_iterations;
    int32_t status;        /* CAPE_POSE_COVARIANCE_* or a CAPE_POSE_SOLVE_* refusal */
    uint32_t flags;        /* CAPE_MATCH_EXACT_OVERFLOW and CAPE_POSE_SCORE_INVALID_FEATURE of the frame */
    int32_t nfev_min, nfev_max; /* over the samples that ran */
    int64_t nfev_sum;
} cape_pose_covariance;
/* x: 6 doubles per frame; subsets: 4 uint32 per frame (cape_map_pose_solve's indexing); deviates: the table -- HOST memory read before
 * the call returns, or device memory with CAPE_POSE_COVARIANCE_DEVICE_INPUT.  With FROM_SOLUTION x and subsets are not read and a
 * current refit and selection covering n_frames are needed (CAPE_ERR_CAPACITY otherwise).  The varied planes live in a slab of the
 * handle, [frame][128][4][iteration], within a byte budget (cape_set_pose_covariance_budget): a call whose frames do not fit is
 * enqueued in chunks of frames without a host wait; CAPE_ERR_CAPACITY if one frame alone (4096 x n_iterations bytes) does not fit.
 * Needs what cape_map_pose_solve needs and is invalidated by what invalidates it.  CAPE_ERR_INVALID_ARGUMENT: what cape_map_pose_solve
 * refuses, n_iterations < 1, CAPE_POSE_COVARIANCE_TABLE with a NULL table, an unknown flag.  Nothing but the call's own buffers is
 * written, and, where they do not cover n_frames yet, the feature rows it shares with cape_map_pose_score -- with the bytes that
 * call gives them.  Asynchronous on `stream`. */
int cape_map_pose_covariance(cape_handle h, int32_t n_frames, int32_t n_iterations, const double* x, const uint32_t* subsets,
                             const double* deviates, uint64_t seed, uint32_t frame_base, const cape_pose_solve_params* params, uint32_t flags,
                             void* stream);
/* Synchronous copy of the last cape_map_pose_covariance (n_frames rows).  CAPE_ERR_CAPACITY: more frames than it covered, or not current. */
int cape_copy_pose_covariance(cape_handle h, int32_t n_frames, cape_pose_covariance* rows);
/* ... and of its sample rows (n_frames x n_iterations of that call; rows of a refused frame are 0): the call must have had
 * CAPE_POSE_COVARIANCE_KEEP_SAMPLES, else CAPE_ERR_INVALID_ARGUMENT. */
int cape_copy_pose_covariance_samples(cape_handle h, int32_t n_frames, cape_pose_solution* samples);
/* Device pointer of the result rows.  CAPE_ERR_CAPACITY when no cape_map_pose_covariance is current. */
int cape_pose_covariance_device(cape_handle h, const cape_pose_covariance** rows);
/* The table [n_iterations][128][4] of the deviates a call with `seed` draws for frame index `frame` (= frame_base + the frame of the
 * call), through the device function that call uses; to host memory, or to device memory with CAPE_POSE_COVARIANCE_DEVICE_INPUT.
 * Synchronous: the table is there when the call returns.  CAPE_POSE_DRAW_UNIFORMS: the four uniforms instead of the normals. */
int cape_pose_draw_deviates(cape_handle h, uint64_t seed, uint32_t frame, int32_t n_iterations, double* out, uint32_t flags);
/* The byte budget of the varied-plane slab (0: CAPE_POSE_COVARIANCE_DEFAULT_BUDGET).  Takes effect with the next call. */
int cape_set_pose_covariance_budget(cape_handle h, uint64_t bytes);

/* A stream of the handle's device for callers that do not link the HIP runtime themselves (the overlay): non-blocking, so the
 * work of several handles driven from several host threads overlaps instead of meeting on the legacy null stream.  Pass it as
 * the `stream` argument of the calls below; destroy it before the handle. */
int cape_stream_create(cape_handle h, void** stream_out);
int cape_stream_destroy(cape_handle h, void* stream);

/* Same, from host memory: H2D copy on `stream`, then cape_extract (host boundary of the reference's
 * cv::Mat_<float> argument).  The copy is part of the call; throughput numbers never use this entry. */
int cape_extract_host(cape_handle h, const float* depth_host, int32_t n_frames, void* stream);
/* The raw 16-bit sensor images from host memory (what a depth PNG decodes to): half the bytes over PCIe, the conversion of
 * cape_extract_u16 on the device.  88 k frames/s against 44 k for float32 input on a PCIe 5 x16 link. */
int cape_extract_u16_host(cape_handle h, const uint16_t* depth_host, float scale, int32_t n_frames, void* stream);

/* Device pointers to the results of the last cape_extract (valid until the next call / destroy):
 * records: n_frames x cape_frame_record ; plane_labels / cyl_labels: n_frames x cells int32
 * (_gridPlaneSegmentMap / _gridCylinderSegMap, primitive_detection.hpp:212-214) ; boundary: n_frames x
 * boundary_capacity x 3 doubles (compute_plane_segment_boundary, primitive_detection.cpp:650-703). */
int cape_device_results(cape_handle h, void** records, int32_t** plane_labels, int32_t** cyl_labels, double** boundary);
/* Sizes the packed buffer (two staging slots of bytes_per_rank on the device) and reports its layout.  May be called
 * again to change the capacities (synchronises). */
int cape_gather_configure(cape_handle h, const cape_gather_config* cfg, cape_gather_layout* layout_out);
/* The same with CAPE_GATHER_POLYGONS implied and the vertex budget of the polygon sections: vertices_capacity = frames_capacity x
 * vertices_per_frame (0 = CAPE_GATHER_DEFAULT_VERTICES_PER_FRAME; the product must fit an int32).  layout_out is filled as by
 * cape_gather_configure, bytes_per_rank including the appended sections; polygon_layout_out has their offsets.  Either may be NULL.
 * cape_gather_configure with the flag in cfg->flags is this call with vertices_per_frame = 0. */
int cape_gather_configure_polygons(cape_handle h, const cape_gather_config* cfg, int32_t vertices_per_frame, cape_gather_layout* layout_out,
                                   cape_gather_polygon_layout* polygon_layout_out);
/* Packs the results of the last cape_extract (frames [0, n_frames) of it) into the next staging slot, asynchronously on
 * `stream`; first_frame goes into the header.  *packed_dev (optional) receives the slot's device address. */
int cape_pack_primitives(cape_handle h, int32_t n_frames, int32_t first_frame, void** packed_dev, void* stream);
/* (With CAPE_GATHER_POLYGONS, cape_pack_primitives and the two gathers need the polygons of the frames they pack: CAPE_ERR_CAPACITY,
 * and nothing is packed, when n_frames exceeds the frames of the last cape_build_polygons of the current batch -- the rule of
 * cape_device_polygons / cape_copy_polygons.) */
/* Synchronous copy of the slot filled by the last cape_pack_primitives / cape_gather_primitives (bytes_per_rank bytes). */
int cape_copy_packed(cape_handle h, void* packed_host);

/* RCCL communicator of the handle (librccl is dlopen'ed on first use).  Rank 0 makes the 128-byte id with
 * cape_comm_unique_id and hands it to the other ranks by any means (file, socket, MPI, torch.distributed store);
 * every rank then calls cape_comm_init, which is collective (ncclCommInitRank on the handle's device). */
#define CAPE_COMM_ID_BYTES 128
int cape_comm_unique_id(void* id_out);
int cape_comm_init(cape_handle h, const void* id, int32_t rank, int32_t world);
int cape_comm_destroy(cape_handle h);
/* What RCCL itself reports for the handle's communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), next to what
 * cape_comm_init was called with: a launcher prints it per rank so that a run on N GPUs can be seen to have had N ranks on N
 * devices.  has_comm = 0 (and -1 in the RCCL fields) when the handle has no communicator -- e.g. when the caller moves the packed
 * bytes with another transport (torch.distributed). */
typedef struct cape_comm_info_t
{
    int32_t has_comm;       /* 1: cape_comm_init succeeded on this handle */
    int32_t has_gather;     /* 1: the loaded librccl offers ncclGather (cape_gather_primitives_root) */
    int32_t nranks, rank;   /* ncclCommCount, ncclCommUserRank (-1: not available) */
    int32_t device;         /* ncclCommCuDevice: the HIP device RCCL bound the communicator to */
    int32_t init_nranks, init_rank; /* world / rank passed to cape_comm_init */
    int32_t handle_device;  /* cape_config.device */
} cape_comm_info_t;
int cape_comm_info(cape_handle h, cape_comm_info_t* out);
/* One batch's exchange: cape_pack_primitives on `stream`, then ONE ncclAllGather of bytes_per_rank per rank on the
 * handle's own communication stream (behind an event, so it runs under whatever the caller enqueues next on `stream`).
 * recv_dev: world x bytes_per_rank device bytes, rank r's shard at r x bytes_per_rank; it must stay untouched until the
 * gather has completed.  A staging slot is reused only after the gather that read it is done (two slots). */
int cape_gather_primitives(cape_handle h, int32_t n_frames, int32_t first_frame, void* recv_dev, void* stream);
/* "gather" in the narrow sense (BASELINE.json north_star): the same exchange with ONE receiver -- ncclGather (an RCCL
 * extension) of bytes_per_rank per rank to rank `root`; recv_dev is read on the root only (may be NULL elsewhere).  At
 * world 8 every other GPU receives nothing instead of 8 x bytes_per_rank.  CAPE_ERR_UNSUPPORTED if the loaded librccl has
 * no ncclGather. */
int cape_gather_primitives_root(cape_handle h, int32_t n_frames, int32_t first_frame, int32_t root, void* recv_dev, void* stream);
/* Totals of the last cape_extract batch (frames [0, n_frames)): what a caller sizes cape_gather_config.planes_per_frame
 * with -- e.g. ceil(1.25 x n_planes / n_frames) + 1 from the previous batch of the same stream -- instead of the default
 * budget.  Synchronous (waits for the batch).  Any output pointer may be NULL. */
int cape_count_primitives(cape_handle h, int32_t n_frames, int32_t* n_planes, int32_t* n_cylinders, int32_t* max_planes_per_frame);
/* Its companion for the vertex budget of CAPE_GATHER_POLYGONS: the ring vertices of every output plane of frames [0, n_frames) of the
 * last cape_build_polygons (record chains followed), and the most one frame holds.  Synchronous.  CAPE_ERR_CAPACITY when
 * cape_build_polygons of the current batch does not cover n_frames.  Either output pointer may be NULL. */
int cape_count_polygon_vertices(cape_handle h, int32_t n_frames, int64_t* n_vertices, int32_t* max_vertices_per_frame);
/* Orders after the last cape_gather_primitives: with host_sync != 0 the call returns when the gather has landed,
 * otherwise `stream` is made to wait for it (hipStreamWaitEvent). */
int cape_gather_wait(cape_handle h, void* stream, int32_t host_sync);

/* Makes `stream` wait for whatever the handle still has in flight for the last cape_extract (the asynchronous second pass of
 * CAPE_FLAG_ASYNC_SECOND_PASS; a no-op otherwise): after it, work enqueued on `stream` may read cape_device_results. */
int cape_sync_results(cape_handle h, void* stream);

/* Synchronous D2H of the results of the last cape_extract.  Any pointer may be NULL. */
int cape_copy_results(cape_handle h, int32_t n_frames, cape_frame_record* records, int32_t* plane_labels,
                      int32_t* cyl_labels, double* boundary);

/* The spill pool of the last cape_extract (synchronous): *used = spill records handed out (a frame's chain is followed through
 * header.next_record, spill record k has index max_batch + k), *capacity = cape_config.spill_records as resolved at create,
 * *frames = frames of the batch that went through the general instance.  Any pointer may be NULL. */
int cape_spill_info(cape_handle h, int32_t* used, int32_t* capacity, int32_t* frames);
/* Synchronous D2H of spill records [first, first + count) -- record indices max_batch + first ... -- and their boundary slabs
 * (count x boundary_capacity x 3 doubles).  Either pointer may be NULL. */
int cape_copy_spill(cape_handle h, int32_t first, int32_t count, cape_frame_record* records, double* boundary);
/* The polygon rows (count x CAPE_MAX_PLANES) and vertex slabs (count x boundary_capacity x 2 doubles) of the same spill records,
 * after cape_build_polygons (which builds the polygons of every spill record in use together with the batch's). */
int cape_copy_spill_polygons(cape_handle h, int32_t first, int32_t count, cape_polygon* polygons, double* vertices);

/* Handles created with max_batch <= 8 (the reference's call pattern: one frame per call) keep records, label grids and
 * boundary points in pinned, device-mapped HOST memory: the kernels write them over PCIe directly and no device-to-host
 * copy exists on the latency path.  cape_host_results waits for the handle's stream and returns pointers to that memory
 * (valid until the next call / destroy); CAPE_ERR_UNSUPPORTED for larger handles, whose results live in HBM.
 * Such a handle also runs the ONE-FRAME CHAIN: stage A as one launch of strip workgroups whenever the frame is in
 * device memory (a device pointer, or the staged copy of a pageable host frame; a frame read in place from pinned memory keeps the
 * two streaming kernels), then ONE grow kernel whose last wave stores the completion number cape_host_results spins on -- two or
 * three launches per call instead of five.  Same results bit for bit; the debug knob CAPE_STAGE_A=bands (read and validated at
 * cape_create, like CAPE_RESUME / CAPE_SCHEDULE) keeps the batch kernels on such a handle, CAPE_STAGE_A=strips forces the strip
 * kernel for pinned input too. */
int cape_host_results(cape_handle h, const cape_frame_record** records, const int32_t** plane_labels,
                      const int32_t** cyl_labels, const double** boundary);

/* Pinned, device-mapped host memory for depth frames (hipHostMalloc / hipHostRegister on the handle's device).  When
 * cape_extract_host is given such a buffer, batches of up to 8 frames are read by the streaming kernel straight from host
 * memory (the image is read exactly once: the PCIe transfer is the kernel's input stream, no staging copy); larger
 * batches take one DMA.  A registered range must stay allocated until it is unregistered. */
int cape_host_alloc(cape_handle h, uint64_t bytes, void** out);
int cape_host_free(cape_handle h, void* p);
int cape_host_register(cape_handle h, void* p, uint64_t bytes);
int cape_host_unregister(cape_handle h, void* p);

/* Debug / parity: per-cell stats of one frame of the last batch (synchronous). */
int cape_copy_cell_stats(cape_handle h, int32_t frame, cape_cell_stats* cells_out);

/* Debug / parity: the seed cells of one frame of the last batch in the order grow_planes_and_cylinders tried them
 * (primitive_detection.cpp:277-307; header.n_seeds of them, at most `capacity` are copied, *n_out = header.n_seeds).
 * Synchronous. */
int cape_copy_seed_sequence(cape_handle h, int32_t frame, int32_t* seeds_out, int32_t capacity, int32_t* n_out);

/* show_statistics (primitive_detection.hpp:46-49): stage timings from HIP events recorded on the caller's stream
 * around each kernel of every cape_extract made while timing is enabled.  cape_get_timings synchronises the
 * pending events, folds them into the running sums and returns the sums; cape_reset_timings zeroes them. */
int cape_enable_timing(cape_handle h, int32_t enable);
int cape_get_timings(cape_handle h, cape_timings* out);
/* the same for a caller compiled against another revision of cape_timings: writes min(out_bytes, sizeof(cape_timings)) bytes */
int cape_get_timings_sized(cape_handle h, void* out, uint64_t out_bytes);
int cape_reset_timings(cape_handle h);

/* Debug / parity: evaluate device scalar math (f64 sqrt / div, ocml acos / atan2, the eigen-solver and plane fit)
 * on host operands so tests can compare gfx950 results with the CPU oracle bit for bit.  `a`,`b`,`out` are HOST
 * pointers; EIGEN3: a = n x 6 (m00 m10 m11 m20 m21 m22), out = n x 12 ; FIT_PLANE: a = n x 10 (9 sums, count),
 * out = n x 10 (normal[3], d, centroid[3], mse, score, planar).  The covariance algebra of cape_map_measure, one row of `a` per
 * case: COV_VALID: a = n x 17 (size 3 or 4, then the matrix row-major in the first size x size of 16 entries), out = n x 1 (0 / 1) ;
 * PLANE_COV: a = n x 13 (normal[3], d, cov[9]), out = n x 17 (ok, then 16 entries) ; WORLD_PLANE_COV: a = n x 45 (normal[3], d,
 * camera_to_world[16], plane covariance[16], pose covariance[9]), out = n x 17 (ok, then 16 entries; all 0 when ok is 0).  The
 * algebra of cape_map_kalman: KALMAN: a = n x 40 (x[4], P[16], z[4], R[16]), out = n x 21 (the KalmanStatus of
 * host/map_tracking.hpp, then x'[4] and P'[16]; zeros unless the status is 0) ; PLANE_FRAME: a = n x 3 (normal), out = n x 7 (ok of
 * get_plane_coordinate_system's norm check, then x axis and y axis; zeros unless ok). */
enum
{
    CAPE_DEBUG_SQRT = 0, CAPE_DEBUG_DIV = 1, CAPE_DEBUG_ACOS = 2, CAPE_DEBUG_ATAN2 = 3, CAPE_DEBUG_QUANT = 4,
    CAPE_DEBUG_SQRTF = 5, CAPE_DEBUG_EIGEN3 = 6, CAPE_DEBUG_FIT_PLANE = 7, CAPE_DEBUG_COV_VALID = 8, CAPE_DEBUG_PLANE_COV = 9,
    CAPE_DEBUG_WORLD_PLANE_COV = 10, CAPE_DEBUG_KALMAN = 11, CAPE_DEBUG_PLANE_FRAME = 12
};
int cape_debug_eval(int op, const double* a, const double* b, double* out, int n);
/* Debug: shader-clock ticks spent per phase of the grow kernel, n_frames x 32 (all zero unless the library was built
 * with -DCAPE_B_PROFILE).  Synchronises. */
int cape_debug_cycles(cape_handle h, int32_t n_frames, unsigned long long* out);
/* frames of the last cape_rectify_depth that its band kernel handed to the general kernels (tests; synchronises) */
int cape_debug_rectify_flagged(cape_handle h, int32_t* count);
/* the task queue of the last cape_build_polygons (tests; synchronises): slots reserved by spawned tasks and quit marks, tickets
 * taken, and the slots the call could use.  reserved > slots means the queue overflowed and waves walked rungs they could not
 * enqueue -- impossible in the shipped library (the queue holds every task a batch can spawn), forced by a test build. */
int cape_debug_polygon_queue(cape_handle h, uint32_t* reserved, uint32_t* tickets, uint32_t* slots);
/* the work lists of the last cape_match_polygons (profiling; synchronises): 32 words -- [0..3] pairs each capacity tier of the
 * intersection kernel was handed, [8 + 4 * tier + reason] pairs that left tier `tier` for a larger one because of reason 1 = ring
 * vertices, 2 = slab boundaries, 3 = edges over one slab */
int cape_debug_match_lists(cape_handle h, uint32_t* words32);
/* the same for the last map-matcher call -- cape_match_map, cape_match_map_wide or cape_match_map_shards, whichever came last
 * (tests; synchronises): 8 words -- [0..1] the (frame, map plane, detected plane) triples the gate kernel reserved (64-bit), [2..4]
 * the pairs handed to capacity tiers 1, 2 and 3 of the intersection kernel, [5..7] the tickets the waves of those tiers drew.  All
 * zero before the first such call. */
int cape_debug_map_match_lists(cape_handle h, uint32_t* words8);
/* cape_map_union's per-pair device function on a one-pair launch (tests; synchronous; the results of the last cape_map_union are not
 * disturbed): how disjoint operands, containment, T-junctions and capacity overflows -- pairs the matcher would never make -- reach
 * the kernel.  All pointers are HOST pointers.  ring_a plays the map plane's outer ring (n_a vertices, (x, y) pairs), ring_b the
 * detection's world ring; frames27 = (x_axis, y_axis, center) of ring a's frame, of ring b's frame and of the target (fusion) frame,
 * NULL = the canonical frame (1,0,0), (0,1,0), (0,0,0) for all three.  row_out: one cape_plane_union (map_plane = 0); vertices_out:
 * room for CAPE_MAP_MAX_RING (x, y) pairs.  CAPE_ERR_INVALID_ARGUMENT: NULL handle, ring or output, n_a or n_b outside [3, 4096]. */
int cape_debug_ring_union(cape_handle h, const double* ring_a, int32_t n_a, const double* ring_b, int32_t n_b, const double* frames27,
                          cape_plane_union* row_out, double* vertices_out);
/* The same for cape_map_union_holes' per-pair function.  rings_a: ring a's outer ring and its interior rings back to back, counts_a
 * their n_rings_a lengths; rings_out: one cape_plane_union_rings; vertices_out: room for CAPE_MAP_UNION_FRAME_VERTICES (x, y) pairs,
 * the served polygon's rings back to back.  CAPE_ERR_INVALID_ARGUMENT: a NULL argument (frames27 may be NULL), n_rings_a outside
 * [1, 1 + CAPE_MAP_MAX_HOLES], a count or n_b outside [3, 4096].  Twin: cape_host_polygon_union. */
int cape_debug_polygon_union(cape_handle h, const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                             const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out);
/* The same for cape_map_union_cut's per-pair function: the arguments, outputs and error codes of cape_debug_polygon_union.  Twin:
 * cape_host_polygon_union_cut. */
int cape_debug_polygon_union_cut(cape_handle h, const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b,
                                 int32_t n_b, const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out,
                                 double* vertices_out);

/* The seed of the reference's random engine (src/utils/random.hpp:59-64): 0 under MAKE_DETERMINISTIC -- the default here, and the
 * mode BASELINE.json's bit-exactness is stated for --, `std::time(0)` taken once at process start otherwise.  The engine is
 * thread_local and find_primitives runs on a fresh thread per frame (rgbd_slam.cpp:291), so EVERY frame restarts the sequence at
 * the seed: the handle keeps the first 40 000 doubles of mt19937(seed) + uniform_real_distribution on the device and this call
 * regenerates them (it waits for the handle's work in flight).  A caller that wants the reference's non-deterministic build passes
 * its own time(0). */
int cape_set_rng_seed(cape_handle h, uint32_t seed);

/* outputs::log / log_warning / log_error of the path (the reference's src/outputs/logger.hpp), for a caller that wants the
 * reference's own lines: level 0 = log, 1 = log_warning, 2 = log_error.  The messages find_primitives prints on the hot path,
 *   "Could not find a single plane segment: invalid seed"                      (warning, primitive_detection.cpp:302)
 *   "Plane segment is not planar after merge"                                  (log, :374 and :497; once per occurrence)
 *   "Could not find a correct boundary polygon, rejecting plane segment"       (warning, :618: a planar merge root with fewer than
 *                                                                               three boundary points)
 * are decided on the device and travel in the frame record (CAPE_FRAME_INVALID_SEED, CAPE_FRAME_NOT_PLANAR_COUNT, the segments'
 * boundary counts); the callback gets them when a batch's records first reach the host -- cape_copy_results with a records
 * pointer, or cape_host_results -- once per extracted batch, frame by frame, on the calling thread.  The library's own
 * capacity warnings (CAPE_FRAME_*_OVERFLOW) come the same way.  (:631 "Polyfit error" belongs to the polygon constructor:
 * a consumer of cape_copy_polygons sees CAPE_POLY_REJECTED.)  fn == NULL removes the callback; nothing is ever printed. */
typedef void (*cape_log_fn)(int32_t level, const char* message, int32_t frame, void* user);
int cape_set_log_callback(cape_handle h, cape_log_fn fn, void* user);
/* The same lines for records the caller holds (HOST memory, e.g. out of cape_copy_results): no handle, no device.  Returns the
 * number of lines (>= 0) or a negative cape_status. */
int cape_log_records(const cape_frame_record* records, int32_t n_frames, cape_log_fn fn, void* user);

const char* cape_last_error(void);
const char* cape_version(void);
/* CAPE_ABI_VERSION of the library that was loaded: a binding compares it with the header it was built against before anything else */
int32_t cape_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CAPE_HIP_H */
