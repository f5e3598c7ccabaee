// Private header of the C ABI's host side (cape_api*.hip): the handle, the owners of its device resources, the device /
// stream guards of the entry points and the helpers the API files share.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cape_internal.h"
#include "cape_map_commit.h"
#include "cape_map_maintain.h"
#include "cape_map_step.h"
#include "cape_pose_score.h"
#include "cape_pose_solve.h"
#include "cape_pose_covariance.h"

namespace cape {
// every launcher returns the error of its own launch(es) (hipGetLastError right behind hipLaunchKernelGGL)
hipError_t launch_cell_moments(const StageAParams& p, int nFrames, hipStream_t stream);
hipError_t launch_cell_plane(const StageAParams& p, int nFrames, hipStream_t stream);
hipError_t launch_cell_strips(const StageAParams& p, int nFrames, uint32_t* frameCounters, hipStream_t stream);
int cell_plane_threads(const StageAParams& p, int nFrames);
int cell_plane_rows_per_tile(const StageAParams& p, int nFrames);
bool cell_fused_eligible(const StageAParams& p);
hipError_t launch_cell_fused(const StageAParams& p, int nFrames, hipStream_t stream);
hipError_t launch_grow(const StageBParams& p, int nFrames, hipStream_t stream, hipStream_t side, hipEvent_t fork, hipEvent_t done,
                       const GenParams* gen);
hipError_t launch_grow_general(const StageBParams& p, const GenParams& g, int nFrames, hipStream_t stream);
size_t grow_lds_bytes(int cells, bool cylinders, int maxPlanes);
size_t grow_state_bytes(int cells);
bool resume_group_fits(const StageBParams& p);
hipError_t launch_rectify(const RectifyParams& p, int nFrames, int computeUnits, hipStream_t stream);
hipError_t launch_match(const MatchParams& p, int nFrames, hipStream_t stream);
hipError_t launch_pack(const PackParams& p, hipStream_t stream);
hipError_t launch_polygons(const PolygonParams& p, int nFrames, hipStream_t stream);
hipError_t launch_match_polygons(const MatchPolygonParams& p, int nFrames, hipStream_t stream);
hipError_t launch_match_map(const MatchMapParams& p, int nFrames, hipStream_t stream);
hipError_t launch_match_map_wide(const MatchMapParams& p, int nFrames, hipStream_t stream);
hipError_t launch_match_wide(const MatchWideParams& p, int nFrames, hipStream_t stream);
hipError_t launch_carry_save(const CarrySaveParams& p, hipStream_t stream);
hipError_t launch_map_visibility(const MapVisibilityParams& p, int nFrames, hipStream_t stream);
hipError_t launch_map_step_visibility(const MapVisibilityParams& p, const MapTrackState* tracks, hipStream_t stream);
hipError_t launch_map_measure(const MapMeasureParams& p, int nFrames, hipStream_t stream);
hipError_t launch_map_kalman(const MapKalmanParams& p, int nFrames, hipStream_t stream);
hipError_t launch_map_pose_pairs(const PosePairsParams& p, int nFrames, hipStream_t stream); // the pair rows alone (enqueue_pose_pairs)
hipError_t launch_map_pose_score(const PoseScoreParams& p, int nFrames, hipStream_t stream); // the score kernel alone
hipError_t launch_map_pose_solve(const PoseSolveParams& p, int nFrames, hipStream_t stream);
hipError_t launch_map_pose_select(const PoseSelectParams& p, int nFrames, hipStream_t stream);
hipError_t launch_map_pose_covariance_chunk(const PoseCovParams& p, hipStream_t stream); // vary, then the varied solve, of p.chunkFrames frames
hipError_t launch_map_pose_covariance_reduce(const PoseCovParams& p, int nFrames, hipStream_t stream);
hipError_t launch_pose_draw_deviates(uint64_t seed, uint32_t frameIndex, int nIterations, bool uniforms, double* out, hipStream_t stream);
hipError_t launch_map_union(const MapUnionParams& p, int nFrames, hipStream_t stream);
hipError_t launch_ring_union(const RingUnionParams& p, hipStream_t stream);
hipError_t launch_map_union_holes(const MapUnionParams& p, cape_plane_union_rings* ringRows /* frames x 128 */, int nFrames, hipStream_t stream);
hipError_t launch_polygon_union(const PolygonUnionParams& p, hipStream_t stream);
hipError_t launch_map_union_cut(const MapUnionParams& p, cape_plane_union_rings* ringRows /* frames x 128 */, int nFrames, hipStream_t stream);
hipError_t launch_polygon_union_cut(const PolygonUnionParams& p, hipStream_t stream);
hipError_t launch_map_commit(const MapCommitParams& p, int outPlanesBound /* workgroups of the copy kernel */, hipStream_t stream);
hipError_t launch_map_maintain(const MapMaintainParams& p, hipStream_t stream);
hipError_t launch_map_step_maintain(const MapStepParams& s, int planesBound /* workgroups of the copy kernel */, hipStream_t stream);
const char* rccl_load(); // nullptr on success, else the reason
int rccl_unique_id(RcclUniqueId* id);
int rccl_comm_init(void** comm, int world, const RcclUniqueId& id, int rank);
int rccl_comm_destroy(void* comm);
int rccl_all_gather_bytes(const void* send, void* recv, size_t bytes, void* comm, hipStream_t stream);
const char* rccl_error_string(int code);
void rccl_comm_query(void* comm, int* count, int* rank, int* device);
bool rccl_has_gather();
int rccl_gather_bytes(const void* send, void* recv, size_t bytes, int root, void* comm, hipStream_t stream);
hipError_t launch_count_primitives(const cape_frame_record* records, int nFrames, int32_t* out, hipStream_t stream);
hipError_t launch_count_polygon_vertices(const PackParams& p, unsigned long long* totals, hipStream_t stream);
int grow_waves_per_group();
int grow_waves_per_cu(const StageBParams& p);
} // namespace cape

namespace cape::abi {

// ---- owners of the handle's device resources: move-only, and a default-constructed owner holds nothing

// n elements of device memory, or of pinned host memory (the owner remembers which, and frees it the same way)
template <typename T> class Buffer
{
  public:
    Buffer() = default;
    ~Buffer() { reset(); }
    Buffer(Buffer&& o) noexcept { swap(o); }
    Buffer& operator=(Buffer&& o) noexcept { swap(o); return *this; }
    void swap(Buffer& o) noexcept { std::swap(_p, o._p); std::swap(_n, o._n); std::swap(_host, o._host); }

    // whatever the owner held before is freed first
    hipError_t alloc(size_t n) { reset(); return took(hipMalloc(reinterpret_cast<void**>(&_p), n * sizeof(T)), n, false); }
    hipError_t alloc_host(size_t n, unsigned flags) // hipHostMalloc flags: mapped / coherent or not
    {
        reset();
        return took(hipHostMalloc(reinterpret_cast<void**>(&_p), n * sizeof(T), flags), n, true);
    }
    hipError_t ensure(size_t n) { return _p ? hipSuccess : alloc(n); } // device memory on first use
    // grow on demand: reallocated (contents dropped) when smaller than n; `sync` runs first, so that nothing still uses the old one
    template <typename Sync> hipError_t grow(size_t n, Sync sync)
    {
        if (_n >= n)
            return hipSuccess;
        const hipError_t e = sync();
        return e != hipSuccess ? e : alloc(n);
    }
    // the same for device memory whose first `held` elements are kept (the retired log): a new allocation of at least twice the old
    // size, a device copy, a swap
    template <typename Sync> hipError_t grow_keeping(size_t n, size_t held, Sync sync)
    {
        if (_n >= n)
            return hipSuccess;
        hipError_t e = sync();
        if (e != hipSuccess)
            return e;
        Buffer wider;
        e = wider.alloc(n > 2 * _n ? n : 2 * _n);
        if (e == hipSuccess && held > 0)
            e = hipMemcpy(wider._p, _p, held * sizeof(T), hipMemcpyDeviceToDevice);
        if (e == hipSuccess)
            swap(wider);
        return e;
    }
    void reset()
    {
        if (_p)
            (void)(_host ? hipHostFree(_p) : hipFree(_p));
        _p = nullptr;
        _n = 0;
    }

    T* get() const { return _p; }
    operator T*() const { return _p; }
    size_t size() const { return _n; } // elements
    bool on_host() const { return _host; }

  private:
    hipError_t took(hipError_t e, size_t n, bool host)
    {
        _p = e == hipSuccess ? _p : nullptr;
        _n = e == hipSuccess ? n : 0;
        _host = host;
        return e;
    }
    T* _p = nullptr;
    size_t _n = 0;
    bool _host = false;
};

// a result buffer: pinned, device-mapped host memory for the few-frame handles (cape_handle_s::resultsOnHost), else device memory
template <typename T> hipError_t alloc_result(Buffer<T>& b, size_t n, bool onHost)
{
    return onHost ? b.alloc_host(n, hipHostMallocMapped | hipHostMallocCoherent) : b.alloc(n);
}

// copies n elements out of a result buffer: a plain memcpy from pinned host memory, a device-to-host copy otherwise.  The caller
// has settled the work that writes them (settle_results / drain_handle).
template <typename T> hipError_t copy_out(T* dst, const Buffer<T>& src, size_t at, size_t n)
{
    if (!dst || n == 0)
        return hipSuccess;
    if (!src.on_host())
        return hipMemcpy(dst, src.get() + at, n * sizeof(T), hipMemcpyDeviceToHost);
    std::memcpy(dst, src.get() + at, n * sizeof(T));
    return hipSuccess;
}

// an event or a stream, created on first use (ensure) and destroyed with its owner
template <typename H, hipError_t (*Destroy)(H)> class Owned
{
  public:
    Owned() = default;
    ~Owned() { if (_h) (void)Destroy(_h); }
    Owned(Owned&& o) noexcept { std::swap(_h, o._h); }
    Owned& operator=(Owned&& o) noexcept { std::swap(_h, o._h); return *this; }
    operator H() const { return _h; }

  protected:
    H _h = nullptr;
};
struct Event : Owned<hipEvent_t, hipEventDestroy>
{
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return _h ? hipSuccess : hipEventCreateWithFlags(&_h, flags); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy>
{
    hipError_t ensure() { return _h ? hipSuccess : hipStreamCreateWithFlags(&_h, hipStreamNonBlocking); }
};

// Pinned twin of a device buffer: the caller's host data is copied into it before the entry point returns and
// travels from there with an asynchronous copy -- any host pointer, no implicit stream synchronisation.  `fill` writes the
// bytes into the twin once the H2D copy of the previous call has left it.
struct PinnedTwin
{
    Buffer<unsigned char> stage;
    Event free; // recorded behind the H2D copy out of the twin: its next writer waits for it
    bool busy = false;

    template <typename Fill> hipError_t upload(void* dev, size_t bytes, size_t capacity, hipStream_t st, Fill fill)
    {
        hipError_t e = stage ? hipSuccess : stage.alloc_host(capacity, hipHostMallocDefault);
        if (e == hipSuccess)
            e = free.ensure(); // (its own guard: a failed creation must not leave the twin without its event for good)
        if (e == hipSuccess && busy)
            e = hipEventSynchronize(free);
        if (e != hipSuccess)
            return e;
        fill(stage.get());
        if ((e = hipMemcpyAsync(dev, stage, bytes, hipMemcpyHostToDevice, st)) == hipSuccess &&
            (e = hipEventRecord(free, st)) == hipSuccess)
            busy = true;
        return e;
    }
};

// One buffer set of the device map: its planes, rings and vertices, the tracks parallel to the planes and their ids.  The handle
// has three (cape_handle_s::MapSets); they rotate by swapping buffers, so every buffer lives as long as its owner.
struct MapSet
{
    Buffer<cape_map_plane> planes;
    Buffer<cape_map_ring> rings;
    Buffer<double> vertices;       // two doubles per vertex
    Buffer<cape::MapTrackState> tracks; // parallel to the planes
    Buffer<cape::MapTrackTag> tags;     // ... and their id / result, which cape::MapTrackState does not hold

    void swap(MapSet& o) noexcept
    {
        planes.swap(o.planes);
        rings.swap(o.rings);
        vertices.swap(o.vertices);
        tracks.swap(o.tracks);
        tags.swap(o.tags);
    }
    // a destination set takes a map of these sizes (contents dropped where a buffer is replaced; `drain` runs first: a set was the front
    // one of an earlier map, and a call in flight may read it)
    template <typename Sync> hipError_t grow(size_t nPlanes, size_t nRings, size_t nVertices, Sync drain)
    {
        hipError_t e = planes.grow(nPlanes, drain);
        if (e == hipSuccess)
            e = rings.grow(nRings, drain);
        if (e == hipSuccess)
            e = vertices.grow(nVertices * 2, drain);
        if (e == hipSuccess)
            e = tracks.grow(nPlanes, drain);
        if (e == hipSuccess)
            e = tags.grow(nPlanes, drain);
        return e;
    }
};

constexpr int kHostResultFrames = 8; // see cape_handle_s::resultsOnHost

} // namespace cape::abi

struct cape_handle_s
{
    template <typename T> using Buffer = cape::abi::Buffer<T>;
    using Event = cape::abi::Event;
    using Stream = cape::abi::Stream;

    cape_config cfg{};
    int hCells = 0, vCells = 0, cells = 0, boundaryCap = 0;
    int computeUnits = 0; // CUs of the handle's device
    int ldsLimit = 0;     // LDS bytes one workgroup may use on this device (hipDeviceAttributeMaxSharedMemoryPerBlock)
    // handles for a few frames at a time (max_batch <= kHostResultFrames) keep records / label grids / boundary points (and
    // polygons) in pinned, device-mapped HOST memory: the grow kernel's stores go straight over PCIe (posted writes), and reading
    // the results is a wait for the chain's signal + a host memcpy instead of three device-to-host copies
    bool resultsOnHost = false;
    // constants
    Buffer<double> acol, brow;
    Buffer<float> ratioCol, ratioRow;
    Buffer<double> rng; // the RANSAC draw table (rng_table_size doubles)
    Buffer<float> xpre, ypre; // rectify_depth (N3): float copies of the back-projection factors
    // per-frame scratch (stage A -> stage B)
    Buffer<double> cellSums, cellPlane, cellScore, cellMse;
    Buffer<float> cellTol;
    Buffer<uint32_t> cellFlags;
    Buffer<int32_t> cellBins;
    Buffer<cape::CellAux> cellAux;
    Buffer<uint16_t> seedSeq;
    Buffer<unsigned long long> debugCycles;
    cape::StageAParams pa{};
    cape::StageBParams pb{};
    cape::GenParams gen{};

    // the kernel chain and its schedule
    struct Chain
    {
        Buffer<double> cylScratch;
        Buffer<uint32_t> needCylinder; // [0] count, [1..] frames the plane-only pass handed to the cylinder kernel
        Buffer<uint32_t> redoList;     // [0] count, [1..] frames that need more than 32 plane-segment slots
        Buffer<uint32_t> resumeList;   // [0] count, [1..] frames handed to the cylinder kernel WITH their recorded regions
        Buffer<unsigned char> growState; // max_batch x grow_state_bytes(): the parked state of those frames
        // the general grow instance (cape_grow_general.hip): frames of more than 64 plane segments / cylinder labels, every frame of
        // a grid beyond 64 x 64 cells
        Buffer<uint32_t> spillList;     // [0] count, [1..] frames the 64-segment instance handed on
        Buffer<uint32_t> spillCounters; // [0] records handed out of the pool by the call in flight, [1] frames through the general instance
        Buffer<unsigned char> genScratch;
        int spillRecords = 0;    // records of the pool = record indices [max_batch, max_batch + spillRecords)
        bool generalAll = false; // the grid is beyond the fast kernels' 64 x 64 cells: the general instance grows every frame
        int rngCount = 0;        // doubles of the RANSAC draw table (rng_table_size)
        // one-frame handles (max_batch <= kHostResultFrames): stage A runs as ONE launch of strip workgroups (cape_cell_strip_kernel);
        // a counter per frame tells the strip that finishes last.  Empty: the two throughput kernels (debug knob CAPE_STAGE_A=bands)
        Buffer<uint32_t> stripCounters;
        bool stripsAlways = false;  // CAPE_STAGE_A=strips: also when the frame is read over the link (see launch_chain)
        bool inputOverLink = false; // the call in flight reads its frames straight from pinned host memory (cape_extract_host)
        bool pinnedByDma = false;   // debug knob CAPE_PINNED_INPUT=dma: pinned frames take the staging copy as well (A/B of the two routes)
        Buffer<float> depthStage;   // host staging for cape_extract_host (float32 frames; cape_extract_u16_host shares it)
        // schedule feedback: the count of the last two-pass call is copied to pinned host memory behind the kernels and read
        // (never waited for) before the next call.  The cylinder kernel works in rounds of cylSlots resident frames; the
        // plane-only first pass pays off when it saves at least one such round (see launch_chain)
        Buffer<uint32_t> handedOverHost;
        Event handedOverReady;
        int handedOverFrames = 0;        // frames of the call the pending count belongs to (0: nothing pending)
        double handedOverFraction = 0.0; // last measured share of frames that took the cylinder branch
        int cylSlots = 1024;             // frames the cylinder kernel keeps resident on the device (occupancy x CUs)
        bool singlePass = false;
        int callsSinceProbe = 0;
        int forcedSchedule = 0; // debug knob CAPE_SCHEDULE=two|single (read at create): 1 = always two-pass, 2 = always single
        // sub-batch pipelining (cfg.sub_batches > 1)
        Stream pipeStream[2];
        Event pipeFork;
        Event pipeJoin[2];
        std::vector<Event> pipeStage; // one per sub-batch: its moments are done
    } chain;

    // results of the last batch and the one-frame chain's completion signal
    struct Results
    {
        Buffer<cape_frame_record> records; // the batch's, then the spill pool's
        Buffer<int32_t> planeLabels, cylLabels;
        Buffer<double> boundary;
        int lastFrames = 0; // frames of the last cape_extract
        // resultsOnHost: a one-thread kernel behind every chain stores a sequence number into this pinned word; whoever reads
        // the results spins on it instead of going through the runtime's stream synchronisation (wait_results)
        Buffer<uint32_t> doneFlag;
        Buffer<uint32_t> doneCounter; // device: the one-frame chain's grow kernel counts its waves out and stores the number itself
        uint32_t doneSeq = 0;         // sequence number of the last chain enqueued
        bool doneArmed = false;       // a chain with a signal behind it is (or was) in flight
        // one-frame chain: the general grow instance is enqueued by whoever waits for the results, and only if the chain's last wave
        // reported frames on the spill list (doneFlag[1], StageBParams::spillHost); the chain's parameters are kept for that launch
        bool lazySpillArmed = false;
        int lazySpillFrames = 0;
        cape::StageBParams lazySpillParams{};
        // cape_set_log_callback
        cape_log_fn logFn = nullptr;
        void* logUser = nullptr;
        bool logPending = false; // a batch has been extracted whose records have not been through the callback yet
        int logDone = 0;         // ... frames [0, logDone) of it have (a cape_copy_results of fewer frames than the batch delivers the rest later)
    } res;

    // timing: one event set per timed chain, folded lazily by cape_get_timings
    struct Timing
    {
        struct Events
        {
            Event e[4];
            Event e2b; // start of the A2 kernel when it runs on another stream than A1 (pipelined mode)
            int frames = 0;
            bool split = false;
        };
        std::vector<Events> pool; // created on demand, reused
        size_t pending = 0;       // sets [0, pending) hold unread measurements
        bool enabled = false;
        cape_timings tm{};
        Buffer<unsigned long long> phaseTicks; // max_batch x 4 u64: ticks in grow / merge / refine of the timed calls (StageBParams::phaseTicks)
    } timing;

    // multi-GPU gather: two packed staging slots, the RCCL communicator and its stream
    struct Gather
    {
        cape_gather_config cfg{};
        cape_gather_layout layout{};
        cape_gather_polygon_layout polygonLayout{}; // CAPE_GATHER_POLYGONS: the appended sections (all zero without the flag)
        Buffer<unsigned char> ringScratch;          // ... and the pack kernels' scratch (ring_scratch_bytes)
        Buffer<unsigned char> packed[2];
        Event packedFree[2]; // recorded behind the gather that read the slot
        bool packedBusy[2] = {false, false};
        int packSlot = 1; // slot filled by the last cape_pack_primitives
        Event packReady;
        void* comm = nullptr;
        int commRank = 0, commWorld = 0;
        Stream commStream;
        Event done;
        bool pending = false;
        Buffer<int32_t> countScratch; // cape_count_primitives
        Buffer<unsigned long long> vertexCountScratch; // cape_count_polygon_vertices
    } gather;

    // rectify_depth (N3): a flag per frame, then the count + list of flagged frames (2 F + 1 words for F frames)
    Buffer<unsigned> rectFlags;
    // plane matching between consecutive frames (N2): max_batch x cape_frame_match, allocated on first use
    Buffer<cape_frame_match> matches;

    // N1 on the device: polygons of the last batch, and the matches between them (allocated on first use)
    struct Polygons
    {
        Buffer<cape_polygon> polygons;   // pinned host memory when resultsOnHost (it follows the records), else device memory
        Buffer<double> vertices;
        Buffer<unsigned char> ladder; // scratch of the polygon kernels: work lists, state words, parking area (polygon_scratch_bytes)
        int frames = 0;          // frames of the last cape_build_polygons (0: none for the current batch)
        int matchFrames = 0;     // frames of the last cape_match_polygons (0: none for the current batch)
        Buffer<double> poses;    // cape_match_polygons_pose: max_batch x 16 doubles
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_frame_match_exact> matches;
        Buffer<unsigned> lists; // counters (padded to 64 entries) + 4 lists of max_batch x 256 pairs
    } poly;

    // cape_match_polygons_wide: consecutive frames of up to CAPE_MATCH_WIDE_MAX_PLANES kept planes over their record chains.  Results
    // and work buffers of its own, allocated on first use (the work list and the area table grown on demand behind drain_handle):
    // cape_match_polygons' state above is not touched
    struct WideMatch
    {
        Buffer<double> poses; // max_batch x 16 doubles
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_frame_match_wide> frames; // max_batch
        Buffer<int32_t> match;                // max_batch x 128 match, then as many seg_prev, then seg_cur
        Buffer<uint2> kept;                   // max_batch x 128: MatchWideParams::kept
        Buffer<double> areas;                 // CAPE_MATCH_MAP_AREAS: frames x 128 x 128 of the call
        Buffer<unsigned char> work;           // counters, frame ranges, work list, its areas, the tier lists (map_work_layout without mask words)
        int matchFrames = 0;                  // frames of the last cape_match_polygons_wide (0: none for the current batch)
        bool matchAreas = false;              // ... and whether it kept the dense table
    } wide;

    // cape_match_carry_save: the carried frame, what cape_match_polygons_wide(CAPE_MATCH_CARRY) reads as the predecessor of frame 0.
    // Device memory (also on a one-frame handle), allocated on the first save; only the save kernel writes it, so it survives every
    // other call on the handle
    struct Carry
    {
        Buffer<cape_match_carry_info_t> info; // the save kernel's description of the frame
        Buffer<double> planes;                // 128 x 4: out_normal, d
        Buffer<int32_t> segs;                 // 128
        Buffer<cape_polygon> polygons;        // 128, vertex_offset rebased into `vertices`
        Buffer<double> vertices;              // 128 x min(kPolyMaxPoints, boundaryCap) x 2: the rings back to back
        bool saved = false;                   // a frame is carried (cape_match_carry_clear: none)
    } carry;

    // The device map (cape_map_upload, cape_map_upload_tracks) and what changes it (cape_map_commit, cape_map_maintain, cape_map_step):
    // three buffer sets and the sizes of the FRONT one, the map every call reads.  `back` is the destination of a commit or a
    // maintenance, swapped with the front set once the call's header says DONE; `third` is what the maintenance behind a step's commit
    // writes, since the commit's source (front) and destination (back) are both live until the one wait of that call.  The sets
    // rotate: after a step whose maintenance is DONE the third set is the front one and the old front one the third.  The front
    // set is sized at upload; a destination is grown behind drain_handle before the first launch, contents dropped.
    struct MapSets
    {
        cape::abi::MapSet front, back, third;
        int n = -1;              // planes of the front set's map (-1: none uploaded yet)
        int nRings = 0;          // ... its rings and vertices
        long long nVertices = 0;
        int tracksN = -1;        // tracks current for that map (-1: none since cape_map_upload)
    } maps;

    // N2 against the map (cape_match_map): results and work buffers, allocated on first use
    struct Map
    {
        Buffer<unsigned char> poses; // the poses of the call (frames x 16 doubles), then its skip words
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_frame_map_match> frames; // max_batch
        Buffer<int32_t> match;               // max_batch x CAPE_MAP_MAX_PLANES
        Buffer<double> areas;                // CAPE_MATCH_MAP_AREAS: frames x n_map x CAPE_MAX_PLANES of the call
        Buffer<unsigned char> work;          // counters, frame ranges, gate masks, work list, its areas, the tier lists (map_work_layout)
        int matchFrames = 0;                 // frames of the last cape_match_map (0: none for the current batch)
        int matchN = 0;                      // map planes of that call
        bool matchAreas = false;             // ... and whether it kept the dense table
    } map;

    // cape_match_map_wide: the uploaded map against frames of up to CAPE_MATCH_MAP_WIDE_MAX_PLANES kept planes over their record
    // chains.  Results and work buffers of its own, allocated on first use (the work list and the area table grown on demand behind
    // drain_handle): cape_match_map's state above is not touched
    struct MapWide
    {
        Buffer<unsigned char> poses; // the poses of the call (frames x 16 doubles), then its skip words
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_frame_map_match_wide> frames; // max_batch
        Buffer<int32_t> match;                    // max_batch x CAPE_MAP_MAX_PLANES
        Buffer<int32_t> planes;                   // max_batch x 128 seg_cur, then as many map_of
        Buffer<uint2> kept;                       // max_batch x 128: MatchMapParams::keptIndex of the chain source
        Buffer<double> areas;                     // CAPE_MATCH_MAP_AREAS: frames x n_map x 128 of the call
        Buffer<unsigned char> work;               // map_work_layout with two mask words per map plane
        int matchFrames = 0;                      // frames of the last cape_match_map_wide (0: none for the current batch)
        int matchN = 0;                           // map planes of that call
        bool matchAreas = false;                  // ... and whether it kept the dense table
    } mapWide;

    // cape_match_map_shards: the uploaded map against gathered shards.  Results and work buffers of its own, sized by the call's
    // slots and grown on demand behind drain_handle -- nothing here depends on max_batch or on the batch of the last cape_extract,
    // and cape_match_map's state above is not touched
    struct ShardMatch
    {
        Buffer<unsigned char> poses; // the poses of the call (slots x 16 doubles), then its skip words
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_frame_map_match> frames; // slots
        Buffer<int32_t> match;               // slots x n_map
        Buffer<uint2> kept;                  // slots x CAPE_MAX_PLANES: MatchMapParams::keptIndex
        Buffer<double> areas;                // CAPE_MATCH_MAP_AREAS: slots x n_map x CAPE_MAX_PLANES
        Buffer<unsigned char> work;          // map_work_layout
        int slots = 0;                       // slots of the last cape_match_map_shards (0: none yet)
        int matchN = 0;                      // map planes of that call
        bool matchAreas = false;             // ... and whether it kept the dense table
    } shardMatch;

    // cape_debug_map_match_lists: whose work buffer holds the counters of the last map-matcher call (they start the buffer:
    // map_work_layout) -- none yet, cape_match_map's, cape_match_map_wide's or cape_match_map_shards'
    enum LastMapMatcher { kNoMapMatch, kMapMatchRecords, kMapMatchWide, kMapMatchShards } lastMapMatcher = kNoMapMatch;

    // cape_map_visibility: the skip words of the uploaded map seen from the poses of the last call, for cape_match_map[_shards] with
    // CAPE_MATCH_MAP_DEVICE_SKIP.  Buffers of its own, sized by the call's frames (or slots) and grown on demand behind drain_handle:
    // no other call writes them
    struct Visibility
    {
        Buffer<unsigned char> poses; // the poses of the call (frames x 16 doubles), then the moving words
        cape::abi::PinnedTwin posesTwin;
        Buffer<uint32_t> skip;       // frames x ceil(n / 32)
        Buffer<unsigned char> work;  // counters, work list, tier lists (visibility_work_layout)
        int frames = 0;              // frames of the last cape_map_visibility on the current map (0: none since cape_map_upload)
        int n = 0;                   // map planes of that call
    } visibility;

    // cape_map_measure: the measurement half of the map update for the kept planes of the last call's frames.  Device memory of its
    // own, allocated on the first call: a row of CAPE_MAX_PLANES measurements and a world-vertex slab per record (the batch's, then the
    // spill pool's), like the polygons they index.  No other call writes them
    struct Measure
    {
        Buffer<double> poses; // the call's camera-to-world matrices (frames x 16), then its pose covariances (frames x 9)
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_plane_measurement> rows; // records x CAPE_MAX_PLANES
        Buffer<double> vertices;             // records x boundary capacity x 2
        int frames = 0;                      // frames of the last cape_map_measure (0: none for the current batch's polygons)
    } measure;

    // Per-handle scratch (depth staging, rectify keys, hand-over feedback, result buffers) is reused from call to call
    // without per-buffer events: ONE stream is in flight per handle.  Every enqueueing call leaves a handle-owned event
    // behind its work (StreamScope); a call that arrives on ANOTHER stream makes that stream wait for the event
    // (hipStreamWaitEvent: no host block, and the previous stream's handle is never touched again -- the caller may have
    // destroyed it).  lastStream is only compared, never dereferenced.
    hipStream_t lastStream = nullptr;
    bool hasLastStream = false;
    int scopeDepth = 0; // nesting of entry points (StreamScope)
    Event workDone;     // recorded behind the last enqueued work of this handle
    bool workRecorded = false;
    // CAPE_FLAG_ASYNC_SECOND_PASS: the cylinder second pass runs on the handle's own stream; whoever touches the handle next
    // (any entry point, cape_destroy) first waits for sideDone
    Stream sideStream;
    Event sideFork, sideDone;
    bool sidePending = false;

    // cape_map_kalman: the state half of the map update for the frames of the last call, on the front set's tracks.  Result buffers
    // of its own, grown on demand behind drain_handle: no other call writes them.
    struct Kalman
    {
        bool matchedThisMap = false;              // a cape_match_map_wide has run since the last cape_map_upload
        Buffer<cape_frame_map_kalman> frames;     // frames of the call
        Buffer<cape_plane_fusion> rows;           // frames x 128
        Buffer<cape_map_track_result> trackResults; // frames x n_map of the call
        int kalmanFrames = 0;                     // frames of the last cape_map_kalman (0: none for the current batch, map, match and measurements)
        int kalmanN = 0;                          // map planes of that call
        unsigned runs = 0;                        // cape_map_kalman calls that launched: what cape_map_union's results belong to
    } kalman;

    // cape_map_union: the polygon half of the map update for the frames of the last call.  Result buffers of its own, grown on demand
    // behind drain_handle: no other call writes them.
    struct Union
    {
        Buffer<cape_plane_union> rows; // frames x 128
        Buffer<double> vertices;       // frames x CAPE_MAP_UNION_FRAME_VERTICES x 2
        int unionFrames = 0;           // frames of the last cape_map_union (0: none)
        unsigned kalmanRun = 0;        // Kalman::runs when it ran: a later cape_map_kalman invalidates the results
    } mapUnion;

    // cape_map_union_holes and cape_map_union_cut: the rings table beside mapUnion's rows and slab, which either call writes too.
    struct UnionRings
    {
        Buffer<cape_plane_union_rings> rows; // frames x 128
        bool current = false;                // mapUnion's rows are those of one of these two calls: the table belongs to them
    } mapUnionRings;

    // cape_map_commit: the call's plan and header.  Its destination is MapSets::back.
    struct MapCommit
    {
        Buffer<cape::CommitPlanRow> plan;          // CAPE_MAP_MAX_PLANES rows
        Buffer<cape_map_commit_result> header;     // device memory: the plan kernel's, read by the copy kernel
        Buffer<cape_map_commit_result> headerHost; // pinned: the header comes back through it before the call returns
    } mapCommit;

    // cape_map_maintain / cape_map_retired_*: the retired log -- the lost planes in a map's layout, offsets relative to these arrays --
    // and the call's plan and header.  Its destination is MapSets::back.  The log outlives every map: only
    // cape_map_retired_clear empties it.  Its arrays are grown behind drain_handle before the launch, their contents kept.
    struct MapMaintain
    {
        Buffer<cape_map_plane> planes;
        Buffer<cape_map_ring> rings;
        Buffer<double> vertices;
        Buffer<cape_map_track> tracks;
        int nPlanes = 0, nRings = 0; // what the log holds
        long long nVertices = 0;
        Buffer<cape::MaintainPlanRow> plan;           // CAPE_MAP_MAX_PLANES rows
        Buffer<cape_map_maintain_result> header;     // device memory: the plan kernel's, read by the copy kernel
        Buffer<cape_map_maintain_result> headerHost; // pinned: the header comes back through it before the call returns
    } mapMaintain;

    // cape_map_step: the two headers of the call side by side, so that one copy brings both back.  Its maintenance writes
    // MapSets::third.
    struct MapStep
    {
        Buffer<cape_map_step_result> header;     // device memory: the commit's and the maintenance's plan kernels write their halves
        Buffer<cape_map_step_result> headerHost; // pinned: both headers come back through it before the call returns
    } mapStep;

    // cape_map_step_visible / cape_map_step_skip_words: the skip words the step decided for its frame against the map as it found
    // it, the work buffers of its visibility kernels and their counters' way back.  Buffers of its own -- cape_map_visibility's words
    // are not touched -- grown behind drain_handle before the first launch.
    struct MapStepVisible
    {
        Buffer<uint32_t> skip;         // CAPE_MAP_MAX_PLANES / 32 words
        Buffer<unsigned char> work;    // counters, work list, tier lists (visibility_work_layout) for one frame
        Buffer<unsigned> countsHost;   // pinned: the 16 counters come back through it before the call returns
        int n = -1;                    // map planes the words of the last cape_map_step_visible stand for (-1: none since cape_map_upload)
    } mapStepVisible;

    // The pair rows of the pose stage: what the pairs kernel makes of the batch's records, the front map, its tracks and the last
    // cape_match_map_wide, for cape_map_pose_score, cape_map_pose_solve and cape_map_pose_covariance alike.  Allocated once, for
    // max_batch frames (a wide match covers no more): never reallocated, so the address cape_pose_score_device hands out stays valid.
    // enqueue_pose_pairs (cape_api_pose.h) is their only writer.
    struct PosePairs
    {
        Buffer<int4> frameInfo;             // max_batch: n_pairs, n_invalid, flags, 0
        Buffer<cape_pose_feature> features; // max_batch x 128
        int frames = 0;                     // the rows describe frames [0, frames) (0: none for the current batch, map, tracks and match)
    } posePairs;

    // cape_map_pose_score: the pose hypotheses of the last call and what it made of them.  Buffers of its own, grown on demand behind
    // drain_handle: no other call writes them, and the call writes nothing else but the pair rows.
    struct PoseScore
    {
        Buffer<double> poses; // the poses of the call (frames x hypotheses x 16), unless they are the caller's device memory
        cape::abi::PinnedTwin posesTwin;
        Buffer<cape_pose_score> scores;     // frames x hypotheses
        Buffer<double> residuals;           // CAPE_POSE_SCORE_RESIDUALS: frames x hypotheses x 128 x 7
        int frames = 0;                     // frames of the last cape_map_pose_score (0: none for the current batch, map, tracks and match)
        int hypotheses = 0;                 // hypotheses per frame of that call
        bool keptResiduals = false;         // ... and whether it kept the per-pair table
    } poseScore;

    // cape_map_pose_solve / cape_map_pose_select: the problems of the last solve, what it made of them and the last selection over
    // them.  Buffers of its own, like PoseScore's; the pair rows it reads are posePairs'.
    struct PoseSolve
    {
        Buffer<unsigned char> input; // the call's x0 (frames x problems x 6 doubles), then its subsets (x 4 words), unless device memory
        cape::abi::PinnedTwin inputTwin;
        Buffer<cape_pose_solution> solutions; // frames x problems
        Buffer<double> poses;                 // frames x problems x 16
        Buffer<cape_pose_selection> selection; // frames
        int frames = 0;          // frames of the last cape_map_pose_solve (0: none for the current batch, map, tracks and match)
        int problems = 0;        // problems per frame of that call
        bool fromSelection = false; // ... and whether they came from the selection
        int selectFrames = 0;    // frames of the last cape_map_pose_select (0: none current)
    } poseSolve;

    // cape_map_pose_covariance: the samples of the last call and what it made of them.  Buffers of its own, like PoseSolve's; the pair
    // rows it reads are posePairs'.
    struct PoseCovariance
    {
        Buffer<unsigned char> input; // the call's x (frames x 6 doubles), then its subsets (x 4 words), unless device memory
        cape::abi::PinnedTwin inputTwin;
        Buffer<double> table;        // the call's deviates (iterations x 128 x 4), unless device memory
        cape::abi::PinnedTwin tableTwin;
        Buffer<unsigned char> frameRows;    // frames x cape::PoseCovFrame: x, subset and refusal as the vary kernel resolved them
        Buffer<double> slab;                // the varied planes of a chunk of frames, [frame][128][4][iteration], within `budget` bytes
        Buffer<unsigned char> samples;      // frames x iterations x cape::PoseCovSample
        Buffer<cape_pose_solution> kept;    // CAPE_POSE_COVARIANCE_KEEP_SAMPLES: frames x iterations
        Buffer<cape_pose_covariance> rows;  // frames
        Buffer<double> drawn;               // cape_pose_draw_deviates to host memory: the table on its way
        unsigned long long budget = 0;      // bytes of the slab (0: CAPE_POSE_COVARIANCE_DEFAULT_BUDGET)
        int frames = 0;                     // frames of the last call (0: none for the current batch, map, tracks and match)
        int iterations = 0;                 // iterations per frame of that call
        bool keptSamples = false;           // ... and whether it kept the sample rows
    } poseCovariance;
};

namespace cape::abi {
// What a replaced input of the map update's per-frame results invalidates, for every call that replaces one (the batch's polygons,
// the wide match, the measurements, the map, its tracks): the results of cape_map_kalman -- and with them the unions' -- and those of
// cape_map_pose_score, cape_map_pose_solve, cape_map_pose_select and cape_map_pose_covariance, with the pair rows they share.  (A cape_extract ends the wide match and the measurements themselves: both results are checked against them.)
inline void invalidate_frame_results(cape_handle_s* h)
{
    h->kalman.kalmanFrames = 0;
    h->posePairs.frames = 0;
    h->poseScore.frames = 0;
    h->poseSolve.frames = h->poseSolve.selectFrames = 0;
    h->poseCovariance.frames = 0;
}
} // namespace cape::abi

namespace cape::abi {

int fail(int code, const std::string& msg); // records msg for cape_last_error (the one definition: cape_api.hip) and returns code

#define CAPE_HIP_TRY(expr)                                                                                   \
    do                                                                                                       \
    {                                                                                                        \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            return ::cape::abi::fail(CAPE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

// Every entry point that allocates, copies, launches or synchronises runs with the HANDLE's device current, whatever
// the calling thread had selected (one process may drive several GPUs, torch may leave another device current), and
// gives the caller its device back on the way out.
class DeviceGuard
{
  public:
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&_prev) != hipSuccess)
            _prev = -1;
        _err = (_prev == device) ? hipSuccess : hipSetDevice(device);
        _restore = (_err == hipSuccess) && _prev >= 0 && _prev != device;
    }
    ~DeviceGuard()
    {
        if (_restore)
            (void)hipSetDevice(_prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    hipError_t error() const { return _err; }

  private:
    int _prev = -1;
    hipError_t _err = hipSuccess;
    bool _restore = false;
};

#define CAPE_ON_DEVICE(h)                                                                                    \
    ::cape::abi::DeviceGuard _deviceGuard((h)->cfg.device);                                                  \
    if (_deviceGuard.error() != hipSuccess)                                                                  \
    return ::cape::abi::fail(CAPE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_deviceGuard.error()))

// A one-frame chain may have left the general grow instance to the first reader of its results (Results::lazySpillArmed):
// an entry point that is about to enqueue work on those results settles that first (a host wait -- such handles serve one frame
// at a time, their callers wait for every call anyway).
#define CAPE_SETTLE_RESULTS(h)                                                                               \
    do                                                                                                       \
    {                                                                                                        \
        if ((h)->res.lazySpillArmed)                                                                         \
            if (const int rc_ = ::cape::abi::wait_results(h); rc_ != CAPE_OK)                                \
                return rc_;                                                                                  \
    } while (0)

// ---- shared helpers (cape_api_extract.hip unless noted)
int enter_stream(cape_handle_s* h, hipStream_t st); // orders a call on `st` behind the handle's earlier work
hipError_t drain_handle(cape_handle_s* h);          // everything this handle has enqueued so far is done (host side)
hipError_t sync_handle(cape_handle_s* h);           // drain_handle, or the whole device if the handle has recorded no work
int wait_results(cape_handle_s* h);                 // the last chain's signal (and the lazy general launch behind it)
int settle_results(cape_handle_s* h);               // the batch's results can be read: wait_results or sync_handle
int fold_timings(cape_handle_s* h);                 // cape_api.hip
void log_batch(cape_handle_s* h, const cape_frame_record* records, int n); // cape_api.hip

// Brackets the enqueueing part of an entry point: orders the call behind the handle's earlier work (enter_stream) and,
// on the way out -- whether or not a launch in between failed -- records the handle's event behind what was enqueued.
class StreamScope
{
  public:
    StreamScope(cape_handle_s* h, hipStream_t st) : _h(h), _st(st)
    {
        _outer = h->scopeDepth++ == 0; // an entry point that calls another one (cape_extract_host -> cape_extract) records once
        _rc = _outer ? enter_stream(h, st) : CAPE_OK;
    }
    ~StreamScope()
    {
        --_h->scopeDepth;
        if (_outer && _rc == CAPE_OK && _h->workDone && hipEventRecord(_h->workDone, _st) == hipSuccess)
            _h->workRecorded = true;
    }
    StreamScope(const StreamScope&) = delete;
    StreamScope& operator=(const StreamScope&) = delete;
    int rc() const { return _rc; }

  private:
    cape_handle_s* _h;
    hipStream_t _st;
    int _rc;
    bool _outer;
};

} // namespace cape::abi
