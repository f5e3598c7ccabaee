// C ABI of libcape_hip (see include/cape_hip.h), host side only.  This file: handle creation / destruction, the debug knobs,
// version and error reporting, the log callback, timings, host memory and streams.  The other entry points live in
// cape_api_extract.hip (extraction and its results), cape_api_gather.hip (packing and RCCL), cape_api_geometry.hip (rectify,
// matching between frames, polygons), cape_api_map_match.hip (the device map and the calls that read it), cape_api_map_update.hip
// (the calls that change it) and cape_api_debug.hip.  The handle itself is in cape_handle.h, what the map's files share in
// cape_api_map.h.
// There is no CPU fallback: without a HIP device cape_create fails with CAPE_ERR_NO_DEVICE.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "cape_handle.h"

using namespace cape::abi;

namespace {

thread_local std::string g_lastError; // written by fail() only, whichever API file raises the error

// RANSAC draws a frame can ask for (the table of the first draws of mt19937(seed) the handle keeps on the device): a run_ransac_loop
// takes at most 43 x 3 draws and every loop but a region's last removes at least six cells (cylinder_segment.cpp:154), so a frame of
// C cells runs at most C / 6 + (regions <= C / 6) loops: 43 C draws bound it.  40 000 covers the 640 x 480 grid's 33 024 as before.
constexpr int kRngTableMin = 40000;
int rng_table_size(int cells) { const int need = 43 * cells + 129; return need > kRngTableMin ? need : kRngTableMin; }

// utils::Random (src/utils/random.hpp:17-30, :59-64): the first kRngTable doubles of mt19937(seed) + uniform_real_distribution(0, 1)
// (libstdc++ on the host = the reference's own generator)
std::vector<double> rng_table(uint32_t seed, int count)
{
    std::vector<double> rng((size_t)count);
    std::mt19937 engine(seed);
    std::uniform_real_distribution<double> dist(0.0, 1.0);
    for (auto& v : rng)
        v = dist(engine);
    return rng;
}

// Matrix3d::inverse as Eigen evaluates it (cofactor method); for K = [[fx,0,cx],[0,fy,cy],[0,0,1]] this yields
// k00 = fy*invdet, k02 = -(cx*fy)*invdet, k11 = fx*invdet, k12 = -(fx*cy)*invdet with invdet = 1/(fx*fy)
// (reference src/coordinates/point_coordinates.cpp:79-83, Parameters::get_camera_1_intrinsics parameters.hpp:144-149)
void inverse_intrinsics(double fx, double fy, double cx, double cy, double& k00, double& k02, double& k11, double& k12)
{
    const double m[3][3] = {{fx, 0.0, cx}, {0.0, fy, cy}, {0.0, 0.0, 1.0}};
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    };
    const double c00 = cof(0, 0), c10 = cof(1, 0), c20 = cof(2, 0);
    const double det = (c00 * m[0][0] + c10 * m[1][0]) + c20 * m[2][0];
    const double invdet = 1.0 / det;
    k00 = c00 * invdet;
    k02 = c20 * invdet;
    k11 = cof(1, 1) * invdet;
    k12 = cof(2, 1) * invdet;
}

// The debug knobs, read once per handle at the top of cape_create (ahead of the device probe); a value they do not know is an
// error, not a silent default.  (CAPE_RECTIFY_BAND / CAPE_RECTIFY_MARGIN are read by each cape_rectify_depth.)
struct Knobs
{
    std::string resume;       // CAPE_RESUME=off|wave|group: off = the round-2 schedule, wave|group forces the resume instance
    bool noResume = false;    // CAPE_RESUME=off or CAPE_NO_RESUME: every handed-over frame is grown again from scratch
    int schedule = 0;         // CAPE_SCHEDULE=two|single: 1 = always two-pass, 2 = always single (cape_handle_s::Chain::forcedSchedule)
    std::string stageA;       // CAPE_STAGE_A=strips|bands (see cape_handle_s::Chain::stripCounters)
    std::string a1;           // CAPE_A1=cells|bands: the instance of the streaming kernel A1 (StageAParams::a1Bands)
    std::string a2;           // CAPE_A2=split|fused: A2 as a launch of its own, or in A1's lanes (StageAParams::a2Fused); unset: fused where eligible
    bool growGeneral = false; // CAPE_GROW=general|fast: general sends every frame through the general instance
    bool pinnedByDma = false; // CAPE_PINNED_INPUT=dma (cape_handle_s::Chain::pinnedByDma)
    int a2WideBatch = 0;      // CAPE_A2_WIDE_BATCH=n: the one-tile stage-A2 instance for batches <= n (cell_plane_threads)
    int generalSlots = 0;     // CAPE_GENERAL_SLOTS=n: scratch slots of the general instance (0: sized by the device)
};

int read_knobs(Knobs& k)
{
    // false if the variable is set to none of `values`; `out` receives its value
    auto one_of = [](const char* name, std::initializer_list<const char*> values, std::string& out) {
        const char* e = std::getenv(name);
        if (!e)
            return true;
        out = e;
        return std::any_of(values.begin(), values.end(), [&](const char* v) { return out == v; });
    };
    std::string schedule, grow;
    if (!one_of("CAPE_RESUME", {"off", "wave", "group"}, k.resume))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_RESUME must be off, wave or group");
    if (!one_of("CAPE_SCHEDULE", {"two", "single"}, schedule))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_SCHEDULE must be two or single");
    if (!one_of("CAPE_STAGE_A", {"strips", "bands"}, k.stageA))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_STAGE_A must be strips or bands");
    if (!one_of("CAPE_A1", {"cells", "bands"}, k.a1))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_A1 must be cells or bands");
    if (!one_of("CAPE_A2", {"split", "fused"}, k.a2))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_A2 must be split or fused");
    if (!one_of("CAPE_GROW", {"general", "fast"}, grow))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_GROW must be general or fast");
    k.noResume = k.resume == "off" || std::getenv("CAPE_NO_RESUME");
    k.schedule = schedule == "two" ? 1 : (schedule == "single" ? 2 : 0);
    k.growGeneral = grow == "general";
    const char* e = std::getenv("CAPE_PINNED_INPUT");
    k.pinnedByDma = e && std::string(e) == "dma";
    if ((e = std::getenv("CAPE_A2_WIDE_BATCH")))
        k.a2WideBatch = std::atoi(e);
    if ((e = std::getenv("CAPE_GENERAL_SLOTS")))
        k.generalSlots = std::max(1, std::atoi(e));
    return CAPE_OK;
}

// the reference's hot-path log lines of one frame, from its record (cape_set_log_callback).  `next`: where the records a frame
// continues in (cape_frame_header::next_record) are found -- null if the caller has none of them at hand
template <typename NextFn> int log_frame(cape_log_fn fn, void* user, const cape_frame_record& r, int frame, NextFn next)
{
    int lines = 0;
    const uint32_t st = r.header.status;
    // grow_planes_and_cylinders comes first in the reference (the seed loop's lines, in the order they fall; only their NUMBER
    // travels in the record), add_planes_to_primitives behind it
    for (uint32_t k = 0; k < CAPE_FRAME_NOT_PLANAR_COUNT(st); ++k, ++lines)
        fn(0, "Plane segment is not planar after merge", frame, user);
    if (st & CAPE_FRAME_INVALID_SEED) // ends the seed loop: the last line of the grow step
        fn(1, "Could not find a single plane segment: invalid seed", frame, user), ++lines;
    // (a chain only ever points FORWARD in the record array -- a spill record's index is beyond the batch's and its successor's beyond
    // its own --, so a zero-filled or damaged link cannot loop)
    int at = frame;
    for (const cape_frame_record* q = &r; q;)
    {
        const int n = q->header.n_plane_segments < CAPE_MAX_PLANES ? q->header.n_plane_segments : CAPE_MAX_PLANES;
        for (int i = 0; i < n; ++i)
        {
            const cape_plane_segment& s = q->segments[i];
            if (s.merge_label == (uint32_t)(i + q->header.segment_base) && s.planar && s.boundary_count < 3)
                fn(1, "Could not find a correct boundary polygon, rejecting plane segment", frame, user), ++lines;
        }
        const int nxt = q->header.next_record;
        q = nxt > at ? next(nxt) : nullptr;
        at = nxt;
    }
    if (st & (CAPE_FRAME_PLANE_OVERFLOW | CAPE_FRAME_CYL_OVERFLOW | CAPE_FRAME_BOUNDARY_OVERFLOW))
        fn(1, "find_primitives: per-frame capacity exceeded, primitive list truncated", frame, user), ++lines;
    return lines;
}

} // namespace

namespace cape::abi {

int fail(int code, const std::string& msg)
{
    g_lastError = msg;
    return code;
}

int fold_timings(cape_handle_s* h)
{
    auto& T = h->timing;
    cape_timings& tm = T.tm;
    if (T.pending == 0 && tm.calls > 0)
        return CAPE_OK; // nothing timed since the last fold: the sums (and the tick slots behind the split) are unchanged
    for (size_t i = 0; i < T.pending; ++i)
    {
        auto& t = T.pool[i];
        CAPE_HIP_TRY(hipEventSynchronize(t.e[3]));
        float a1 = 0, a2 = 0, b = 0;
        CAPE_HIP_TRY(hipEventElapsedTime(&a1, t.e[0], t.e[1]));
        CAPE_HIP_TRY(hipEventElapsedTime(&a2, t.split ? t.e2b : t.e[1], t.e[2]));
        CAPE_HIP_TRY(hipEventElapsedTime(&b, t.e[2], t.e[3]));
        tm.cell_moments_s += a1 * 1e-3;
        tm.cell_plane_s += a2 * 1e-3;
        tm.cell_fit_s += (a1 + a2) * 1e-3;
        tm.grow_s += b * 1e-3;
        tm.total_s += (a1 + a2 + b) * 1e-3;
        tm.frames += (uint64_t)t.frames;
        tm.calls += 1;
    }
    T.pending = 0;
    // the reference's buckets: stage B's event time split by the ticks its waves booked (all timed calls since the last reset)
    tm.reset_s = 0.0;
    tm.init_s = tm.cell_fit_s;
    tm.grow_phase_s = tm.grow_s;
    tm.merge_s = tm.refine_s = 0.0;
    if (T.phaseTicks && tm.calls > 0)
    {
        unsigned long long ticks[4] = {0, 0, 0, 0};
        std::vector<unsigned long long> slots((size_t)h->cfg.max_batch * 4);
        CAPE_HIP_TRY(hipMemcpy(slots.data(), T.phaseTicks, slots.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < slots.size(); ++i)
            ticks[i & 3] += slots[i];
        const double all = (double)ticks[0] + (double)ticks[1] + (double)ticks[2];
        if (all > 0)
        {
            tm.merge_s = tm.grow_s * ((double)ticks[1] / all);
            tm.refine_s = tm.grow_s * ((double)ticks[2] / all);
            tm.grow_phase_s = tm.grow_s - tm.merge_s - tm.refine_s;
        }
    }
    return CAPE_OK;
}

void log_batch(cape_handle_s* h, const cape_frame_record* records, int n)
{
    auto& r = h->res;
    if (!r.logFn || !r.logPending || !records)
        return;
    const int upTo = n < r.lastFrames ? n : r.lastFrames;
    // spill records (frames of more than 64 plane segments) are fetched from the handle's pool when a frame points at one
    cape_frame_record spill;
    auto next = [&](int idx) -> const cape_frame_record* {
        if (idx < h->cfg.max_batch || idx >= h->cfg.max_batch + h->chain.spillRecords)
            return nullptr;
        return copy_out(&spill, r.records, (size_t)idx, 1) == hipSuccess ? &spill : nullptr;
    };
    for (int f = r.logDone; f < upTo; ++f) // every frame of the batch once, whichever copy brings it to the host first
        (void)log_frame(r.logFn, r.logUser, records[f], f, next);
    if (upTo > r.logDone)
        r.logDone = upTo;
    if (r.logDone >= r.lastFrames)
        r.logPending = false;
}

} // namespace cape::abi

extern "C" {

const char* cape_last_error(void) { return g_lastError.c_str(); }
const char* cape_version(void) { return "cape_hip 0.2 (gfx950)"; }
int32_t cape_abi_version(void) { return CAPE_ABI_VERSION; }

int cape_device_count(int32_t* count_out)
{
    if (!count_out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    int ndev = 0;
    *count_out = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(CAPE_ERR_NO_DEVICE, "no HIP device: libcape_hip has no CPU fallback");
    *count_out = ndev;
    return CAPE_OK;
}

int cape_create(const cape_config* cfg, cape_handle* out)
{
    if (!cfg || !out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    // any image the reference's constructor takes (primitive_detection.cpp:26-67: whole cells of 20 px) up to the widths of the
    // index types used here: 16-bit cell numbers (65 535 cells), one stage-A2 tile row per workgroup (256 cells = 5120 px wide)
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->width % CAPE_CELL_SIZE || cfg->height % CAPE_CELL_SIZE || cfg->max_batch <= 0 ||
        cfg->spill_records < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "width/height must be positive multiples of 20; max_batch > 0; spill_records >= 0");
    if (cfg->width / CAPE_CELL_SIZE > 256 || (long long)(cfg->width / CAPE_CELL_SIZE) * (cfg->height / CAPE_CELL_SIZE) > 65535)
        return fail(CAPE_ERR_UNSUPPORTED, "cell grid beyond 256 cells wide (5120 px) or 65 535 cells");
    if (!(cfg->fx > 0) || !(cfg->fy > 0))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "focal lengths must be positive");
    if (cfg->flags & ~(uint32_t)(CAPE_FLAG_CYLINDERS | CAPE_FLAG_ASYNC_SECOND_PASS))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown CAPE_FLAG_* bit in cape_config.flags");
    Knobs knobs;
    if (const int rc = read_knobs(knobs); rc != CAPE_OK)
        return rc;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(CAPE_ERR_NO_DEVICE, "no HIP device: libcape_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    DeviceGuard deviceGuard(cfg->device); // (outlives the handle below: an early return frees it on its device)
    if (deviceGuard.error() != hipSuccess)
        return fail(CAPE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(deviceGuard.error()));
    int ldsLimit = 0;
    CAPE_HIP_TRY(hipDeviceGetAttribute(&ldsLimit, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device));

    std::unique_ptr<cape_handle_s> owner(new (std::nothrow) cape_handle_s());
    if (!owner)
        return fail(CAPE_ERR_HIP, "out of host memory");
    cape_handle_s* h = owner.get();
    auto& c = h->chain;
    auto& r = h->res;
    h->cfg = *cfg;
    h->ldsLimit = ldsLimit;
    {
        hipDeviceProp_t prop;
        h->computeUnits = hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0
                              ? prop.multiProcessorCount
                              : 256;
    }
    h->hCells = cfg->width / CAPE_CELL_SIZE;
    h->vCells = cfg->height / CAPE_CELL_SIZE;
    h->cells = h->hCells * h->vCells;
    h->boundaryCap = cfg->boundary_capacity > 0 ? cfg->boundary_capacity : 2 * h->cells;
    const size_t B = (size_t)cfg->max_batch, C = (size_t)h->cells;
    // beyond "one lane per grid row, two mask words per row" (or the knob CAPE_GROW=general)
    c.generalAll = h->hCells > 128 || h->vCells > 64 || knobs.growGeneral;
    c.spillRecords = cfg->spill_records > 0 ? cfg->spill_records : std::max(8, cfg->max_batch / 8);
    c.rngCount = rng_table_size(h->cells);
    const size_t R = B + (size_t)c.spillRecords; // records / boundary slabs: the batch's, then the spill pool

    CAPE_HIP_TRY(h->acol.alloc(cfg->width));
    CAPE_HIP_TRY(h->brow.alloc(cfg->height));
    CAPE_HIP_TRY(h->ratioCol.alloc(h->hCells));
    CAPE_HIP_TRY(h->ratioRow.alloc(h->vCells));
    CAPE_HIP_TRY(h->rng.alloc((size_t)c.rngCount));
    CAPE_HIP_TRY(h->cellSums.alloc(B * C * cape::kSumStride));
    CAPE_HIP_TRY(h->cellPlane.alloc(B * C * cape::kPlaneStride));
    CAPE_HIP_TRY(h->cellScore.alloc(B * C));
    CAPE_HIP_TRY(h->cellTol.alloc(B * C));
    CAPE_HIP_TRY(h->cellFlags.alloc(B * C));
    CAPE_HIP_TRY(h->cellBins.alloc(B * C));
    CAPE_HIP_TRY(h->cellAux.alloc(B * C));
    CAPE_HIP_TRY(h->cellMse.alloc(B * C));
    CAPE_HIP_TRY(h->seedSeq.alloc(B * C));
    if (cfg->flags & CAPE_FLAG_CYLINDERS)
    {
        CAPE_HIP_TRY(c.cylScratch.alloc(B * C * cape::kCylStride));
        CAPE_HIP_TRY(c.needCylinder.alloc(2 * B + 2));
        if (!knobs.noResume)
        {
            // the list + its cost-class lists (StageBParams::resumeBucketStride), one stride apart
            const size_t words = (1 + cape::kResumeClasses) * (2 * B + 2);
            CAPE_HIP_TRY(c.resumeList.alloc(words));
            CAPE_HIP_TRY(hipMemset(c.resumeList, 0, words * sizeof(uint32_t)));
            CAPE_HIP_TRY(c.growState.alloc(B * cape::grow_state_bytes(h->cells)));
        }
        CAPE_HIP_TRY(c.handedOverHost.alloc_host(2, hipHostMallocDefault));
        c.handedOverHost[0] = c.handedOverHost[1] = 0;
        CAPE_HIP_TRY(c.handedOverReady.ensure());
    }
    CAPE_HIP_TRY(c.redoList.alloc(2 * B + 2));
    CAPE_HIP_TRY(c.spillList.alloc(2 * B + 2));
    CAPE_HIP_TRY(hipMemset(c.spillList, 0, (2 * B + 2) * sizeof(uint32_t)));
    CAPE_HIP_TRY(c.spillCounters.alloc(2));
    CAPE_HIP_TRY(hipMemset(c.spillCounters, 0, 2 * sizeof(uint32_t)));
    if (cfg->max_batch <= kHostResultFrames && cfg->sub_batches <= 1 && knobs.stageA != "bands")
    {
        c.stripsAlways = knobs.stageA == "strips";
        c.pinnedByDma = knobs.pinnedByDma;
        CAPE_HIP_TRY(r.doneCounter.alloc(1));
        CAPE_HIP_TRY(hipMemset(r.doneCounter, 0, sizeof(uint32_t)));
        CAPE_HIP_TRY(c.stripCounters.alloc((size_t)kHostResultFrames));
        CAPE_HIP_TRY(hipMemset(c.stripCounters, 0, kHostResultFrames * sizeof(uint32_t)));
    }
    CAPE_HIP_TRY(h->workDone.ensure());
    if ((cfg->flags & CAPE_FLAG_ASYNC_SECOND_PASS) && (cfg->flags & CAPE_FLAG_CYLINDERS) && cfg->max_batch > kHostResultFrames &&
        cfg->sub_batches <= 1)
    {
        CAPE_HIP_TRY(h->sideStream.ensure());
        CAPE_HIP_TRY(h->sideFork.ensure());
        CAPE_HIP_TRY(h->sideDone.ensure());
    }
    CAPE_HIP_TRY(h->debugCycles.alloc(B * cape::kProfileSlots));
    CAPE_HIP_TRY(hipMemset(h->debugCycles, 0, B * cape::kProfileSlots * 8));
    CAPE_HIP_TRY(h->timing.phaseTicks.alloc(B * 4));
    CAPE_HIP_TRY(hipMemset(h->timing.phaseTicks, 0, B * 4 * 8));
    h->resultsOnHost = cfg->max_batch <= kHostResultFrames;
    CAPE_HIP_TRY(alloc_result(r.records, R, h->resultsOnHost));
    CAPE_HIP_TRY(alloc_result(r.planeLabels, B * C, h->resultsOnHost));
    CAPE_HIP_TRY(alloc_result(r.cylLabels, B * C, h->resultsOnHost));
    CAPE_HIP_TRY(alloc_result(r.boundary, R * (size_t)h->boundaryCap * 3, h->resultsOnHost));
    if (h->resultsOnHost)
    {
        CAPE_HIP_TRY(alloc_result(r.doneFlag, 16, true)); // the completion word, then the spill count of the one-frame chain
        *r.doneFlag = 0;
    }

    // ---- constant tables
    double k00, k02, k11, k12;
    inverse_intrinsics(cfg->fx, cfg->fy, cfg->cx, cfg->cy, k00, k02, k11, k12);
    std::vector<double> acol(cfg->width), brow(cfg->height);
    // transform_screen_to_camera: K^-1[:, :2] * [u v] + K^-1[:, 2] with k01 = k10 = 0
    for (int u = 0; u < cfg->width; ++u)
        acol[u] = (k00 * (double)u + 0.0) + k02;
    for (int v = 0; v < cfg->height; ++v)
        brow[v] = (0.0 + k11 * (double)v) + k12;
    auto ratios = [](const std::vector<double>& t, int ncell) {
        std::vector<float> r(ncell, 1.0f);
        for (int c = 0; c < ncell; ++c)
        {
            double mx = 0.0, mn = 0.0;
            for (int i = 0; i < CAPE_CELL_SIZE; ++i)
            {
                const double a = std::fabs(t[c * CAPE_CELL_SIZE + i]);
                if (a > 0.0)
                {
                    mx = (a > mx) ? a : mx;
                    mn = (mn == 0.0 || a < mn) ? a : mn;
                }
            }
            // rounded up so the device-side guard stays conservative
            r[c] = (mn > 0.0) ? std::nextafter((float)(mx / mn), INFINITY) : 1.0f;
        }
        return r;
    };
    const std::vector<float> rc = ratios(acol, h->hCells), rr = ratios(brow, h->vCells);
    const std::vector<double> rng = rng_table(0u, c.rngCount); // MAKE_DETERMINISTIC's seed; cape_set_rng_seed changes it
    {
        // _Xpre / _Ypre of Depth_Map_Transformation::init_matrices (depth_map_transformation.cpp:156-161)
        std::vector<float> xp(acol.begin(), acol.end()), yp(brow.begin(), brow.end());
        CAPE_HIP_TRY(h->xpre.alloc(xp.size()));
        CAPE_HIP_TRY(h->ypre.alloc(yp.size()));
        CAPE_HIP_TRY(hipMemcpy(h->xpre, xp.data(), xp.size() * sizeof(float), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(h->ypre, yp.data(), yp.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    CAPE_HIP_TRY(hipMemcpy(h->acol, acol.data(), acol.size() * sizeof(double), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(h->brow, brow.data(), brow.size() * sizeof(double), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(h->ratioCol, rc.data(), rc.size() * sizeof(float), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(h->ratioRow, rr.data(), rr.size() * sizeof(float), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(h->rng, rng.data(), rng.size() * sizeof(double), hipMemcpyHostToDevice));
    if (h->resultsOnHost)
        std::memset(r.records, 0, R * sizeof(cape_frame_record));
    else
        CAPE_HIP_TRY(hipMemset(r.records, 0, R * sizeof(cape_frame_record)));

    // ---- kernel parameter blocks
    cape::StageAParams& a = h->pa;
    a.W = cfg->width;
    a.H = cfg->height;
    a.hCells = h->hCells;
    a.vCells = h->vCells;
    a.cells = h->cells;
    a.segsPerRow = (h->hCells + 31) / 32;
    a.bandsPerFrame = h->vCells * a.segsPerRow;
    a.pairsPerFrame = (a.bandsPerFrame + 1) / 2;
    a.acol = h->acol;
    a.brow = h->brow;
    a.ratio_col = h->ratioCol;
    a.ratio_row = h->ratioRow;
    a.cell_sums = h->cellSums;
    a.cell_plane = h->cellPlane;
    a.cell_score = h->cellScore;
    a.cell_tol = h->cellTol;
    a.cell_flags = h->cellFlags;
    a.cell_bins = h->cellBins;
    a.cell_aux = h->cellAux;
    a.cell_mse = h->cellMse;
    // primitive_detection.cpp:189-190 ; parameters.hpp:75 maximumPlaneAngleForMerge_d = 18.0f
    a.sinMerge = sinf(static_cast<float>(18.0f * M_PI / 180.0));
    a.cosMergeA = std::cos(static_cast<double>(18.0f) * M_PI / 180.0); // plane_segment.cpp:324
    a.smallBatchFrames = knobs.a2WideBatch; // see cell_plane_threads()
    a.a1Bands = knobs.a1 == "bands" ? 1 : 0;
    // Stage A in one launch where the lane-per-cell workgroups are A2's tiles; CAPE_A1=bands implies split.  CAPE_A2=fused is a
    // promise about which kernel runs, so whatever would send a call of this handle down the split path is an error here.
    a.a2Fused = (knobs.a2 != "split" && !a.a1Bands && cape::cell_fused_eligible(a)) ? 1 : 0;
    if (knobs.a2 == "fused" && (!a.a2Fused || knobs.a2WideBatch > 0 || cfg->sub_batches > 1))
        return fail(CAPE_ERR_INVALID_ARGUMENT,
                    "CAPE_A2=fused: this handle's grid of " + std::to_string(h->hCells) + " x " + std::to_string(h->vCells) +
                        " cells is not eligible (256 cells per workgroup must be whole cell rows and divide the frame), or CAPE_A1=bands, "
                        "CAPE_A2_WIDE_BATCH or sub_batches > 1 select the split kernels");
    // plane_segment.hpp:33-34 ; parameters.hpp:72 minimumZeroDepthProportion = 0.7f
    a.minZeroPointCount = static_cast<int>(std::floor(static_cast<float>(400) * 0.7f));

    cape::StageBParams& b = h->pb;
    b.W = cfg->width;
    b.H = cfg->height;
    b.hCells = h->hCells;
    b.vCells = h->vCells;
    b.cells = h->cells;
    b.acol = h->acol;
    b.brow = h->brow;
    b.cell_sums = h->cellSums;
    b.cell_plane = h->cellPlane;
    b.cell_score = h->cellScore;
    b.cell_tol = h->cellTol;
    b.cell_flags = h->cellFlags;
    b.cell_bins = h->cellBins;
    b.cell_aux = h->cellAux;
    b.cell_mse = h->cellMse;
    b.records = r.records;
    b.plane_labels = r.planeLabels;
    b.cyl_labels = r.cylLabels;
    b.boundary = r.boundary;
    b.boundaryCapacity = h->boundaryCap;
    b.flags = cfg->flags;
    b.cosMerge = std::cos(static_cast<double>(18.0f) * M_PI / 180.0); // plane_segment.cpp:324
    b.planeSeedCount = static_cast<int>(static_cast<unsigned>((0.8 / 100.0) * h->cells));
    b.minCellActivated = static_cast<int>(static_cast<unsigned>((0.65 / 100.0) * h->cells));
    b.cylScratch = c.cylScratch;
    b.needCylinder = c.needCylinder;
    b.redoList = c.redoList;
    b.spillList = c.spillList;
    b.resumeList = c.resumeList;
    b.resumeBucketStride = c.resumeList ? (uint32_t)(2 * B + 2) : 0u;
    b.growState = c.growState;
    b.growStateStride = (uint32_t)cape::grow_state_bytes(h->cells);
    b.ldsLimitBytes = h->ldsLimit;
    // Parked frames are finished by one WORKGROUP each on the wide grids (1280x960: 0.64 ms against 0.74 ms per 1 024 tunnel
    // frames) and by one WAVEFRONT each on grids up to 32 cells wide, where the lean lone-wave instance keeps four times as
    // many frames in flight and wins (640x480: 0.33 against 0.44 ms per 2 048 tunnel frames, 0.52 against 0.60 ms per 4 096
    // room frames; profiles/r03_cylinder_schedules.txt).  CAPE_RESUME=wave|group forces one (A/B runs, tests).
    b.resumeMode = (h->hCells > 32 && knobs.resume != "wave") || knobs.resume == "group" ? 2 : 1;
    if (!cape::resume_group_fits(b))
        b.resumeMode = 1;
    b.twoPass = c.needCylinder ? 1 : 0;
    if (!c.generalAll && cape::grow_lds_bytes(h->cells, (cfg->flags & CAPE_FLAG_CYLINDERS) != 0, CAPE_MAX_PLANES) > (size_t)h->ldsLimit)
        c.generalAll = true; // (a device with less LDS than the 64-segment instance wants: the general instance needs 20 KB)
    {
        // the general instance: a persistent grid of waves, one scratch slot each (two workgroups per CU hold its 64 KB of LDS; a handle
        // whose frames only reach it through the spill list gets by with fewer)
        const bool cyl = (cfg->flags & CAPE_FLAG_CYLINDERS) != 0;
        cape::GenParams& g = h->gen;
        g.slotBytes = cape::general_slot_bytes(h->cells, h->hCells, h->vCells, cyl, b.minCellActivated, &g.capSeg, &g.capCyl);
        g.ldsBytes = (int)cape::general_lds_bytes(h->cells, h->hCells, h->vCells, cyl, g.capSeg, g.capCyl, h->ldsLimit);
        if (g.ldsBytes <= 0)
            return fail(CAPE_ERR_UNSUPPORTED, "this device offers too little LDS per workgroup for the grow kernels (" + std::to_string(ldsLimit) + " bytes)");
        const int cus = h->computeUnits;
        size_t slots = knobs.generalSlots > 0 ? (size_t)knobs.generalSlots : c.generalAll ? (size_t)2 * cus : (size_t)std::min(cus, 64);
        slots = std::min(slots, B);
        while (slots > 1 && slots * g.slotBytes > ((size_t)2 << 30)) // keep the scratch under 2 GB whatever the grid
            slots /= 2;
        g.scratchSlots = (int)slots;
        CAPE_HIP_TRY(c.genScratch.alloc(slots * g.slotBytes));
        g.scratch = c.genScratch;
        g.spillAlloc = c.spillCounters;
        g.genFrames = c.spillCounters + 1;
        g.poolRecords = r.records + B;
        g.poolBoundary = r.boundary + B * (size_t)h->boundaryCap * 3;
        g.poolCapacity = c.spillRecords;
        g.poolBase = cfg->max_batch;
        g.rowWords = (h->hCells + 63) / 64;
        g.allFrames = c.generalAll ? 1 : 0;
    }
    if (c.needCylinder && !c.generalAll)
        if (const int perCu = cape::grow_waves_per_cu(h->pb); perCu > 0)
            c.cylSlots = perCu * h->computeUnits;
    c.forcedSchedule = knobs.schedule;
    b.debugCycles = h->debugCycles;
    b.phaseTicks = nullptr; // set per launch (launch_chain) while timing is on
    b.seed_sequence = h->seedSeq;
    b.rngTable = h->rng;
    b.rngCount = c.rngCount;
    // cylinder_segment.cpp:132
    b.ransacMaxIterations = static_cast<int>(static_cast<unsigned>(logf(1.0f - 0.8f) / logf(1.0f - powf(0.33f, 3.0f))));

    if (cfg->sub_batches > 1)
    {
        for (auto& st : c.pipeStream)
            CAPE_HIP_TRY(st.ensure());
        CAPE_HIP_TRY(c.pipeFork.ensure());
        for (auto& e : c.pipeJoin)
            CAPE_HIP_TRY(e.ensure());
        c.pipeStage.resize((size_t)cfg->sub_batches);
        for (auto& e : c.pipeStage)
            CAPE_HIP_TRY(e.ensure());
    }
    *out = owner.release();
    return CAPE_OK;
}

void cape_destroy(cape_handle h)
{
    if (!h)
        return;
    DeviceGuard deviceGuard(h->cfg.device);
    (void)drain_handle(h); // nothing of the handle's may still be running on its buffers
    if (h->gather.comm)
        (void)cape::rccl_comm_destroy(h->gather.comm); // the communicator goes first, then every buffer, event and stream
    delete h;
}

int cape_get_layout(cape_handle h, cape_layout* out)
{
    if (!h || !out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    CAPE_ON_DEVICE(h);
    out->compute_units = h->computeUnits;
    out->grow_frames_per_cu = cape::grow_waves_per_cu(h->pb);
    out->h_cells = h->hCells;
    out->v_cells = h->vCells;
    out->cells = h->cells;
    out->boundary_capacity = h->boundaryCap;
    out->frame_record_bytes = sizeof(cape_frame_record);
    out->effective_flags = h->cfg.flags & ~(uint32_t)(h->sideStream ? 0u : CAPE_FLAG_ASYNC_SECOND_PASS);
    out->reserved = 0;
    return CAPE_OK;
}

int cape_stream_create(cape_handle h, void** stream_out)
{
    if (!h || !stream_out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    CAPE_ON_DEVICE(h);
    hipStream_t s = nullptr;
    CAPE_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream_out = s;
    return CAPE_OK;
}

int cape_stream_destroy(cape_handle h, void* stream)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!stream)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h)); // (the handle's event may still refer to work on it)
    CAPE_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    CAPE_HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return CAPE_OK;
}

int cape_host_alloc(cape_handle h, uint64_t bytes, void** out)
{
    if (!h || !out || bytes == 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or zero size");
    CAPE_ON_DEVICE(h);
    *out = nullptr;
    CAPE_HIP_TRY(hipHostMalloc(out, (size_t)bytes, hipHostMallocMapped));
    return CAPE_OK;
}

int cape_host_free(cape_handle h, void* p)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!p)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h)); // a kernel of this handle may still be reading the buffer
    CAPE_HIP_TRY(hipHostFree(p));
    return CAPE_OK;
}

int cape_host_register(cape_handle h, void* p, uint64_t bytes)
{
    if (!h || !p || bytes == 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or zero size");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipHostRegister(p, (size_t)bytes, hipHostRegisterMapped));
    return CAPE_OK;
}

int cape_host_unregister(cape_handle h, void* p)
{
    if (!h || !p)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(hipHostUnregister(p));
    return CAPE_OK;
}

int cape_log_records(const cape_frame_record* records, int32_t n_frames, cape_log_fn fn, void* user)
{
    if (!records || !fn || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null records / callback or negative frame count");
    int lines = 0;
    // (a chain is followed as far as the caller's array reaches: records + pool copied together hold all of it)
    auto next = [&](int idx) -> const cape_frame_record* { return idx >= 0 && idx < n_frames ? records + idx : nullptr; };
    for (int f = 0; f < n_frames; ++f)
        lines += log_frame(fn, user, records[f], f, next);
    return lines;
}

int cape_set_rng_seed(cape_handle h, uint32_t seed)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h)); // a grow kernel in flight may still be drawing from the table
    const std::vector<double> rng = rng_table(seed, h->chain.rngCount);
    CAPE_HIP_TRY(hipMemcpy(h->rng, rng.data(), rng.size() * sizeof(double), hipMemcpyHostToDevice));
    return CAPE_OK;
}

int cape_set_log_callback(cape_handle h, cape_log_fn fn, void* user)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    h->res.logFn = fn;
    h->res.logUser = user;
    return CAPE_OK;
}

int cape_enable_timing(cape_handle h, int32_t enable)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    h->timing.enabled = enable != 0;
    return CAPE_OK;
}

int cape_get_timings(cape_handle h, cape_timings* out)
{
    return cape_get_timings_sized(h, out, sizeof(cape_timings));
}

int cape_get_timings_sized(cape_handle h, void* out, uint64_t out_bytes)
{
    if (!h || !out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    CAPE_ON_DEVICE(h);
    const int rc = fold_timings(h);
    if (rc != CAPE_OK)
        return rc;
    std::memcpy(out, &h->timing.tm, (size_t)std::min<uint64_t>(out_bytes, sizeof(cape_timings)));
    return CAPE_OK;
}

int cape_reset_timings(cape_handle h)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    CAPE_ON_DEVICE(h);
    const int rc = fold_timings(h);
    h->timing.tm = cape_timings{};
    if (h->timing.phaseTicks)
        CAPE_HIP_TRY(hipMemset(h->timing.phaseTicks, 0, (size_t)h->cfg.max_batch * 4 * 8));
    return rc;
}

} // extern "C"
