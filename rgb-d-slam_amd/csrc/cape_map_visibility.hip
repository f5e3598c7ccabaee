// The first statement of the Feature_Map::get_matches loop (reference src/map_management/feature_map.hpp:658, :683),
// `if (mapFeature.is_moving() or not mapFeature.is_visible(worldToCamera)) continue;`, for every (frame, map plane) pair: the skip
// words cape_match_map / cape_match_map_shards read.  MapPlane::is_visible (map_primitive.cpp:186-189) sends the map polygon through
// to_camera_space (polygon_coordinates.cpp:135-162), every vertex of its OUTER ring to the screen (get_screen_points :77-100 over
// CameraCoordinate::to_screen_coordinates, point_coordinates.cpp:201-210; holes are not read) and intersects that ring with the
// screen rectangle (is_visible_in_screen_space :120-127, get_static_screen_boundary_polygon utils/polygon.cpp:24-46): visible <=>
// the intersection is not empty, here rings_inter_area(screen ring, rectangle) > 0 with the ring intersection of cape_ring_area.h.
//
//   cape_map_classify_kernel    : one wavefront per frame, lanes over map planes (64 at a time): each lane walks the outer ring of
//        its plane once -- are all screen coordinates finite, and their bounding box.  A ring with a non-finite coordinate is not
//        visible, one whose box misses the rectangle neither (see box_misses_screen); every other plane that is not moving goes to
//        the work list, per frame in j order.  Every bit j < n_map of the frame's words is set here; the next kernel clears the bits
//        of the visible planes.
//   cape_map_classify_one_kernel: the same decision for ONE frame (cape_map_step_visible), spread over the chip: a workgroup per 64
//        map planes (two skip words), a wave per plane at a time, the lanes over the ring's vertices (cape_map_step_visible.h has the
//        ownership rules).  The moving bit comes from the device tracks, not from host words.
//   cape_map_visible_kernel<TIER>: the walk of the list through the capacity tiers (walk_tier, cape_pair_list.h) around one pair's
//        area: the screen ring as ring A, the rectangle as ring B, each oriented like the host class orients an outer ring
//        (orient_ring).  Area > 0: the bit of the pair is cleared.  A pair beyond every tier's capacities is not decided: it counts as
//        visible (a plane visited in vain costs work, a plane skipped in vain loses a match) and is counted.
//
// + - x / and comparisons only, in the order of the host twin cape_host_map_visibility (-ffp-contract=off): the words are compared
// BIT FOR BIT with it (tests/test_gpu_map_visibility.py).  The twin takes no shortcut.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_map_camera.h"
#include "cape_map_step_visible.h"
#include "cape_pair_list.h"
#include "cape_ring_area.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int kVisFrames = 4; // frames (waves) of a classify workgroup

// A ring vertex (a, b) of the camera-space polygon on the screen: get_point_from_plane_coordinates (polygon.cpp:146-166:
// `center + point.x() * xAxis + point.y() * yAxis`, i.e. (c + a x) + b y), then to_screen_coordinates (point_coordinates.cpp:203:
// `1.0 / z() * transform_camera_to_screen(...)`: the reciprocal first, then the product); the handle has no skew
__device__ __forceinline__ double2 screen_vertex(const MapVisibilityParams& p, const CameraFrame& F, double2 q)
{
    const double X = F.nc[0] + q.x * F.nx[0] + q.y * F.ny[0], Y = F.nc[1] + q.x * F.nx[1] + q.y * F.ny[1], Z = F.nc[2] + q.x * F.nx[2] + q.y * F.ny[2];
    const double inv = 1.0 / Z;
    return make_double2(inv * (p.fx * X + p.cx * Z), inv * (p.fy * Y + p.cy * Z));
}

// The one shortcut: the bounding box [minU, maxU] x [minV, maxV] of a screen ring A with finite coordinates lies beside the open
// rectangle B = (1, W-1) x (1, H-1).  rings_inter_area(A, B) is then exactly 0, because it only adds a term for a slab [x0, x1],
// x0 < x1, that an edge of A and an edge of B both span (`a.x <= x0 && b.x >= x1`) and in which their height intervals overlap:
//  * maxU <= 1: an edge of A spans only slabs with x1 <= maxU <= 1, the two non-vertical edges of B (x from 1 to W-1) only slabs
//    with x0 >= 1 -- no slab has x0 < x1 with both.  minU >= W-1 likewise (x0 >= W-1 against x1 <= W-1).  Comparisons of
//    coordinates only: no rounding enters.
//  * maxV <= 1: in a shared slab the heights of B are exactly 1 and H-1 (horizontal edges: 1 + 0 * t), those of A are
//    y_at = a.y + (b.y - a.y) * t with t in [0, 1] (a.x <= xm <= b.x and rounding is monotone), which rounding can lift above
//    max(a.y, b.y) by at most 4 x 2^-53 x max(|a.y|, |b.y|).  The test therefore asks for that slack, generously (2^-50): then
//    every height of A is <= 1, so min(hiA, H-1) <= 1 <= max(loA, 1) and `hi <= lo` drops the pair of intervals.  minV >= H-1
//    likewise.  Coordinates beyond 2^1000 (xm or b.y - a.y could overflow) take the full computation.
// A box the test lets through costs an intersection and nothing else.
__device__ __forceinline__ bool box_misses_screen(const MapVisibilityParams& p, double minU, double maxU, double minV, double maxV)
{
    const double right = p.width - 1.0, top = p.height - 1.0;
    if (maxU <= 1.0 || minU >= right)
        return true;
    const double magU = fmax(fabs(minU), fabs(maxU)), magV = fmax(fabs(minV), fabs(maxV));
    if (!(fmax(magU, magV) <= 0x1p1000))
        return false;
    const double slack = magV * 0x1p-50;
    return maxV + slack <= 1.0 || minV - slack >= top;
}

// map plane j from the frame's camera, one lane: false = certainly not visible (a non-finite screen coordinate, or the shortcut)
__device__ inline bool may_be_visible(const double* Tm, const MapVisibilityParams& p, int j)
{
    const cape_map_plane& M = p.mapPlanes[j];
    const CameraFrame F = camera_frame(Tm, M);
    const cape_map_ring R = p.mapRings[M.ring_first];
    const double2* src = p.mapVertices + R.vertex_offset;
    const int n = (int)R.vertex_count;
    bool finite = true;
    double minU = __builtin_inf(), maxU = -__builtin_inf(), minV = __builtin_inf(), maxV = -__builtin_inf();
    for (int i = 0; i < n; ++i)
    {
        const double2 s = screen_vertex(p, F, to_camera_vertex(Tm, F, src[i]));
        finite = finite && isfinite(s.x) && isfinite(s.y);
        minU = s.x < minU ? s.x : minU;
        maxU = s.x > maxU ? s.x : maxU;
        minV = s.y < minV ? s.y : minV;
        maxV = s.y > maxV ? s.y : maxV;
    }
    return finite && !box_misses_screen(p, minU, maxU, minV, maxV);
}

// the minimum / maximum of the 64 lanes' doubles, uniform: comparisons only, so for finite values the order of the reduction does not
// show (a -0 against a +0 may come out either way; box_misses_screen compares and takes magnitudes, where the two are one value)
template <bool MAX> __device__ __forceinline__ double op_extreme_f64_bits(unsigned long long a, unsigned long long b)
{
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    return MAX ? (y > x ? y : x) : (y < x ? y : x);
}
template <bool MAX> __device__ __forceinline__ double wave_extreme_f64(double x)
{
    unsigned long long v = (unsigned long long)__double_as_longlong(x);
#define CAPE_F64_STEP(CTRL) v = (unsigned long long)__double_as_longlong(op_extreme_f64_bits<MAX>(v, dpp_u64<CTRL>(v)));
    CAPE_F64_STEP(kDppQuadXor1)
    CAPE_F64_STEP(kDppQuadXor2)
    CAPE_F64_STEP(kDppRowHalfMirror)
    CAPE_F64_STEP(kDppRowMirror)
#undef CAPE_F64_STEP
    const double a = op_extreme_f64_bits<MAX>(readlane_u64(v, 0), readlane_u64(v, 16)), b = op_extreme_f64_bits<MAX>(readlane_u64(v, 32), readlane_u64(v, 48));
    return MAX ? (b > a ? b : a) : (b < a ? b : a);
}

// may_be_visible by one wave, lane l on the vertices l, l + 64, ..: the same statements per vertex; a non-finite coordinate in any
// lane decides before the box is looked at, and the box of finite coordinates does not depend on the order they were met in
__device__ inline bool may_be_visible_wave(const double* Tm, const MapVisibilityParams& p, int j, int lane)
{
    const cape_map_plane& M = p.mapPlanes[j];
    const CameraFrame F = camera_frame(Tm, M);
    const cape_map_ring R = p.mapRings[M.ring_first];
    const double2* src = p.mapVertices + R.vertex_offset;
    const int n = (int)R.vertex_count;
    bool finite = true;
    double minU = __builtin_inf(), maxU = -__builtin_inf(), minV = __builtin_inf(), maxV = -__builtin_inf();
    for (int i = lane; i < n; i += 64)
    {
        const double2 s = screen_vertex(p, F, to_camera_vertex(Tm, F, src[i]));
        finite = finite && isfinite(s.x) && isfinite(s.y);
        minU = s.x < minU ? s.x : minU;
        maxU = s.x > maxU ? s.x : maxU;
        minV = s.y < minV ? s.y : minV;
        maxV = s.y > maxV ? s.y : maxV;
    }
    if (__ballot(!finite))
        return false;
    return !box_misses_screen(p, wave_extreme_f64<false>(minU), wave_extreme_f64<true>(maxU), wave_extreme_f64<false>(minV), wave_extreme_f64<true>(maxV));
}

} // namespace

__global__ __launch_bounds__(64 * kVisFrames) void cape_map_classify_kernel(MapVisibilityParams p, int nFrames)
{
    __shared__ unsigned s_count[kVisFrames];
    __shared__ unsigned long long s_base;
    __shared__ unsigned long long s_listed[kVisFrames][CAPE_MAP_MAX_PLANES / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frame = blockIdx.x * kVisFrames + wave;
    const bool live = frame < nFrames; // (idle waves of the last workgroup list nothing and store nothing)
    unsigned myCount = 0;
    if (live)
    {
        const double* T = p.poses + (size_t)frame * 16;
        uint32_t* words = p.skip + (size_t)frame * p.skipWords;
        for (int jb = 0; jb < p.nMap; jb += 64)
        {
            const int j = jb + lane;
            const bool has = j < p.nMap;
            const bool moving = has && p.moving && ((p.moving[j >> 5] >> (j & 31)) & 1u);
            const bool listed = has && !moving && may_be_visible(T, p, j);
            // bit j = moving, or not visible: every listed plane starts as not visible, and only a listed plane can turn out
            // visible -- so every bit below n_map starts set, and the bits beyond it in the last word are 0
            const unsigned long long set = __ballot(has), l = __ballot(listed);
            if (lane == 0)
            {
                words[jb >> 5] = (uint32_t)set;
                if ((jb >> 5) + 1 < p.skipWords)
                    words[(jb >> 5) + 1] = (uint32_t)(set >> 32);
                s_listed[wave][jb >> 6] = l;
            }
            myCount += (unsigned)__popcll(l);
        }
    }
    // (the list holds frames x n_map entries: every pair fits)
    unsigned long long at = reserve_pairs<kVisFrames>(p.list, s_count, s_base, myCount);
    if (!live)
        return;
    for (int jb = 0; jb < p.nMap; jb += 64)
    {
        const unsigned long long l = s_listed[wave][jb >> 6];
        if ((l >> lane) & 1ull)
            p.list.work[at + (unsigned)__popcll(l & ((1ull << lane) - 1ull))] = ((unsigned long long)(unsigned)frame << 32) | (unsigned)(jb + lane);
        at += (unsigned)__popcll(l);
    }
}

// cape_map_step_visible: frame 0 of p (one pose, one row of words) against the map whose tracks are `tracks`.  Group, wave and round of
// a plane and the words of a group: cape_map_step_visible.h.  The words and the content of the work list are the batch kernel's for
// n_frames = 1 with the tracks' moving bits as its moving words; the ORDER of the list is not (groups reserve their entries as they
// finish): no result depends on it -- the visible kernels decide every entry on its own and clear its own bit.  counts[10] and
// counts[11]: the moving planes and the listed ones.
__global__ __launch_bounds__(64 * kStepVisGroupWaves) void cape_map_classify_one_kernel(MapVisibilityParams p, const MapTrackState* tracks)
{
    __shared__ unsigned long long s_listed[kStepVisGroupWaves], s_moving[kStepVisGroupWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, group = blockIdx.x;
    unsigned long long listed = 0ull, moving = 0ull; // (uniform in the wave)
    for (int r = 0; r < kStepVisRounds; ++r)
    {
        const int j = step_vis_plane(group, wave, r);
        if (j >= p.nMap)
            break;
        const unsigned long long bit = 1ull << step_vis_slot(wave, r);
        if (tracks[j].flags & CAPE_MAP_TRACK_MOVING)
            moving |= bit;
        else if (may_be_visible_wave(p.poses, p, j, lane))
            listed |= bit;
    }
    if (lane == 0)
    {
        s_listed[wave] = listed;
        s_moving[wave] = moving;
    }
    __syncthreads();
    if (wave != 0)
        return;
    listed = moving = 0ull;
    for (int w = 0; w < kStepVisGroupWaves; ++w)
    {
        listed |= s_listed[w];
        moving |= s_moving[w];
    }
    unsigned long long base = 0ull;
    if (lane == 0)
    {
        // every bit of a plane starts set (moving, or not visible until a visible kernel says otherwise), the bits beyond n_map clear
        step_vis_store_words(p.skip, p.skipWords, group, step_vis_present(group, p.nMap));
        if (listed)
        {
            base = atomicAdd(reinterpret_cast<unsigned long long*>(p.list.counts), (unsigned long long)__popcll(listed));
            atomicAdd(&p.list.counts[11], (unsigned)__popcll(listed));
        }
        if (moving)
            atomicAdd(&p.list.counts[10], (unsigned)__popcll(moving));
    }
    base = readlane_u64(base, 0);
    // (the list holds n_map entries: every plane fits)
    if ((listed >> lane) & 1ull)
        p.list.work[base + (unsigned)__popcll(listed & ((1ull << lane) - 1ull))] = (unsigned long long)(unsigned)(group * kStepVisGroupPlanes + lane);
}

// One tier of the list's walk (walk_tier, cape_pair_list.h; p.lastTier: the largest tier that runs on this device).  A pair beyond
// the capacities of every tier that runs is undecided.
template <int TIER> __global__ __launch_bounds__(64 * Tier<TIER>::kWavesPerGroup) void cape_map_visible_kernel(MapVisibilityParams p, int ldsPerWave)
{
    using T = Tier<TIER>;
    walk_tier<TIER>(
        p.list, ldsPerWave, p.lastTier,
        [&](const TierCtx<TIER>& ctx, unsigned long long e) -> double {
            const MpLds& L = ctx.L;
            const int frame = (int)(e >> 32), j = (int)(e & 0xFFFFFFFFu);
            const cape_map_plane& M = p.mapPlanes[j];
            const cape_map_ring R = p.mapRings[M.ring_first];
            const int na = (int)R.vertex_count;
            if (na > T::kRing)
                return nan_code(kNanRing);
            const double* Tm = p.poses + (size_t)frame * 16;
            const CameraFrame F = camera_frame(Tm, M);
            // the outer ring seen from the camera (transform_boundary, polygon.cpp:430-451), oriented as the CameraPolygon holds it ...
            const double2* src = p.mapVertices + R.vertex_offset;
            for (int v = ctx.tid; v < na; v += ctx.kStride)
                L.ringA[v] = to_camera_vertex(Tm, F, src[v]);
            ctx.sync();
            orient_ring(L.ringA, na, false, ctx);
            // ... on the screen, oriented again (boost::geometry::correct in to_screen_space)
            for (int v = ctx.tid; v < na; v += ctx.kStride)
                L.ringA[v] = screen_vertex(p, F, L.ringA[v]);
            // the screen rectangle (utils/polygon.cpp:27-37)
            if (ctx.tid < 4)
                L.ringB[ctx.tid] = make_double2((ctx.tid == 1 || ctx.tid == 2) ? p.width - 1.0 : 1.0, ctx.tid >= 2 ? p.height - 1.0 : 1.0);
            ctx.sync();
            orient_ring(L.ringA, na, false, ctx);
            orient_ring(L.ringB, 4, false, ctx);
            return ctx.inter_area(na, 4);
        },
        [&](size_t, unsigned long long e, double result) {
            const int frame = (int)(e >> 32), j = (int)(e & 0xFFFFFFFFu);
            const bool undecided = is_nan_code(result, kNanStack) || is_nan_code(result, kNanSlabs) || is_nan_code(result, kNanRing);
            if (result > 0 || undecided)
                atomicAnd(&p.skip[(size_t)frame * p.skipWords + (j >> 5)], ~(1u << (j & 31)));
            if (undecided)
                atomicAdd(reinterpret_cast<unsigned long long*>(p.list.counts + 8), 1ull);
        });
}

namespace {

// the visible kernels behind either classify kernel
hipError_t launch_visible_tiers(const MapVisibilityParams& p, hipStream_t stream)
{
    if (const hipError_t e = launch_tier<0>(cape_map_visible_kernel<0>, p, stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<1>(cape_map_visible_kernel<1>, p, stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<2>(cape_map_visible_kernel<2>, p, stream); e != hipSuccess)
        return e;
    // (a device without the LDS for the largest tier: lastTier = 2, the pairs it would take are undecided)
    if (p.lastTier >= 3)
        return launch_tier<3>(cape_map_visible_kernel<3>, p, stream);
    return hipSuccess;
}

} // namespace

hipError_t launch_map_visibility(const MapVisibilityParams& params, int nFrames, hipStream_t stream)
{
    MapVisibilityParams p = params;
    p.lastTier = tier_lds_bytes<3>() <= (size_t)p.ldsLimitBytes ? 3 : 2;
    if (const hipError_t e = hipMemsetAsync(p.list.counts, 0, 16 * sizeof(unsigned), stream); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_map_classify_kernel, dim3((nFrames + kVisFrames - 1) / kVisFrames), dim3(64 * kVisFrames), 0, stream, p, nFrames);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    return launch_visible_tiers(p, stream);
}

// one frame (p.poses: its pose; p.skip: its words; p.moving is not read) of a map of p.nMap >= 1 planes with the tracks `tracks`
hipError_t launch_map_step_visibility(const MapVisibilityParams& params, const MapTrackState* tracks, hipStream_t stream)
{
    MapVisibilityParams p = params;
    p.lastTier = tier_lds_bytes<3>() <= (size_t)p.ldsLimitBytes ? 3 : 2;
    if (const hipError_t e = hipMemsetAsync(p.list.counts, 0, 16 * sizeof(unsigned), stream); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_map_classify_one_kernel, dim3(step_vis_groups(p.nMap)), dim3(64 * kStepVisGroupWaves), 0, stream, p, tracks);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    return launch_visible_tiers(p, stream);
}

} // namespace cape
