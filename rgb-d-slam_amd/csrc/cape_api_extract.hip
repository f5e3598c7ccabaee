// C ABI, host side: the extraction entry points, the kernel chain and its schedule, the sub-batch pipeline, the wait for a
// chain's results and the readers of those results (see cape_api.hip for the map of the API files).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>

#include "cape_handle.h"

using namespace cape::abi;

namespace {

// completion signal of a chain whose results live in pinned host memory (see wait_results)
__global__ void cape_signal_kernel(uint32_t* flag, uint32_t seq)
{
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// parameter blocks of a sub-batch that starts at frame f0
void offset_params(const cape_handle_s* h, int f0, cape::StageAParams& a, cape::StageBParams& b)
{
    a = h->pa;
    b = h->pb;
    const size_t C = (size_t)h->cells, F = (size_t)f0;
    const size_t px = F * (size_t)h->cfg.width * h->cfg.height;
    if (a.depth)
        a.depth += px;
    if (a.depth_u16)
        a.depth_u16 += px;
    a.cell_sums += F * C * cape::kSumStride;
    a.cell_plane += F * C * cape::kPlaneStride;
    a.cell_score += F * C;
    a.cell_tol += F * C;
    a.cell_flags += F * C;
    a.cell_bins += F * C;
    a.cell_aux += F * C;
    a.cell_mse += F * C;
    b.cell_aux = a.cell_aux;
    b.cell_mse = a.cell_mse;
    b.cell_sums = a.cell_sums;
    b.cell_plane = a.cell_plane;
    b.cell_score = a.cell_score;
    b.cell_tol = a.cell_tol;
    b.cell_flags = a.cell_flags;
    b.cell_bins = a.cell_bins;
    b.records += F;
    b.plane_labels += F * C;
    b.cyl_labels += F * C;
    b.boundary += F * (size_t)h->boundaryCap * 3;
    if (b.cylScratch)
        b.cylScratch += F * C * cape::kCylStride;
    if (b.needCylinder)
        b.needCylinder += 2 * F; // a sub-batch of n frames uses 1 + n entries of its own
    if (b.resumeList)
    {
        b.resumeList += 2 * F;
        b.growState += F * (size_t)b.growStateStride;
    }
    b.redoList += 2 * F;
    b.spillList += 2 * F;
    b.seed_sequence += F * C;
    b.debugCycles += F * cape::kProfileSlots;
}

// the per-launch fields of one chain of `frames` frames: the kernel that ends stage A (A2, the fused A1 or the strip kernel) clears the chain's lists (and the spill pool's counters,
// `clear4`, unless they are shared with other sub-batches), stage B learns A2's tiling and whether this chain is timed
void prepare_launch(const cape_handle_s* h, cape::StageAParams& a2, cape::StageBParams& b, uint32_t* clear4, bool strips, int frames,
                    bool timed)
{
    a2.clear0 = b.redoList;
    a2.clear1 = b.needCylinder;
    a2.clear2 = b.resumeList;
    a2.clear2Buckets = b.resumeList ? b.resumeBucketStride : 0u;
    a2.clear3 = b.spillList;
    a2.clear4 = clear4;
    b.phaseTicks = timed ? h->timing.phaseTicks.get() : nullptr; // the reference's grow / merge / refine buckets, only while timing is on
    b.a2RowsPerTile = strips ? a2.vCells : cape::cell_plane_rows_per_tile(a2, frames);
    b.countersCleared = 1;
}

// next free event set for one timed kernel chain (creates / recycles on demand)
int acquire_events(cape_handle_s* h, int frames, cape_handle_s::Timing::Events** out)
{
    auto& T = h->timing;
    *out = nullptr;
    if (!T.enabled)
        return CAPE_OK;
    if (T.pending == T.pool.size())
    {
        if (T.pool.size() >= 4096)
        {
            const int rc = fold_timings(h); // synchronises; keeps the pool bounded
            if (rc != CAPE_OK)
                return rc;
        }
        else
        {
            cape_handle_s::Timing::Events nt;
            for (auto& e : nt.e)
                CAPE_HIP_TRY(e.ensure(hipEventDefault));
            CAPE_HIP_TRY(nt.e2b.ensure(hipEventDefault));
            T.pool.push_back(std::move(nt));
        }
    }
    *out = &T.pool[T.pending];
    (*out)->frames = frames;
    (*out)->split = h->cfg.sub_batches > 1;
    T.pending += 1;
    return CAPE_OK;
}

// one kernel chain (A1 -> A2 -> B) on `st`, optionally bracketed by timing events
int launch_chain(cape_handle_s* h, const cape::StageAParams& a, const cape::StageBParams& b, int frames, hipStream_t st)
{
    auto& c = h->chain;
    auto& r = h->res;
    cape_handle_s::Timing::Events* t = nullptr;
    const int rc = acquire_events(h, frames, &t);
    if (rc != CAPE_OK)
        return rc;
    if (t)
        CAPE_HIP_TRY(hipEventRecord(t->e[0], st));
    // A frame read straight from pinned host memory arrives at the link's pace (~34 us for 1.2 MB): the band kernel streams it in
    // and the plane kernel's 17 us follow; a strip's tail behind its last pixel is as long, so nothing is gained there (measured,
    // profiles/r04_single_frame_latency.txt).  With the frame in HBM the one-launch form is 5-10 us faster.
    const bool strips = c.stripCounters && frames <= kHostResultFrames && (!c.inputOverLink || c.stripsAlways);
    cape::StageAParams a2 = a;
    cape::StageBParams bb = b;
    prepare_launch(h, a2, bb, c.spillCounters, strips, frames, t != nullptr);
    if (strips)
    {
        // the latency instance: all of stage A in one launch (timing: booked as the moments kernel, the plane kernel reads 0)
        CAPE_HIP_TRY(cape::launch_cell_strips(a2, frames, c.stripCounters, st));
        if (t)
        {
            CAPE_HIP_TRY(hipEventRecord(t->e[1], st));
            CAPE_HIP_TRY(hipEventRecord(t->e[2], st));
        }
    }
    else if (a.a2Fused && cape::cell_plane_threads(a2, frames) == 256)
    {
        // the lanes of A1 fit their cells: one launch, whose tiles are those of the 256-thread A2 that the split path would run for
        // this call -- so a2RowsPerTile is what stage B was told anyway (timing: booked as the moments kernel, the plane kernel reads 0)
        CAPE_HIP_TRY(cape::launch_cell_fused(a2, frames, st));
        if (t)
        {
            CAPE_HIP_TRY(hipEventRecord(t->e[1], st));
            CAPE_HIP_TRY(hipEventRecord(t->e[2], st));
        }
    }
    else
    {
        CAPE_HIP_TRY(cape::launch_cell_moments(a, frames, st));
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e[1], st));
        CAPE_HIP_TRY(cape::launch_cell_plane(a2, frames, st));
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e[2], st));
    }
    // The one-frame chain: stage A, then ONE grow kernel -- the 64-segment instance on every frame of the call, no
    // 32-segment pass in front, no redo pass and no one-thread signal kernel behind: its last wave stores the sequence number the
    // host spins on.  Two launches instead of four or five on the path the reference calls (CAPE_STAGE_A=bands: the classic chain).
    const bool oneFrameChain = h->resultsOnHost && r.doneFlag && r.doneCounter && frames <= kHostResultFrames;
    if (oneFrameChain)
    {
        bb.allFrames = c.generalAll ? 0 : 1;
        bb.doneFlag = r.doneFlag;
        bb.doneCounter = r.doneCounter;
        bb.doneSeq = ++r.doneSeq;
        bb.spillHost = c.generalAll ? nullptr : r.doneFlag + 1;
    }
    if (bb.needCylinder)
    {
        // Cost model, in rounds of the cylinder kernel (one round = cylSlots resident frames, ~0.25 ms at 640x480):
        //   cylinder kernel alone      ceil(frames / slots)
        //   plane-only pass first      kPlanePassPerRound * frames / slots  +  ceil(handed_over / slots)
        // kPlanePassPerRound = 0.29 is the measured cost of growing one round's worth of frames with the plane-only
        // kernel (profiles/schedule_crossover.py).  A single handed-over frame is cheaper alone; a batch that hands
        // over half of its frames usually saves a round.
        constexpr double kPlanePassPerRound = 0.29;
        constexpr int kProbeEvery = 32; // a single-pass handle re-measures with a two-pass call now and then
        if (c.handedOverFrames > 0 && hipEventQuery(c.handedOverReady) == hipSuccess)
        {
            c.handedOverFraction = (double)(c.handedOverHost[0] + c.handedOverHost[1]) / (double)c.handedOverFrames; // redone + parked
            c.handedOverFrames = 0;
        }
        {
            const double slots = (double)(c.cylSlots > 0 ? c.cylSlots : 1024);
            const double alone = std::ceil((double)frames / slots);
            // a parked frame is finished, not grown again: its round of the second pass is shorter (measured, 640x480: 0.12 ms
            // per 1 024 tunnel frames by the lone-wave RESUME instance against 0.15 ms for the full kernel; the workgroup
            // kernel of the wide grids: 0.5 ms against 0.97 ms per 1 024 frames of 1280x960)
            const double secondPassPerRound = !bb.resumeList ? 1.0 : (bb.resumeMode == 2 ? 0.5 : 0.8);
            const double twoPass = kPlanePassPerRound * (double)frames / slots +
                                   secondPassPerRound * std::ceil(c.handedOverFraction * (double)frames / slots);
            c.singlePass = twoPass >= alone;
            // a handful of frames (the reference's one-frame call pattern): what counts is the number of launches on the
            // latency path, and the cylinder kernel alone is one launch instead of four
            if (frames <= kHostResultFrames)
                c.singlePass = true;
        }
        const bool probe = c.singlePass && frames > kHostResultFrames && ++c.callsSinceProbe >= kProbeEvery;
        bb.twoPass = (!c.singlePass || probe) ? 1 : 0;
        if (c.forcedSchedule)
            bb.twoPass = c.forcedSchedule == 1 ? 1 : 0;
        if (probe)
            c.callsSinceProbe = 0;
    }
    CAPE_HIP_TRY(cape::launch_grow(bb, frames, st, c.generalAll ? nullptr : h->sideStream, h->sideFork, h->sideDone, &h->gen));
    if (h->sideStream && bb.needCylinder && !c.generalAll)
        h->sidePending = true;
    if (bb.needCylinder && bb.twoPass && c.handedOverFrames == 0 && !c.generalAll)
    {
        CAPE_HIP_TRY(hipMemcpyAsync(c.handedOverHost, bb.needCylinder, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (bb.resumeList)
            CAPE_HIP_TRY(hipMemcpyAsync(c.handedOverHost + 1, bb.resumeList, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CAPE_HIP_TRY(hipEventRecord(c.handedOverReady, st));
        c.handedOverFrames = frames;
    }
    if (t)
        CAPE_HIP_TRY(hipEventRecord(t->e[3], h->sidePending ? (hipStream_t)h->sideStream : st));
    if (h->resultsOnHost && r.doneFlag)
    {
        if (!oneFrameChain)
        {
            hipLaunchKernelGGL(cape_signal_kernel, dim3(1), dim3(1), 0, st, r.doneFlag.get(), ++r.doneSeq);
            CAPE_HIP_TRY(hipGetLastError());
        }
        r.doneArmed = true;
    }
    r.lazySpillArmed = bb.spillHost != nullptr;
    if (r.lazySpillArmed)
    {
        r.lazySpillParams = bb;
        r.lazySpillFrames = frames;
    }
    return CAPE_OK;
}

// sub-batch pipelining: stream 0 runs the streaming kernel of every sub-batch back to back; stream 1 runs the per-cell fit and
// the grow kernel of sub-batch i as soon as its moments are done, i.e. underneath the moments of sub-batch i+1
int launch_pipelined(cape_handle_s* h, int n_frames, hipStream_t stream)
{
    auto& c = h->chain;
    // fork: both internal streams wait for everything already enqueued on the caller's stream
    CAPE_HIP_TRY(hipMemsetAsync(c.spillCounters, 0, 2 * sizeof(uint32_t), stream));
    CAPE_HIP_TRY(hipEventRecord(c.pipeFork, stream));
    for (auto& st : c.pipeStream)
        CAPE_HIP_TRY(hipStreamWaitEvent(st, c.pipeFork, 0));
    const int k = h->cfg.sub_batches;
    for (int i = 0; i < k; ++i)
    {
        const int f0 = (int)((long long)n_frames * i / k), f1 = (int)((long long)n_frames * (i + 1) / k);
        cape::StageAParams a;
        cape::StageBParams b;
        offset_params(h, f0, a, b);
        cape_handle_s::Timing::Events* t = nullptr;
        const int rc = acquire_events(h, f1 - f0, &t);
        if (rc != CAPE_OK)
            return rc;
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e[0], c.pipeStream[0]));
        CAPE_HIP_TRY(cape::launch_cell_moments(a, f1 - f0, c.pipeStream[0]));
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e[1], c.pipeStream[0]));
        CAPE_HIP_TRY(hipEventRecord(c.pipeStage[i], c.pipeStream[0]));
        CAPE_HIP_TRY(hipStreamWaitEvent(c.pipeStream[1], c.pipeStage[i], 0));
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e2b, c.pipeStream[1]));
        // (the pool's counters are shared by the sub-batches: cleared once, in front of the fork)
        prepare_launch(h, a, b, nullptr, false, f1 - f0, t != nullptr);
        CAPE_HIP_TRY(cape::launch_cell_plane(a, f1 - f0, c.pipeStream[1]));
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e[2], c.pipeStream[1]));
        CAPE_HIP_TRY(cape::launch_grow(b, f1 - f0, c.pipeStream[1], nullptr, nullptr, nullptr, &h->gen));
        if (t)
            CAPE_HIP_TRY(hipEventRecord(t->e[3], c.pipeStream[1]));
    }
    // join
    for (int i = 0; i < 2; ++i)
    {
        CAPE_HIP_TRY(hipEventRecord(c.pipeJoin[i], c.pipeStream[i]));
        CAPE_HIP_TRY(hipStreamWaitEvent(stream, c.pipeJoin[i], 0));
    }
    return CAPE_OK;
}

int extract_impl(cape_handle h, const float* depth_dev, const uint16_t* depth_u16, float scale, int32_t n_frames, void* stream_)
{
    if (!h || (!depth_dev && !depth_u16) || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle/depth or negative frame count");
    if (n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds max_batch");
    // the streaming kernel reads four pixels per lane with one vector load
    if ((depth_dev && reinterpret_cast<uintptr_t>(depth_dev) % 16 != 0) || (depth_u16 && reinterpret_cast<uintptr_t>(depth_u16) % 8 != 0))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "depth must be aligned to four pixels (16 bytes of float32, 8 bytes of uint16)");
    auto& r = h->res;
    r.lastFrames = n_frames;
    r.logPending = n_frames > 0; // cape_set_log_callback: this batch's records have not reached the host yet
    r.logDone = 0;
    h->poly.frames = 0;      // the polygons on the device belong to the previous batch
    h->poly.matchFrames = 0; // and so do the polygon matches
    h->map.matchFrames = 0;  // and the map matches
    h->wide.matchFrames = 0; // and the wide polygon matches
    h->mapWide.matchFrames = 0; // and the wide map matches
    h->measure.frames = 0;      // and the measurements of its kept planes
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h); // the handle's device, whatever the calling thread had current
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    h->pa.depth = depth_dev;
    h->pa.depth_u16 = depth_u16;
    h->pa.u16_scale = scale;
    r.doneArmed = false;      // only launch_chain puts a signal behind the work; every other path drains the stream
    r.lazySpillArmed = false; // (a one-frame chain nobody read: its results are about to be overwritten)
    if (h->cfg.sub_batches > 1 && n_frames >= 2 * h->cfg.sub_batches)
        return launch_pipelined(h, n_frames, stream);
    return launch_chain(h, h->pa, h->pb, n_frames, stream);
}

int extract_device(cape_handle h, const float* depth, float, int32_t n_frames, void* stream)
{
    return cape_extract(h, depth, n_frames, stream);
}
int extract_device(cape_handle h, const uint16_t* depth, float scale, int32_t n_frames, void* stream)
{
    return cape_extract_u16(h, depth, scale, n_frames, stream);
}

// cape_extract_host / cape_extract_u16_host.  Pinned input (cape_host_alloc / cape_host_register, or any hipHostMalloc'ed /
// registered buffer): a few frames are read by the streaming kernel straight from host memory -- the image is read exactly once,
// so the PCIe transfer IS the kernel's input stream and no staging copy precedes it; larger batches take one DMA from the pinned
// pages.  Pageable input goes through the runtime's staged copy.
template <typename Pixel> int extract_host(cape_handle h, const Pixel* depth_host, float scale, int32_t n_frames, void* stream_)
{
    constexpr size_t kAlign = 4 * sizeof(Pixel); // four pixels per lane (extract_impl)
    if (!h || !depth_host || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle/depth or negative frame count");
    if (n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds max_batch");
    CAPE_ON_DEVICE(h);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    auto& c = h->chain;
    const size_t framePixels = (size_t)h->cfg.width * h->cfg.height;
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, depth_host) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer;
    if (!pinned)
        (void)hipGetLastError(); // an unregistered pointer is not an error here
    if (pinned && !c.pinnedByDma && n_frames <= kHostResultFrames && reinterpret_cast<uintptr_t>(attr.devicePointer) % kAlign == 0)
    {
        c.inputOverLink = true;
        const int rc = extract_device(h, static_cast<const Pixel*>(attr.devicePointer), scale, n_frames, stream_);
        c.inputOverLink = false;
        return rc;
    }
    CAPE_HIP_TRY(c.depthStage.ensure((size_t)h->cfg.max_batch * framePixels)); // (float32 frames: the uint16 path shares it)
    CAPE_HIP_TRY(hipMemcpyAsync(c.depthStage, depth_host, (size_t)n_frames * framePixels * sizeof(Pixel), hipMemcpyHostToDevice, stream));
    return extract_device(h, reinterpret_cast<const Pixel*>(c.depthStage.get()), scale, n_frames, stream_);
}

// Results in pinned host memory: wait for the signal word of the last chain.  The runtime's hipStreamSynchronize costs
// ~10 us of wake-up on top of the kernels when the whole call is ~130 us; a spin on a pinned word costs a PCIe write.
// If the word does not arrive in time (a faulted kernel, a descheduled process) the stream synchronisation takes over
// and reports whatever went wrong.
int wait_results_once(cape_handle_s* h)
{
    auto& r = h->res;
    if (r.doneArmed && r.doneFlag)
    {
        volatile const uint32_t* flag = r.doneFlag;
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0;; ++spin)
        {
            if (*flag == r.doneSeq)
            {
                std::atomic_thread_fence(std::memory_order_acquire); // the results are read after the word
                return CAPE_OK;
            }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#elif defined(__aarch64__)
            __asm__ __volatile__("yield");
#endif
            if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5))
                break;
        }
    }
    if (h->workRecorded)
        CAPE_HIP_TRY(hipEventSynchronize(h->workDone));
    else
        CAPE_HIP_TRY(hipDeviceSynchronize());
    return CAPE_OK;
}

} // namespace

namespace cape::abi {

// one stream in flight per handle (see cape_handle_s::lastStream): a call on another stream is ordered behind the
// handle's previous work on the device, through the handle's own event
int enter_stream(cape_handle_s* h, hipStream_t st)
{
    const bool other = h->hasLastStream && h->lastStream != st;
    h->lastStream = st;
    h->hasLastStream = true;
    if (other && h->workRecorded)
        CAPE_HIP_TRY(hipStreamWaitEvent(st, h->workDone, 0));
    if (h->sidePending)
    {
        // the previous call's second pass is still on the handle's side stream: this call (and the caller's stream from here
        // on) is ordered behind it
        CAPE_HIP_TRY(hipStreamWaitEvent(st, h->sideDone, 0));
        h->sidePending = false;
    }
    return CAPE_OK;
}

hipError_t drain_handle(cape_handle_s* h)
{
    if (h->sidePending)
    {
        if (const hipError_t e = hipEventSynchronize(h->sideDone); e != hipSuccess)
            return e;
        h->sidePending = false;
    }
    if (h->workRecorded)
        return hipEventSynchronize(h->workDone);
    return hipSuccess;
}

// behind THIS handle's work only (its event, its side stream): several handles driven from several host threads -- the overlay's
// shards -- must not wait for each other's kernels here (through round 5 this was a hipDeviceSynchronize)
hipError_t sync_handle(cape_handle_s* h)
{
    return (h->workRecorded || h->sidePending) ? drain_handle(h) : hipDeviceSynchronize();
}

int wait_results(cape_handle_s* h)
{
    auto& r = h->res;
    if (const int rc = wait_results_once(h); rc != CAPE_OK)
        return rc;
    if (r.lazySpillArmed)
    {
        // the one-frame chain left the general grow instance to us: a frame of more than 64 plane segments / cylinder labels is on
        // the spill list (the word next to the completion word says how many) -- enqueue that kernel now and wait for its signal
        r.lazySpillArmed = false;
        if (r.doneFlag && r.doneFlag[1] != 0u)
        {
            cape::StageBParams p = r.lazySpillParams;
            p.spillHost = nullptr;
            p.allFrames = 0;
            p.doneSeq = ++r.doneSeq;
            CAPE_HIP_TRY(cape::launch_grow_general(p, h->gen, r.lazySpillFrames, h->lastStream));
            if (h->workDone && hipEventRecord(h->workDone, h->lastStream) == hipSuccess)
                h->workRecorded = true;
            r.doneArmed = true;
            return wait_results_once(h);
        }
    }
    return CAPE_OK;
}

int settle_results(cape_handle_s* h)
{
    if (h->resultsOnHost)
        return wait_results(h); // the kernels wrote into pinned host memory: once the signal word has arrived the data is there
    CAPE_HIP_TRY(sync_handle(h));
    return CAPE_OK;
}

} // namespace cape::abi

extern "C" {

int cape_extract(cape_handle h, const float* depth_dev, int32_t n_frames, void* stream_)
{
    return extract_impl(h, depth_dev, nullptr, 0.0f, n_frames, stream_);
}

int cape_extract_u16(cape_handle h, const uint16_t* depth_dev, float scale, int32_t n_frames, void* stream_)
{
    if (!(scale > 0.0f))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "scale must be positive");
    return extract_impl(h, nullptr, depth_dev, scale, n_frames, stream_);
}

int cape_extract_host(cape_handle h, const float* depth_host, int32_t n_frames, void* stream_)
{
    return extract_host(h, depth_host, 0.0f, n_frames, stream_);
}

int cape_extract_u16_host(cape_handle h, const uint16_t* depth_host, float scale, int32_t n_frames, void* stream_)
{
    return extract_host(h, depth_host, scale, n_frames, stream_);
}

int cape_device_results(cape_handle h, void** records, int32_t** plane_labels, int32_t** cyl_labels, double** boundary)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (records)
        *records = h->res.records;
    if (plane_labels)
        *plane_labels = h->res.planeLabels;
    if (cyl_labels)
        *cyl_labels = h->res.cylLabels;
    if (boundary)
        *boundary = h->res.boundary;
    return CAPE_OK;
}

int cape_sync_results(cape_handle h, void* stream_)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    CAPE_ON_DEVICE(h);
    StreamScope streamScope(h, static_cast<hipStream_t>(stream_)); // enter_stream does the waiting
    return streamScope.rc();
}

int cape_copy_results(cape_handle h, int32_t n_frames, cape_frame_record* records, int32_t* plane_labels,
                      int32_t* cyl_labels, double* boundary)
{
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    CAPE_ON_DEVICE(h);
    if (const int rc = settle_results(h); rc != CAPE_OK)
        return rc;
    const auto& r = h->res;
    const size_t n = (size_t)n_frames, C = (size_t)h->cells;
    CAPE_HIP_TRY(copy_out(records, r.records, 0, n));
    log_batch(h, records, n_frames);
    CAPE_HIP_TRY(copy_out(plane_labels, r.planeLabels, 0, n * C));
    CAPE_HIP_TRY(copy_out(cyl_labels, r.cylLabels, 0, n * C));
    CAPE_HIP_TRY(copy_out(boundary, r.boundary, 0, n * (size_t)h->boundaryCap * 3));
    return CAPE_OK;
}

int cape_host_results(cape_handle h, const cape_frame_record** records, const int32_t** plane_labels, const int32_t** cyl_labels,
                      const double** boundary)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->resultsOnHost)
        return fail(CAPE_ERR_UNSUPPORTED, "results live in device memory for this handle (max_batch > 8): use cape_copy_results");
    CAPE_ON_DEVICE(h);
    if (const int rc = wait_results(h); rc != CAPE_OK)
        return rc;
    const auto& r = h->res;
    log_batch(h, r.records, r.lastFrames);
    if (records)
        *records = r.records;
    if (plane_labels)
        *plane_labels = r.planeLabels;
    if (cyl_labels)
        *cyl_labels = r.cylLabels;
    if (boundary)
        *boundary = r.boundary;
    return CAPE_OK;
}

int cape_spill_info(cape_handle h, int32_t* used, int32_t* capacity, int32_t* frames)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    CAPE_ON_DEVICE(h);
    uint32_t c[2] = {0u, 0u};
    if (h->res.lastFrames > 0)
    {
        if (const int rc = settle_results(h); rc != CAPE_OK)
            return rc;
        CAPE_HIP_TRY(hipMemcpy(c, h->chain.spillCounters, sizeof(c), hipMemcpyDeviceToHost));
    }
    if (used)
        *used = (int32_t)std::min<uint32_t>(c[0], (uint32_t)h->chain.spillRecords);
    if (capacity)
        *capacity = h->chain.spillRecords;
    if (frames)
        *frames = (int32_t)c[1];
    return CAPE_OK;
}

int cape_copy_spill(cape_handle h, int32_t first, int32_t count, cape_frame_record* records, double* boundary)
{
    if (!h || first < 0 || count < 0 || first > h->chain.spillRecords || count > h->chain.spillRecords - first)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / spill record range");
    CAPE_ON_DEVICE(h);
    if (const int rc = settle_results(h); rc != CAPE_OK)
        return rc;
    const size_t at = (size_t)h->cfg.max_batch + (size_t)first, n = (size_t)count, cap = (size_t)h->boundaryCap;
    CAPE_HIP_TRY(copy_out(records, h->res.records, at, n));
    CAPE_HIP_TRY(copy_out(boundary, h->res.boundary, at * cap * 3, n * cap * 3));
    return CAPE_OK;
}

} // extern "C"
