"""cape_map_maintain against the route it replaces -- cape_map_download + cape_host_map_maintain + cape_map_upload +
cape_map_upload_tracks -- and what it adds to a tracking loop's frame, on the eight room frames of tests/test_gpu_map_kalman.py (room
stream, seed 11, frames 20, 25, .. 55; the map: the stageable planes of the first frame with several planes; and that map filled up to
896 planes with copies of its planes a little off, as profiles/map_commit_rate.py makes it).

1. The call.  Per repetition the map and tracks are uploaded again -- every seventh plane a staged one due for promotion, every seventh
   a staged one due to be dropped, every seventh a local one that is lost (in the 2-plane map: one promoted, one lost) -- and the
   retired log is cleared, untimed; then
     the call:       a host clock around cape_map_maintain, which returns after its own stream synchronise, and device events around
                     the same call (the two kernels and the header's copy);
     the host route: a host clock around Extractor.download_map, the C call cape_host_map_maintain (output arrays allocated
                     beforehand) and Extractor.upload_map + Extractor.upload_tracks of its result, which are synchronous.
   The two routes alternate repetition by repetition in one run; the figures are medians with their ranges.
2. The loop.  For f = 0 .. 7 on the same batch: cape_match_map_wide, cape_map_kalman, cape_map_union_cut, cape_map_commit(f,
   ADD_STAGED) -- and, every other repetition, cape_map_maintain behind it; a host clock around the eight frames, divided by eight.  The
   difference of the two periods is what the second header round trip costs a frame (the maintained map is also a little smaller, so
   the other calls of the frame see a different map; the maintain calls' own times inside the loop are given beside it).

    python profiles/map_maintain_rate.py [--reps 30] [--out profiles/map_maintain_rate.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def spread(ms):
    return f"median {statistics.median(ms) * 1e3:8.1f} us (min {min(ms) * 1e3:8.1f}, max {max(ms) * 1e3:8.1f} over {len(ms)} repetitions)"


def due_tracks(ca, tracks):
    """every seventh plane promoted, dropped and lost in turn; the 2-plane map: one promoted, one lost"""
    t = tracks.copy()
    t["successive_matched"], t["failed_tracking"] = 0, 0
    for j in range(len(t)):
        kind = j % 7 if len(t) > 2 else (0, 5)[j]
        if kind == 0:
            t[j]["flags"], t[j]["successive_matched"] = ca.MAP_TRACK_STAGED, 4
        elif kind == 3:
            t[j]["flags"], t[j]["failed_tracking"] = ca.MAP_TRACK_STAGED, 2
        elif kind == 5:
            t[j]["flags"], t[j]["failed_tracking"] = 0, 10
    return t


def host_route(ca, ex, n_planes, n_rings, n_vertices):
    """download + cape_host_map_maintain + upload, the output arrays allocated beforehand: returns run() -> the twin's result"""
    L = ca._host_library()
    out = dict(planes=np.zeros(max(n_planes, 1), ca.MAP_PLANE_DTYPE), rings=np.zeros(max(n_rings, 1), ca.MAP_RING_DTYPE),
               vertices=np.zeros((max(n_vertices, 1), 2)), tracks=np.zeros(max(n_planes, 1), ca.MAP_TRACK_DTYPE))
    log = {k: a.copy() for k, a in out.items()}
    result = np.zeros(1, ca.MAP_MAINTAIN_RESULT_DTYPE)

    def run():
        arrays, tracks = ex.download_map()
        _, src_view = ca._map_arrays(arrays, tracks)
        caps = dict(planes_capacity=len(out["planes"]), rings_capacity=len(out["rings"]), vertices_capacity=len(out["vertices"]))
        v, lv = ca._view(ca.cape_host_map, out, **caps), ca._view(ca.cape_host_map, log, **caps)
        rc = L.cape_host_map_maintain(C.byref(src_view), C.byref(v), C.byref(lv), result.ctypes.data)
        if rc != 0 or result[0]["flags"] != ca.MAINTAIN_DONE:
            raise ca.CapeError(f"cape_host_map_maintain failed ({rc}, flags {int(result[0]['flags']):#x})")
        ex.upload_map((out["planes"][:v.n_planes], out["rings"][:v.n_rings], out["vertices"][:v.n_vertices]))
        ex.upload_tracks(out["tracks"][:v.n_planes])
        return result[0]

    return run


def the_call(ca, ex, st, torch, arrays, tracks, reps, lines):
    due = due_tracks(ca, tracks)
    P, R, V = arrays
    run_host = host_route(ca, ex, len(P), len(R), len(V))

    def prepare():
        ex.upload_map(arrays)
        ex.upload_tracks(due)
        ex.clear_retired()
        torch.cuda.synchronize()

    call_ms, span_ms, host_ms, result = [], [], [], None
    for rep in range(reps + 3):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        result = ex.map_maintain(0, st)
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        prepare()
        t2 = time.perf_counter()
        twin = run_host()
        t3 = time.perf_counter()
        assert result.tobytes() == twin.tobytes()
        if rep >= 3:
            call_ms.append((t1 - t0) * 1e3)
            span_ms.append(e0.elapsed_time(e1))
            host_ms.append((t3 - t2) * 1e3)
    lines.append(f"a map of {len(P)} planes, {len(R)} rings, {len(V)} vertices: flags {int(result['flags']):#x}, {int(result['n_promoted'])} promoted, "
                 f"{int(result['n_dropped'])} dropped, {int(result['n_lost'])} lost, {int(result['n_planes'])} planes / {int(result['n_vertices'])} vertices after; "
                 f"maintain call {spread(call_ms)}, device span {spread(span_ms)}; host route {spread(host_ms)}; ratio of the medians (host route / call) "
                 f"{statistics.median(host_ms) / statistics.median(call_ms):.1f}")


def the_loop(ca, ex, st, torch, n, arrays, tracks, W2C, reps, lines):
    periods, inside = {False: [], True: []}, []
    counts = None
    for rep in range(2 * (reps + 3)):
        with_maintain = rep % 2 == 1
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.clear_retired()
        torch.cuda.synchronize()
        next_id, mine, totals = 1000, [], np.zeros(3, int)
        t0 = time.perf_counter()
        for f in range(n):
            ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
            ex.map_kalman(n, st)
            ex.map_union_cut(n, st)
            result, next_id = ex.map_commit(f, ca.COMMIT_ADD_STAGED, next_id, st)
            if not result["flags"] & ca.COMMIT_DONE:
                raise ca.CapeError(f"frame {f} is refused ({int(result['flags']):#x})")
            if with_maintain:
                m0 = time.perf_counter()
                r = ex.map_maintain(0, st)
                mine.append((time.perf_counter() - m0) * 1e3)
                totals += [int(r["n_promoted"]), int(r["n_dropped"]), int(r["n_lost"])]
        t1 = time.perf_counter()
        if rep >= 6:
            periods[with_maintain].append((t1 - t0) * 1e3 / n)
            inside += mine
            counts = totals if with_maintain else counts
    a, b = statistics.median(periods[False]), statistics.median(periods[True])
    lines.append(f"the loop (wide match, Kalman, union_cut, commit per frame; a map of {len(arrays[0])} planes at the start, {counts[0]} promoted, "
                 f"{counts[1]} dropped, {counts[2]} lost over the eight frames): period per frame with commit alone {spread(periods[False])}; with commit + "
                 f"maintain {spread(periods[True])}; difference of the medians {(b - a) * 1e3:.1f} us; the maintain calls inside the loop {spread(inside)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd as ca
    from cape_amd import Extractor, synth, synth_gpu
    from map_commit_rate import wall_copies

    st = torch.cuda.current_stream().cuda_stream
    n, seed, start, stride = 8, 11, 20, 5
    picks = [start + stride * i for i in range(n)]
    dev = torch.cat([synth_gpu.stream("room", seed, 1, start=f, device="cuda", chunk=1) for f in picks]).contiguous()
    poses = synth_gpu._poses("room", seed, 0, start + stride * n)
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    T, W2C = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    for f in range(n):
        R, o = poses[picks[f]]
        T[f, :3, :3], T[f, :3, 3], T[f, 3, 3] = R, o, 1.0
        W2C[f, :3, :3], W2C[f, :3, 3], W2C[f, 3, 3] = R.T, -R.T @ o, 1.0
    rng = np.random.default_rng(21)
    S = np.zeros((n, 3, 3))
    for f in range(n):
        A = rng.normal(size=(3, 3))
        S[f] = A @ A.T + 3 * np.eye(3)
    ex.map_measure(n, T, S, st)
    meas = ex.map_measurements(n)
    source = next(f for f in range(n) if len(meas[f]) > 1)
    map_meas = [m for m in meas[source] if m["flags"] & ca.MEASURE_STAGEABLE]
    own = ca.pack_map([m["plane"] for m in map_meas])
    own_tracks = np.zeros(len(map_meas), ca.MAP_TRACK_DTYPE)
    for j, m in enumerate(map_meas):
        own_tracks[j]["covariance"], own_tracks[j]["id"], own_tracks[j]["flags"] = m["covariance"], 100 + j, ca.MAP_TRACK_STAGED if j % 2 == 0 else 0
    lines = [f"cape_map_maintain against cape_map_download + cape_host_map_maintain + cape_map_upload + cape_map_upload_tracks: room stream, frames {picks}, "
             f"{a.reps} repetitions behind 3 warm-up repetitions, the two routes alternating"]
    for size in (len(own[0]), 896):
        arrays, tracks = (own, own_tracks) if size == len(own[0]) else wall_copies(ca, map_meas, own_tracks, size)
        the_call(ca, ex, st, torch, arrays, tracks, a.reps, lines)
    # the loop: the staged planes one match short of promotion, the local ones one miss short of being lost
    loop_tracks = own_tracks.copy()
    loop_tracks["successive_matched"] = np.where(loop_tracks["flags"] & ca.MAP_TRACK_STAGED, 3, 0)
    loop_tracks["failed_tracking"] = np.where(loop_tracks["flags"] & ca.MAP_TRACK_STAGED, 0, 9)
    the_loop(ca, ex, st, torch, n, own, loop_tracks, W2C, a.reps, lines)
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
