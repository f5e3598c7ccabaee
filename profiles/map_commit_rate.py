"""cape_map_commit against the route it replaces -- cape_host_map_update + cape_map_upload + cape_map_upload_tracks -- on the eight room
frames of tests/test_gpu_map_kalman.py (room stream, seed 11, frames 20, 25, .. 55; the map: the stageable planes of the first frame
with several planes; and that map filled up to 896 planes with copies of its planes a little off, as the 1 024-plane maps of the other
profiles are made), one frame at a time, as a tracking loop meets them.

Per frame and repetition the map and the tracks are uploaded again and the wide match, the Kalman step and cape_map_union_cut run
untimed; then
  the commit:     a host clock around cape_map_commit(frame, CAPE_COMMIT_ADD_STAGED), which returns after its own stream synchronise,
                  and device events around the same call (the two kernels and the header's copy);
  the host route: a host clock around the C call cape_host_map_update (arrays packed beforehand, the device's own match) followed by
                  Extractor.upload_map and Extractor.upload_tracks of its result, which are synchronous.
The two routes alternate repetition by repetition in one run; the figures are medians over the repetitions.

    python profiles/map_commit_rate.py [--reps 30] [--out profiles/map_commit_rate.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))


def host_update_call(ca, arrays, tracks, match, detected, T, S, next_id):
    """cape_host_map_update with CAPE_MAP_ADD_STAGED, prepared: returns run() -> ((planes, rings, vertices), tracks)"""
    L = ca._host_library()
    src, src_view = ca._map_arrays(arrays, np.ascontiguousarray(tracks, ca.MAP_TRACK_DTYPE))
    M = np.ascontiguousarray(match, np.int32)
    cols, det_view = ca._pack_detected(detected, with_cov=True)
    T, S = np.ascontiguousarray(T, np.float64).reshape(16), np.ascontiguousarray(S, np.float64).reshape(9)
    n = len(src["planes"]) + len(detected)
    out = dict(planes=np.zeros(n, ca.MAP_PLANE_DTYPE), rings=np.zeros(9 * n, ca.MAP_RING_DTYPE),
               vertices=np.zeros((len(src["vertices"]) + len(cols["vertices"]) + 4096, 2)), tracks=np.zeros(n, ca.MAP_TRACK_DTYPE))
    used = np.zeros(max(len(detected), 1), np.int32)

    def run():
        nid = C.c_uint64(next_id)
        v = ca._view(ca.cape_host_map, out, planes_capacity=len(out["planes"]), rings_capacity=len(out["rings"]), vertices_capacity=len(out["vertices"]))
        rc = L.cape_host_map_update(C.byref(src_view), ca._as(M, C.c_int32), C.byref(det_view), ca._as(T, C.c_double), ca._as(S, C.c_double),
                                    ca.MAP_ADD_STAGED, C.byref(nid), C.byref(v), ca._as(used, C.c_int32))
        if rc != 0:
            raise ca.CapeError(f"cape_host_map_update failed ({rc})")
        return (out["planes"][:v.n_planes], out["rings"][:v.n_rings], out["vertices"][:v.n_vertices]), out["tracks"][:v.n_planes], (src, cols)

    return run


def spread(ms):
    return f"median {statistics.median(ms) * 1e3:8.1f} us (min {min(ms) * 1e3:8.1f}, max {max(ms) * 1e3:8.1f} over {len(ms)} repetitions)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd as ca
    from cape_amd import Extractor, synth, synth_gpu

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
    arrays = ca.pack_map([m["plane"] for m in map_meas])
    tracks = np.zeros(len(map_meas), ca.MAP_TRACK_DTYPE)
    for j, m in enumerate(map_meas):
        tracks[j]["covariance"], tracks[j]["id"], tracks[j]["flags"] = m["covariance"], 100 + j, ca.MAP_TRACK_STAGED if j % 2 == 0 else 0
    res = ex.results(n, with_boundary=False)
    kept = ex.kept_planes(n)
    det = [[d + (res.segments(f)[s]["cov"].reshape(3, 3).copy(),) for d, s in zip(*kept[f])] for f in range(n)]

    own, own_tracks = arrays, tracks
    lines = []
    for size in (len(own[0]), 896):
        arrays, tracks = (own, own_tracks) if size == len(own[0]) else wall_copies(ca, map_meas, own_tracks, size)
        measure(ca, ex, st, torch, n, picks, arrays, tracks, W2C, T, S, det, a.reps, lines)
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


def wall_copies(ca, map_meas, own_tracks, size):
    """the map's own planes, then copies of them a little off (profiles/map_kalman_rate.py)"""
    rng = np.random.default_rng(0)
    planes, tracks = [m["plane"] for m in map_meas], np.zeros(size, ca.MAP_TRACK_DTYPE)
    tracks[:len(own_tracks)] = own_tracks
    while len(planes) < size:
        at = int(rng.integers(len(map_meas)))
        nw, d, x, y, c, ring, h = map_meas[at]["plane"]
        j = len(planes)
        planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        tracks[j]["covariance"], tracks[j]["id"], tracks[j]["flags"] = map_meas[at]["covariance"], 100 + j, ca.MAP_TRACK_STAGED if j % 2 == 0 else 0
    return ca.pack_map(planes), tracks


def measure(ca, ex, st, torch, n, picks, arrays, tracks, W2C, T, S, det, reps, lines):
    def prepare():
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
        ex.map_kalman(n, st)
        ex.map_union_cut(n, st)
        torch.cuda.synchronize()

    prepare()
    _, match, _, _ = ex.map_matches_wide(n)
    host_calls = [host_update_call(ca, arrays, tracks, match[f], det[f], T[f], S[f], 1000) for f in range(n)]
    lines.append(f"cape_map_commit against cape_host_map_update + cape_map_upload + cape_map_upload_tracks: room stream, frames {picks}, a map of "
                 f"{len(arrays[0])} planes, one frame per call, {reps} repetitions per frame behind 3 warm-up repetitions, the two routes alternating")
    all_commit, all_span, all_host = [], [], []
    for f in range(n):
        commit_ms, span_ms, host_ms, result = [], [], [], None
        for rep in range(reps + 3):
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            result, _ = ex.map_commit(f, ca.COMMIT_ADD_STAGED, 1000, st)
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            new, new_tracks, _ = host_calls[f]()
            ex.upload_map(new)
            ex.upload_tracks(new_tracks)
            t3 = time.perf_counter()
            if rep >= 3:
                commit_ms.append((t1 - t0) * 1e3)
                span_ms.append(e0.elapsed_time(e1))
                host_ms.append((t3 - t2) * 1e3)
        lines.append(f"frame {f}: flags {int(result['flags']):#x}, {int(result['n_updated'])} updated, {int(result['n_appended'])} appended, "
                     f"{int(result['n_planes'])} planes / {int(result['n_vertices'])} vertices after; commit call {spread(commit_ms)}, device span "
                     f"{spread(span_ms)}; host route {spread(host_ms)}; ratio of the medians (host route / commit) "
                     f"{statistics.median(host_ms) / statistics.median(commit_ms):.1f}")
        all_commit += commit_ms
        all_span += span_ms
        all_host += host_ms
    lines.append(f"all frames: commit call {spread(all_commit)}, device span {spread(all_span)}; host route {spread(all_host)}; ratio of the medians "
                 f"(host route / commit) {statistics.median(all_host) / statistics.median(all_commit):.1f}")


if __name__ == "__main__":
    main()
