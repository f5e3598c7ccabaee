"""cape_map_pose_score (device events after warm-up) at 1, 64 and 256 hypotheses per frame, with the poses in host memory (through the
pinned twin) and in device memory (CAPE_POSE_SCORE_DEVICE_POSES), on
  1. the eight room frames of the map tests (room stream, seed 11, frames 20, 25, .. 55) against their own map, and
  2. the 4 096-frame room batch with the poses of its trajectory against a map of 64 planes (the map of profiles/map_kalman_rate.py);
and the route it replaces: the copies a caller needs to build the features on the host -- cape_copy_map_matches_wide, cape_map_download
with its tracks, cape_copy_results for the records (a host clock around the three) -- plus 16 threads over the host twin
cape_host_pose_score, one call per frame (the C call only: the arrays are packed beforehand).  The hypotheses are the frame's pose and
perturbed ones (up to 3 degrees, up to 100 mm), the same perturbations for every frame.

    python profiles/map_pose_score_rate.py [--frames 4096] [--out profiles/map_pose_score_rate.txt]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def perturbations(rng, n_hyp):
    """(n_hyp, 4, 4): the identity, then rigid motions of up to 3 degrees and 100 mm"""
    D = np.tile(np.eye(4), (n_hyp, 1, 1))
    for h in range(1, n_hyp):
        k = rng.normal(size=3)
        k /= np.linalg.norm(k)
        a = rng.uniform(-math.radians(3.0), math.radians(3.0))
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        D[h, :3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
        D[h, :3, 3] = rng.uniform(-100.0, 100.0, 3)
    return D


def host_twin_call(ca, arrays, tracks, match, det, poses):
    """cape_host_pose_score, prepared: returns run() -> (inliers of all hypotheses, the arrays it keeps alive)"""
    L = ca._host_library()
    src, src_view = ca._map_arrays(arrays, tracks)
    match = np.ascontiguousarray(match, np.int32)
    det = np.ascontiguousarray(det, np.float64).reshape(-1, 4)
    det_view = ca._view(ca.cape_host_planes, dict(planes=det), n=len(det))
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
    scores = np.zeros(len(poses), ca.POSE_SCORE_DTYPE)

    def run():
        rc = L.cape_host_pose_score(C.byref(src_view), ca._as(match, C.c_int32), C.byref(det_view), 0, len(poses), ca._as(poses, C.c_double),
                                    scores.ctypes.data, None, None)
        if rc != 0:
            raise ca.CapeError(f"cape_host_pose_score failed ({rc})")
        return int(scores["n_inliers"].sum()), (src, match, det, poses, scores)

    return run


def spread(ms):
    return f"{statistics.median(ms):9.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})"


def measure(ca, torch, ex, st, n, W2C, arrays, tracks, kept, what, rounds, reps, lines):
    rng = np.random.default_rng(3)
    _, match, _, _ = ex.map_matches_wide(n)
    pairs = int((match >= 0).sum())
    det = [np.array([[*k[0], k[1]] for k in kept[f][0]], np.float64).reshape(-1, 4) for f in range(n)]
    lines.append(f"{what}: {n} frames, a map of {len(arrays[0])} planes, {pairs} pairs in all ({pairs / n:.2f} per frame)")
    # the copies of the replaced route, once per batch whatever the number of hypotheses
    copy_ms = []
    for _ in range(1 + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex.map_matches_wide(n)
        ex.download_map()
        ex.results(n, with_boundary=False)
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    copy_ms = copy_ms[1:]
    for n_hyp in (1, 64, 256):
        poses = np.ascontiguousarray(np.einsum("hij,fjk->fhik", perturbations(rng, n_hyp), W2C))
        dev = torch.from_numpy(poses).cuda()
        calls = {"host poses": lambda: ex.map_pose_score(n, poses, 0, stream=st),
                 "device poses": lambda: ex.map_pose_score(n, dev.data_ptr(), ca.POSE_SCORE_DEVICE_POSES, n_hypotheses=n_hyp, stream=st)}
        ms = {k: [] for k in calls}
        for call in calls.values():
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        for _ in range(rounds):  # the two routes alternate round by round
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / reps)
        scores = ex.pose_scores(n)
        twins = [host_twin_call(ca, arrays, tracks, match[f], det[f], poses[f]) for f in range(n)]
        host_ms = []
        for _ in range(1 + max(1, rounds // 2)):
            with ThreadPoolExecutor(16) as pool:
                t0 = time.perf_counter()
                out = list(pool.map(lambda run: run(), twins))
                host_ms.append((time.perf_counter() - t0) * 1e3)
        host_ms = host_ms[1:]
        inliers = sum(k for k, _ in out)
        assert inliers == int(scores["n_inliers"].sum()), "the device and the twin count different inliers"
        d = statistics.median(ms["device poses"])
        evaluations = pairs * n_hyp
        lines.append(f"  {n_hyp:3d} hypotheses per frame: cape_map_pose_score, host poses {spread(ms['host poses'])}; device poses {spread(ms['device poses'])} = "
                     f"{n * n_hyp / d / 1e3:9.2f} M (frame, hypothesis) rows/s, {evaluations / d / 1e3:9.2f} M pair evaluations/s; replaced route: copies "
                     f"{spread(copy_ms)} + 16 threads over cape_host_pose_score {spread(host_ms)} = "
                     f"{(statistics.median(copy_ms) + statistics.median(host_ms)) / statistics.median(ms['host poses']):8.1f}x the call with host poses; "
                     f"{inliers} inliers of {evaluations} evaluations on both routes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd as ca
    from cape_amd import Extractor, synth, synth_gpu
    from map_match_wide_rate import lift

    st = torch.cuda.current_stream().cuda_stream
    lines = [f"cape_map_pose_score, {a.rounds} rounds of {a.reps} enqueues behind 3 warm-up calls per route, device events; the replaced route by a host clock"]

    def poses_of(c2w):
        W2C = np.zeros((len(c2w), 4, 4))
        for f, (R, o) in enumerate(c2w):
            W2C[f, :3, :3], W2C[f, :3, 3], W2C[f, 3, 3] = R.T, -R.T @ o, 1.0
        return W2C

    def tracks_for(n_planes, rng):
        tracks = np.zeros(n_planes, ca.MAP_TRACK_DTYPE)
        for j in range(n_planes):
            A = rng.normal(size=(4, 4))
            tracks[j]["covariance"], tracks[j]["id"] = 1e-3 * (A @ A.T + 4 * np.eye(4)), 100 + j
        return tracks

    # 1. the eight room frames against their own map
    n, seed, start, stride = 8, 11, 20, 5
    picks = [start + stride * i for i in range(n)]
    dev = torch.cat([synth_gpu.stream("room", seed, 1, start=f, device="cuda", chunk=1) for f in picks]).contiguous()
    all_poses = synth_gpu._poses("room", seed, 0, start + stride * n)
    c2w = [all_poses[f] for f in picks]
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    kept = ex.kept_planes(n)
    rng = np.random.default_rng(0)
    planes = [lift(k, *c2w[f]) for f in (4, 5) for k in kept[f][0]]
    arrays, tracks = ca.pack_map(planes), tracks_for(len(planes), rng)
    W2C = poses_of(c2w)
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    measure(ca, torch, ex, st, n, W2C, arrays, tracks, kept, "the eight room frames against the map of frames 4 and 5", a.rounds, a.reps, lines)
    ex.close()

    # 2. the batch
    n = a.frames
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    c2w = synth_gpu._poses("room", 1, 0, n)
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    kept = ex.kept_planes(n)
    base = [lift(k, *c2w[f]) for f in range(0, n, max(1, n // 16)) for k in kept[f][0]]
    planes = list(base[:64])
    while len(planes) < 64:
        nw, d, x, y, c, ring, h = base[int(rng.integers(len(base)))]
        planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
    arrays, tracks = ca.pack_map(planes), tracks_for(64, rng)
    W2C = poses_of(c2w)
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    measure(ca, torch, ex, st, n, W2C, arrays, tracks, kept, "the room batch against a map of 64 planes", a.rounds, a.reps, lines)
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
