"""cape_map_pose_solve / cape_map_pose_select (device events after warm-up), the inputs in device memory, on
  1. the 4 096-frame room batch with the poses of its trajectory against a map of 64 planes (the batch of profiles/map_pose_score_rate.py):
     119 subsets of three of the frame's pairs per frame (every pair where the frame has fewer: such a problem is refused, and the room
     shows two or three planes per frame, so most are), then score, select and one refit per frame from the selection;
  2. the chained checkerboard frame of the tests (116 facets in four orientations, its own planes as the map): 119 three-pair subsets
     and the refit over every inlier, where every problem runs;
with the spread of nfev inside each wave of 64 problems (the wave runs to its slowest lane) and the single-thread time of the host twin
cape_host_pose_solve on the same problems (a sample of the batch's frames, scaled).

    python profiles/map_pose_solve_rate.py [--frames 4096] [--out profiles/map_pose_solve_rate.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_SUBSETS = 119  # maximumIterations of pose_optimization.cpp:129-132


def spread(ms):
    return f"{statistics.median(ms):9.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})"


def timed(torch, call, rounds, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def measure(ca, torch, ex, st, n, W2C, arrays, tracks, kept, what, rounds, reps, twin_frames, lines):
    from test_gpu_pose_solve import _starts, _subsets

    rng = np.random.default_rng(5)
    _, match, _, _ = ex.map_matches_wide(n)
    pairs = (match >= 0).sum(axis=1)
    lines.append(f"{what}: {n} frames, a map of {len(arrays[0])} planes, {pairs.sum() / n:.2f} pairs per frame, {int((pairs >= 3).sum())} frames with three or more")
    x0 = _starts(rng, W2C, N_SUBSETS)
    subsets = _subsets(rng, match, N_SUBSETS, 3)
    dx, ds = torch.from_numpy(x0).cuda(), torch.from_numpy(subsets.view(np.int32)).cuda()
    torch.cuda.synchronize()
    solve = lambda: ex.map_pose_solve(n, dx.data_ptr(), ds.data_ptr(), flags=ca.POSE_SOLVE_DEVICE_INPUT, n_hypotheses=N_SUBSETS, stream=st)  # noqa: E731
    ms = timed(torch, solve, rounds, reps)
    rows, _ = ex.pose_solutions(n)
    ran = rows["status"] > 0
    d = statistics.median(ms)
    lines.append(f"  cape_map_pose_solve, {N_SUBSETS} three-pair subsets per frame: {spread(ms)} = {n * N_SUBSETS / d / 1e3:9.2f} M problems/s in all, "
                 f"{int(ran.sum())} of {ran.size} ran ({ran.sum() / d / 1e3:9.3f} M minimisations/s), statuses "
                 f"{dict(zip(*[v.tolist() for v in np.unique(rows['status'], return_counts=True)]))}")
    if ran.any():
        # the waves of the kernel: 64 consecutive problems of a frame (119 = 64 + 55)
        lo, hi, idle = [], [], 0
        for f in np.flatnonzero(ran.any(axis=1)):
            for a in (0, 64):
                w, r = rows[f, a: a + 64]["nfev"], ran[f, a: a + 64]
                if r.any():
                    lo.append(int(w[r].min())), hi.append(int(w[r].max()))
                    idle += int(w[r].max()) * len(w) - int(w.sum())
        nfev = rows["nfev"][ran]
        lines.append(f"  nfev of the problems that ran: {int(nfev.min())} .. {int(nfev.max())}, mean {nfev.mean():.1f}; per wave of 64 the slowest lane needs "
                     f"{statistics.mean(hi):.1f} evaluations on average against {statistics.mean(lo):.1f} for the fastest: "
                     f"{idle / max(1, sum(h * 64 for h in hi)):.1%} of the lane-evaluations of a wave with work are idle (refused lanes included)")
    # score, select, refit: the rest of the chain
    _, pose_ptr = ex.pose_solve_device()
    score = lambda: ex.map_pose_score(n, pose_ptr, ca.POSE_SCORE_DEVICE_POSES, n_hypotheses=N_SUBSETS, stream=st)  # noqa: E731
    ms_score = timed(torch, score, rounds, reps)
    ms_select = timed(torch, lambda: ex.map_pose_select(n, st), rounds, reps)
    sel = ex.pose_selection(n)
    ms_refit = timed(torch, lambda: ex.map_pose_solve(n, flags=ca.POSE_SOLVE_FROM_SELECTION, stream=st), rounds, reps)
    refit, _ = ex.pose_solutions(n)
    ok = refit[:, 0]["status"] > 0
    lines.append(f"  cape_map_pose_score of the solve's poses {spread(ms_score)}; cape_map_pose_select {spread(ms_select)} ({int((sel['best'] >= 0).sum())} frames "
                 f"with a best); refit, 1 problem per frame {spread(ms_refit)} = {n / statistics.median(ms_refit) / 1e3:9.3f} M problems/s, {int(ok.sum())} ran, "
                 f"pairs used up to {int(refit['n_pairs_used'].max())}, nfev up to {int(refit['nfev'].max())}")
    # the twin, one thread, on a sample of the frames
    sample = list(range(0, n, max(1, n // twin_frames)))[:twin_frames]
    det = [np.array([[*k[0], k[1]] for k in kept[f][0]], np.float64).reshape(-1, 4) for f in sample]
    t0 = time.perf_counter()
    for i, f in enumerate(sample):
        r, _, _ = ca.host_pose_solve(arrays, tracks, match[f], det[i], x0[f], subsets[f])
        assert r.tobytes() == rows[f].tobytes(), f"frame {f}: the device and the twin differ"
    twin_ms = (time.perf_counter() - t0) * 1e3
    lines.append(f"  cape_host_pose_solve, one thread, {len(sample)} frames x {N_SUBSETS} problems: {twin_ms:.2f} ms = {twin_ms * n / len(sample):.1f} ms for the "
                 f"{n} frames = {twin_ms * n / len(sample) / d:.1f} x the device call (through the Python wrapper, which packs the map per call)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd as ca
    from cape_amd import Extractor, synth, synth_gpu
    from map_match_wide_rate import lift

    st = torch.cuda.current_stream().cuda_stream
    lines = [f"cape_map_pose_solve, {a.rounds} rounds of {a.reps} enqueues behind 2 warm-up calls, device events, x0 and subsets in device memory; the twin by a host clock"]

    def tracks_for(n_planes, rng):
        tracks = np.zeros(n_planes, ca.MAP_TRACK_DTYPE)
        for j in range(n_planes):
            A = rng.normal(size=(4, 4))
            tracks[j]["covariance"], tracks[j]["id"] = 1e-3 * (A @ A.T + 4 * np.eye(4)), 100 + j
        return tracks

    rng = np.random.default_rng(0)
    # 1. the batch
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
    W2C = np.zeros((n, 4, 4))
    for f, (R, o) in enumerate(c2w):
        W2C[f, :3, :3], W2C[f, :3, 3], W2C[f, 3, 3] = R.T, -R.T @ o, 1.0
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    measure(ca, torch, ex, st, n, W2C, arrays, tracks, kept, "the room batch against a map of 64 planes", a.rounds, a.reps, 64, lines)
    ex.close()
    del dev

    # 2. the chained checkerboard frame between two room frames
    from test_gpu_match_map_wide import _chained_input
    from test_gpu_match_wide import _small_pose

    frames, Wd, Ht, intr = _chained_input()
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    ex = Extractor(Wd, Ht, cylinders=False, max_batch=len(frames), **intr)
    ex.extract_device(dev.data_ptr(), len(frames), st)
    ex.build_polygons(len(frames), st)
    kept = ex.kept_planes(len(frames))
    eye = (np.eye(3), np.zeros(3))
    planes = [lift(k, *eye) for k in kept[1][0]][::-1]
    arrays, tracks = ca.pack_map(planes), tracks_for(len(planes), rng)
    W2C = _small_pose(len(frames))
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(len(frames), W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    measure(ca, torch, ex, st, len(frames), W2C, arrays, tracks, kept, "[room, checkerboard of 116 facets, room] against the checkerboard's own planes",
            a.rounds, a.reps, 3, lines)
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
