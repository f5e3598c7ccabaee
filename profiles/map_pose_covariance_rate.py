"""cape_map_pose_covariance (device events after warm-up) behind the chain of profiles/map_pose_solve_rate.py on its 4 096-frame room batch
against a map of 64 planes: 119 three-pair subsets per frame, score, select, the refit, then the covariance of every refitted pose at
100 iterations with CAPE_POSE_COVARIANCE_FROM_SOLUTION -- Philox deviates, the frames in chunks through the slab's default budget.  Beside
the call as a whole: what its samples take (nfev; they start at the optimum), the replaced route (the refit's rows and the selection
copied to the host, cape_host_pose_covariance on 16 threads over the frames whose refit ran) and the plain solve of the same batch.
The figure is the whole call's -- pairs kernel, vary and solve per chunk, reduce; a split per kernel needs a kernel trace of one call
(`rocprofv3 --kernel-trace --stats -- python profiles/map_pose_covariance_rate.py --rounds 1 --reps 1`) and has not been recorded.

    python profiles/map_pose_covariance_rate.py [--frames 4096] [--iterations 100] [--out profiles/map_pose_covariance_rate.txt]"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from map_pose_solve_rate import N_SUBSETS, spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--twin-frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd as ca
    from cape_amd import Extractor, synth, synth_gpu
    from map_match_wide_rate import lift
    from test_gpu_pose_solve import _starts, _subsets

    st = torch.cuda.current_stream().cuda_stream
    n, it = a.frames, a.iterations
    lines = [f"cape_map_pose_covariance, {a.rounds} rounds of {a.reps} enqueues behind 2 warm-up calls, device events; the twin by a host clock"]
    rng = np.random.default_rng(0)
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
    tracks = np.zeros(64, ca.MAP_TRACK_DTYPE)
    for j in range(64):
        # standard deviations of 1e-4 .. 1e-3 in a normal's component and 0.1 .. 2 mm in a distance
        tracks[j]["covariance"], tracks[j]["id"] = np.diag(np.concatenate([rng.uniform(1e-4, 1e-3, 3), rng.uniform(0.1, 2.0, 1)]) ** 2), 100 + j
    arrays = ca.pack_map(planes)
    W2C = np.zeros((n, 4, 4))
    for f, (R, o) in enumerate(c2w):
        W2C[f, :3, :3], W2C[f, :3, 3], W2C[f, 3, 3] = R.T, -R.T @ o, 1.0
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    _, match, _, _ = ex.map_matches_wide(n)
    pairs = (match >= 0).sum(axis=1)
    lines.append(f"the room batch against a map of 64 planes: {n} frames, {pairs.sum() / n:.2f} pairs per frame, {int((pairs >= 3).sum())} frames with three or more")
    x0, subsets = _starts(rng, W2C, N_SUBSETS), _subsets(rng, match, N_SUBSETS, 3)
    dx, ds = torch.from_numpy(x0).cuda(), torch.from_numpy(subsets.view(np.int32)).cuda()
    torch.cuda.synchronize()
    solve = lambda: ex.map_pose_solve(n, dx.data_ptr(), ds.data_ptr(), flags=ca.POSE_SOLVE_DEVICE_INPUT, n_hypotheses=N_SUBSETS, stream=st)  # noqa: E731
    ms_solve = timed(torch, solve, a.rounds, a.reps)
    rows, _ = ex.pose_solutions(n)
    ran = rows["status"] > 0
    lines.append(f"  cape_map_pose_solve, {N_SUBSETS} three-pair subsets per frame: {spread(ms_solve)}, {int(ran.sum())} of {ran.size} ran "
                 f"({ran.sum() / statistics.median(ms_solve) / 1e3:.3f} M minimisations/s), nfev mean {rows['nfev'][ran].mean():.1f}")
    ex.map_pose_score(n, ex.pose_solve_device()[1], ca.POSE_SCORE_DEVICE_POSES, n_hypotheses=N_SUBSETS, stream=st)
    ex.map_pose_select(n, st)
    ex.map_pose_solve(n, flags=ca.POSE_SOLVE_FROM_SELECTION, stream=st)
    refit, _ = ex.pose_solutions(n)
    sel = ex.pose_selection(n)
    ok = refit[:, 0]["status"] > 0
    covariance = lambda: ex.map_pose_covariance(n, it, seed=2026, flags=ca.POSE_COVARIANCE_FROM_SOLUTION, stream=st)  # noqa: E731
    ms = timed(torch, covariance, a.rounds, a.reps)
    out = ex.pose_covariance(n)
    d = statistics.median(ms)
    done = out["status"] >= -17
    samples = int(ok.sum()) * it
    lines.append(f"  cape_map_pose_covariance, {it} iterations, FROM_SOLUTION, Philox, {-(-n // ((256 << 20) // (4096 * it)))} chunks of frames: {spread(ms)}; "
                 f"{int(ok.sum())} frames with a refit = {samples} samples ({samples / d / 1e3:.3f} M minimisations/s); statuses "
                 f"{dict(zip(*[v.tolist() for v in np.unique(out['status'], return_counts=True)]))}")
    valid = out["status"] == ca.POSE_COVARIANCE_VALID
    if valid.any():
        v = out[valid]
        lines.append(f"  the samples start at the optimum: nfev {int(v['nfev_min'].min())} .. {int(v['nfev_max'].max())}, mean {v['nfev_sum'].sum() / (len(v) * it):.1f} "
                     f"(the hypotheses of the solve above: mean {rows['nfev'][ran].mean():.1f}); n_ok {int(v['n_ok'].min())} .. {int(v['n_ok'].max())}; "
                     f"median position variances {np.median(v['covariance'][:, 0, 0]):.4g} {np.median(v['covariance'][:, 1, 1]):.4g} {np.median(v['covariance'][:, 2, 2]):.4g} mm^2")
    assert done.any()
    # ---- the replaced route: the refit's rows and the selection on the host, the twin on 16 threads over the frames whose refit ran
    frames = np.flatnonzero(ok)[:: max(1, int(ok.sum()) // a.twin_frames)][: a.twin_frames]
    det = {int(f): np.array([[*k[0], k[1]] for k in kept[f][0]], np.float64).reshape(-1, 4) for f in frames}

    def twin(f):
        return ca.host_pose_covariance(arrays, tracks, match[f], det[int(f)], it, solution=refit[f, 0], selection=sel[f], seed=2026, frame_index=int(f))[0]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        twins = list(pool.map(twin, frames))
    twin_ms = (time.perf_counter() - t0) * 1e3
    same = sum(int(t["n_ok"] == out[f]["n_ok"] and t["status"] == out[f]["status"]) for t, f in zip(twins, frames))
    t0 = time.perf_counter()
    ex.pose_solutions(n), ex.pose_selection(n)
    copy_ms = (time.perf_counter() - t0) * 1e3
    scaled = twin_ms * int(ok.sum()) / max(1, len(frames))
    lines.append(f"  the replaced route: copies of the refit and the selection {copy_ms:.2f} ms; cape_host_pose_covariance on 16 threads, {len(frames)} frames x {it} "
                 f"iterations: {twin_ms:.1f} ms = {scaled:.0f} ms for the {int(ok.sum())} frames = {(scaled + copy_ms) / d:.0f} x the device call (through the Python "
                 f"wrapper, which packs the map per call); {same} of {len(frames)} frames with the device's n_ok and status")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
