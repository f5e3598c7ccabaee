"""cape_map_step against the five calls it stands for -- cape_match_map_wide, cape_map_kalman, cape_map_union_cut, cape_map_commit and
cape_map_maintain -- on the eight room frames of tests/test_gpu_map_kalman.py (room stream, seed 11, frames 20, 25, .. 55; the map: the
stageable planes of the first frame with several planes, the staged ones one match short of promotion, the local ones one miss short of
being lost, as profiles/map_maintain_rate.py's loop has them).

1. One frame.  Per repetition the map and tracks are uploaded again and the retired log is cleared, untimed; then a host clock around
     the step:       cape_map_step(0), which returns after its one stream synchronise;
     the five calls: the same frame with n_frames = 1 -- the one-frame prefix, the only like-for-like route -- where the commit and
                     the maintenance each return after a stream synchronise of their own.
   The map, tracks, log and headers the two leave are compared once, byte for byte.
2. The loop.  For f = 0 .. 7 on the same batch, no upload in between: cape_map_step(f) -- against the loop of
   profiles/map_maintain_rate.py, which matches, filters and unites all eight frames for every frame it commits and maintains.  A host
   clock around the eight frames, divided by eight.
The routes alternate repetition by repetition in one run; the figures are medians with their ranges.

    python profiles/map_step_rate.py [--reps 30] [--out profiles/map_step_rate.txt]"""
import argparse
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


def five_calls(ca, ex, st, n, f, W2C, next_id):
    ex.match_map_wide(n, W2C[:n], None, ca.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)
    commit, next_id = ex.map_commit(f, ca.COMMIT_ADD_STAGED, next_id, st)
    if not commit["flags"] & ca.COMMIT_DONE:
        raise ca.CapeError(f"frame {f} is refused ({int(commit['flags']):#x})")
    return commit, ex.map_maintain(0, st), next_id


def step(ca, ex, st, f, W2C, next_id):
    result, next_id = ex.map_step(f, W2C[f], None, ca.MATCH_ALLOW_INDEX0, ca.COMMIT_ADD_STAGED, next_id, st)
    if not result["commit"]["flags"] & ca.COMMIT_DONE:
        raise ca.CapeError(f"frame {f} is refused ({int(result['commit']['flags']):#x})")
    return result["commit"], result["maintain"], next_id


def state(ex):
    (P, R, V), T = ex.download_map()
    (LP, LR, LV), LT = ex.download_retired()
    return [np.ascontiguousarray(a).tobytes() for a in (P, R, V, T, LP, LR, LV, LT)]


def measure(ca, ex, st, torch, arrays, tracks, reps, routes):
    """routes: name -> run() returning what to compare; each repetition starts from a fresh upload and the cleared log"""
    ms, left = {k: [] for k in routes}, {}
    for rep in range(len(routes) * (reps + 3)):
        name = list(routes)[rep % len(routes)]
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.clear_retired()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        headers = routes[name]()
        t1 = time.perf_counter()
        if rep >= len(routes) * 3:
            ms[name].append((t1 - t0) * 1e3)
        left[name] = [h.tobytes() for h in headers] + state(ex)
    return ms, left


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
    tracks["successive_matched"] = np.where(tracks["flags"] & ca.MAP_TRACK_STAGED, 3, 0)
    tracks["failed_tracking"] = np.where(tracks["flags"] & ca.MAP_TRACK_STAGED, 0, 9)
    lines = [f"cape_map_step against cape_match_map_wide + cape_map_kalman + cape_map_union_cut + cape_map_commit + cape_map_maintain: room stream, frames "
             f"{picks}, a map of {len(arrays[0])} planes, {a.reps} repetitions behind 3 warm-up repetitions, the routes alternating"]

    # 1. one frame
    ms, left = measure(ca, ex, st, torch, arrays, tracks, a.reps, {
        "step": lambda: step(ca, ex, st, 0, W2C, 1000)[:2],
        "five": lambda: five_calls(ca, ex, st, 1, 0, W2C, 1000)[:2]})
    assert left["step"] == left["five"], "the step and the five calls leave different bytes"
    b, c = statistics.median(ms["step"]), statistics.median(ms["five"])
    lines.append(f"one frame, frame 0 alone (headers, map, tracks and log equal byte for byte): cape_map_step(0) {spread(ms['step'])}; the five calls "
                 f"with n_frames = 1 {spread(ms['five'])}; difference of the medians {(c - b) * 1e3:.1f} us, ratio {c / b:.2f}")

    # 2. the loop
    def loop(one):
        def run():
            next_id, last = 1000, None
            for f in range(n):
                *last, next_id = one(f, next_id)
            return last
        return run

    ms, left = measure(ca, ex, st, torch, arrays, tracks, a.reps, {
        "step": loop(lambda f, nid: step(ca, ex, st, f, W2C, nid)),
        "five": loop(lambda f, nid: five_calls(ca, ex, st, n, f, W2C, nid))})
    assert left["step"] == left["five"], "the two loops leave different bytes"
    b, c = statistics.median(ms["step"]) / n, statistics.median(ms["five"]) / n
    per = {k: [v / n for v in ms[k]] for k in ms}
    lines.append(f"the loop of eight frames (map, tracks and log equal byte for byte after it): period per frame by cape_map_step(f) {spread(per['step'])}; "
                 f"by the five calls on all eight frames per committed frame {spread(per['five'])}; difference of the medians {(c - b) * 1e3:.1f} us, "
                 f"ratio {c / b:.2f}")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
