"""cape_map_kalman beside the cape_match_map_wide that feeds it (device events after warm-up, the two calls alternating round by round in
one run) on the 4 096-frame room batch with the poses of its trajectory, a pose covariance of a few mm^2 per frame and maps of 64 and
1 024 planes (the maps of profiles/map_match_wide_rate.py, each track holding the covariance of the measurement its plane came from);
and the same frames through the host twin: 16 threads over cape_host_map_kalman, one call per frame, fed with the device's match and
measurement rows (the C call only: the arrays are packed beforehand).

    python profiles/map_kalman_rate.py [--frames 4096] [--out profiles/r12_map_kalman.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def host_kalman_call(ca, arrays, tracks, match, rows_in):
    """cape_host_map_kalman, prepared: returns run() -> (n_updated, the arrays it keeps alive)"""
    L = ca._host_library()
    src, src_view = ca._map_arrays(arrays, tracks)
    match = np.ascontiguousarray(match, np.int32)
    rows_in = np.ascontiguousarray(rows_in, ca.PLANE_MEASUREMENT_DTYPE)
    frame = np.zeros(1, ca.FRAME_MAP_KALMAN_DTYPE)
    rows = np.zeros(max(len(rows_in), 1), ca.PLANE_FUSION_DTYPE)
    results = np.zeros(max(len(match), 1), ca.MAP_TRACK_RESULT_DTYPE)

    def run():
        rc = L.cape_host_map_kalman(C.byref(src_view), ca._as(match, C.c_int32), rows_in.ctypes.data, len(rows_in), frame.ctypes.data,
                                    rows.ctypes.data, results.ctypes.data)
        if rc != 0:
            raise ca.CapeError(f"cape_host_map_kalman failed ({rc})")
        return int(frame[0]["n_updated"]), (src, match, rows_in, rows, results)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu
    from map_match_wide_rate import lift, spread

    st = torch.cuda.current_stream().cuda_stream

    n = a.frames
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    c2w = synth_gpu._poses("room", 1, 0, n)
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    kept = ex.kept_planes(n)
    rng = np.random.default_rng(0)
    T, W2C, S = np.zeros((n, 4, 4)), np.zeros((n, 4, 4)), np.zeros((n, 3, 3))
    for f in range(n):
        R, o = c2w[f]
        T[f, :3, :3], T[f, :3, 3], T[f, 3, 3] = R, o, 1.0
        W2C[f, :3, :3], W2C[f, :3, 3], W2C[f, 3, 3] = R.T, -R.T @ o, 1.0
        A = rng.normal(size=(3, 3))
        S[f] = A @ A.T + 3 * np.eye(3)
    ex.map_measure(n, T, S, st)
    mrows, _ = ex.measurement_rows(n)
    # the maps of map_match_wide_rate.py; each plane's track holds the covariance of the measurement it came from
    src = [(f, k, s) for f in range(0, n, max(1, n // 16)) for k, s in zip(*kept[f])]
    base = [lift(k, *c2w[f]) for f, k, _ in src]
    base_cov = [mrows[f, s]["covariance"].copy() for f, _, s in src]
    lines = [f"cape_map_kalman beside cape_match_map_wide, room stream, {n} frames, {a.rounds} rounds of {a.reps} enqueues behind 3 warm-up calls"]
    for size in (64, 1024):
        planes, covs = list(base[:size]), list(base_cov[:size])
        while len(planes) < size:
            at = int(rng.integers(len(base)))
            nw, d, x, y, c, ring, h = base[at]
            planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
            covs.append(base_cov[at])
        arrays = cape_amd.pack_map(planes)
        tracks = np.zeros(size, cape_amd.MAP_TRACK_DTYPE)
        for j in range(size):
            tracks[j]["covariance"] = covs[j]
            tracks[j]["flags"] = cape_amd.MAP_TRACK_STAGED if j % 2 else 0
            tracks[j]["successive_matched"], tracks[j]["failed_tracking"] = j % 5, j % 3
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.match_map_wide(n, W2C, None, 0, st)
        kalman_ms, match_ms = [], []
        # (cape_match_map_wide invalidates cape_map_kalman's results, not its inputs: the two calls can take turns)
        for call in (lambda: ex.map_kalman(n, st), lambda: ex.match_map_wide(n, W2C, None, 0, st)):
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for out, call in ((kalman_ms, lambda: ex.map_kalman(n, st)), (match_ms, lambda: ex.match_map_wide(n, W2C, None, 0, st))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / a.reps)
        ex.map_kalman(n, st)
        frames, rows, results = ex.map_kalman_rows(n)
        _, match, _, _ = ex.map_matches_wide(n)
        lines.append(f"map of {size:4d} planes: cape_map_kalman {spread(kalman_ms)}; cape_match_map_wide {spread(match_ms)}; ratio of the medians "
                     f"(kalman / match) {statistics.median(kalman_ms) / statistics.median(match_ms):.3f}; {int((match >= 0).sum())} matched pairs, "
                     f"{int(frames['n_updated'].sum())} updated, {int(np.count_nonzero(frames['flags']))} frames flagged")
        calls = [host_kalman_call(cape_amd, arrays, tracks, match[f], mrows[f, kept[f][1]]) for f in range(n)]
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            out = list(pool.map(lambda run: run(), calls))
            host_ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"map of {size:4d} planes: host route, 16 threads over cape_host_map_kalman: {host_ms:9.1f} ms, "
                     f"{host_ms / statistics.median(kalman_ms):7.1f}x the device call; {sum(k for k, _ in out)} updated "
                     f"(device: {int(frames['n_updated'].sum())})")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
