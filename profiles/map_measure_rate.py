"""cape_map_measure beside cape_match_map_wide (device events after warm-up, the two calls alternating round by round in one run) on the
4 096-frame room batch with the poses of its trajectory, a pose covariance of a few mm^2 per frame and a 64-plane map for the matcher;
and the same planes through the host route: 16 threads over cape_host_map_update(CAPE_MAP_ADD_STAGED) on an empty map, one call per
frame (the C call only: the arrays are packed beforehand).

    python profiles/map_measure_rate.py [--frames 4096] [--out profiles/r12_map_measure.txt]"""
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


def host_update_call(ca, det, T, S):
    """cape_host_map_update on an empty map with CAPE_MAP_ADD_STAGED, prepared: returns run() -> planes appended"""
    L = ca._host_library()
    src, src_view = ca._map_arrays(ca.pack_map([]), np.zeros(0, ca.MAP_TRACK_DTYPE))
    cols, det_view = ca._pack_detected(det, with_cov=True)
    n, nv = max(len(det), 1), max(len(cols["vertices"]), 1)
    out = dict(planes=np.zeros(n, ca.MAP_PLANE_DTYPE), rings=np.zeros(n, ca.MAP_RING_DTYPE), vertices=np.zeros((nv, 2)),
               tracks=np.zeros(n, ca.MAP_TRACK_DTYPE))
    view = ca._view(ca.cape_host_map, out, planes_capacity=n, rings_capacity=n, vertices_capacity=nv)
    T, S = np.ascontiguousarray(T, np.float64).reshape(16), np.ascontiguousarray(S, np.float64).reshape(9)
    match, used, nid = np.zeros(1, np.int32), np.zeros(n, np.int32), C.c_uint64(0)

    def run():
        rc = L.cape_host_map_update(C.byref(src_view), ca._as(match, C.c_int32), C.byref(det_view), ca._as(T, C.c_double), ca._as(S, C.c_double),
                                    ca.MAP_ADD_STAGED, C.byref(nid), C.byref(view), ca._as(used, C.c_int32))
        if rc != 0:
            raise ca.CapeError(f"cape_host_map_update failed ({rc})")
        return int(view.n_planes), (src, cols, out)  # (the arrays stay alive with the closure)

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

    def alternate(calls):
        """per call: the mean ms of --reps enqueues, --rounds times, the calls taking turns (3 warm-up enqueues each first)"""
        for call in calls:
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        out = [[] for _ in calls]
        for _ in range(a.rounds):
            for k, call in enumerate(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                out[k].append(e0.elapsed_time(e1) / a.reps)
        return out

    n = a.frames
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    c2w = synth_gpu._poses("room", 1, 0, n)
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    res = ex.results(n, with_boundary=False)
    kept = ex.kept_planes(n)
    rng = np.random.default_rng(0)
    T, W2C, S = np.zeros((n, 4, 4)), np.zeros((n, 4, 4)), np.zeros((n, 3, 3))
    for f in range(n):
        R, o = c2w[f]
        T[f, :3, :3], T[f, :3, 3], T[f, 3, 3] = R, o, 1.0
        W2C[f, :3, :3], W2C[f, :3, 3], W2C[f, 3, 3] = R.T, -R.T @ o, 1.0
        A = rng.normal(size=(3, 3))
        S[f] = A @ A.T + 3 * np.eye(3)
    base = [lift(k, *c2w[f]) for f in range(0, n, max(1, n // 16)) for k in kept[f][0]]
    ex.upload_map(cape_amd.pack_map(base[:64]))
    measure_ms, match_ms = alternate([lambda: ex.map_measure(n, T, S, st), lambda: ex.match_map_wide(n, W2C, None, 0, st)])
    rows, _ = ex.measurement_rows(n)
    n_kept = int(np.count_nonzero(rows["flags"] & cape_amd.MEASURE_KEPT))
    n_stageable = int(np.count_nonzero(rows["flags"] & cape_amd.MEASURE_STAGEABLE))
    lines = [f"cape_map_measure beside cape_match_map_wide (64-plane map), room stream, {n} frames, {a.rounds} rounds of {a.reps} enqueues behind "
             f"3 warm-up calls",
             f"cape_map_measure    {spread(measure_ms)}: {n_kept} kept planes, {n_stageable} stageable",
             f"cape_match_map_wide {spread(match_ms)}; ratio of the medians (measure / match) {statistics.median(measure_ms) / statistics.median(match_ms):.3f}"]
    calls = []
    for f in range(n):
        det, segs = kept[f]
        seg = res.segments(f)
        calls.append(host_update_call(cape_amd, [d + (seg[s]["cov"].reshape(3, 3).copy(),) for d, s in zip(det, segs)], T[f], S[f]))
    with ThreadPoolExecutor(16) as pool:
        t0 = time.perf_counter()
        out = list(pool.map(lambda run: run(), calls))
        host_ms = (time.perf_counter() - t0) * 1e3
    appended = sum(k for k, _ in out)
    lines.append(f"host route, 16 threads over cape_host_map_update(CAPE_MAP_ADD_STAGED) on an empty map: {host_ms:9.1f} ms, "
                 f"{host_ms / statistics.median(measure_ms):7.1f}x the device call; {appended} planes appended (device: {n_stageable} stageable)")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
