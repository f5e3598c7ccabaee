"""cape_map_union beside the cape_match_map_wide that feeds it (device events after warm-up, the two calls alternating round by round in
one run; the cape_map_kalman a union needs after every match runs untimed in between) on the 4 096-frame room batch with the poses of
its trajectory, a pose covariance of a few mm^2 per frame and maps of 64 and 1 024 planes (the maps of profiles/map_kalman_rate.py);
the share of pairs per flag and the largest n_nodes; and the same frames through the host twin: 16 threads over cape_host_map_union,
one call per frame, fed with the device's match, fusion and measurement rows and world rings (the C call only: the arrays are packed
beforehand).  The figure to beat is the host route's time for the same pairs.

    python profiles/map_union_rate.py [--frames 4096] [--out profiles/map_union_rate.txt]"""
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


def host_union_call(ca, arrays, match, fusion, rows_in, rings):
    """cape_host_map_union, prepared: returns run() -> (served pairs, the arrays it keeps alive)"""
    L = ca._host_library()
    src, src_view = ca._map_arrays(arrays)
    match = np.ascontiguousarray(match, np.int32)
    fusion = np.ascontiguousarray(fusion, ca.PLANE_FUSION_DTYPE)
    rows_in = np.ascontiguousarray(rows_in, ca.PLANE_MEASUREMENT_DTYPE)
    world = np.ascontiguousarray(np.concatenate(list(rings) + [np.zeros((1, 2))]))
    rows = np.zeros(ca.MATCH_MAP_WIDE_MAX_PLANES, ca.PLANE_UNION_DTYPE)
    slab = np.zeros((ca.MAP_UNION_FRAME_VERTICES, 2))

    def run():
        rc = L.cape_host_map_union(C.byref(src_view), ca._as(match, C.c_int32), fusion.ctypes.data, rows_in.ctypes.data, world.ctypes.data,
                                   len(rows_in), rows.ctypes.data, slab.ctypes.data)
        if rc != 0:
            raise ca.CapeError(f"cape_host_map_union failed ({rc})")
        return int(np.count_nonzero(rows["flags"] & ca.UNION_SERVED)), (src, match, fusion, rows_in, world, rows, slab)

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
    mrows, mver = ex.measurement_rows(n)
    # the maps of map_match_wide_rate.py; each plane's track holds the covariance of the measurement it came from
    src = [(f, k, s) for f in range(0, n, max(1, n // 16)) for k, s in zip(*kept[f])]
    base = [lift(k, *c2w[f]) for f, k, _ in src]
    base_cov = [mrows[f, s]["covariance"].copy() for f, _, s in src]
    lines = [f"cape_map_union beside cape_match_map_wide, room stream, {n} frames, {a.rounds} rounds of {a.reps} enqueues behind 3 warm-up calls"]
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
        union_ms, match_ms = [], []
        ex.map_kalman(n, st)
        for _ in range(3):
            ex.map_union(n, st)
        for _ in range(3):
            ex.match_map_wide(n, W2C, None, 0, st)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            ex.map_kalman(n, st)  # (untimed: the match of the round before invalidated its results)
            for out, call in ((union_ms, lambda: ex.map_union(n, st)), (match_ms, lambda: ex.match_map_wide(n, W2C, None, 0, st))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / a.reps)
        ex.map_kalman(n, st)
        ex.map_union(n, st)
        _, fusion, _ = ex.map_kalman_rows(n)
        _, match, _, _ = ex.map_matches_wide(n)
        urows, _ = ex.map_union_rows(n)
        pairs = urows[urows["map_plane"] >= 0]
        pairs = pairs[(pairs["flags"] != 0)]
        names = ("SERVED", "UNCHANGED", "DISJOINT", "HOST_MAP_HOLES", "HOST_NEW_HOLE", "HOST_CAPACITY", "HOST_AMBIGUOUS")
        share = ", ".join(f"{nm} {100.0 * np.count_nonzero(pairs['flags'] & (1 << k)) / max(len(pairs), 1):.2f} %" for k, nm in enumerate(names))
        lines.append(f"map of {size:4d} planes: cape_map_union {spread(union_ms)}; cape_match_map_wide {spread(match_ms)}; ratio of the medians "
                     f"(union / match) {statistics.median(union_ms) / statistics.median(match_ms):.3f}; {len(pairs)} pairs: {share}; largest "
                     f"n_nodes {int(pairs['n_nodes'].max()) if len(pairs) else 0}, mean result ring "
                     f"{float(pairs['vertex_count'][pairs['vertex_count'] > 0].mean()) if len(pairs) else 0:.1f} vertices")
        calls = []
        for f in range(n):
            rows_f = mrows[f, kept[f][1]]
            rings = [mver[f, r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]] for r in rows_f]
            calls.append(host_union_call(cape_amd, arrays, match[f], fusion[f, :len(rows_f)], rows_f, rings))
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            out = list(pool.map(lambda run: run(), calls))
            host_ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"map of {size:4d} planes: host route, 16 threads over cape_host_map_union: {host_ms:9.1f} ms, "
                     f"{host_ms / statistics.median(union_ms):7.1f}x the device call; {sum(k for k, _ in out)} served "
                     f"(device: {int(np.count_nonzero(pairs['flags'] & 1))})")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
