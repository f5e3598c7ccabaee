"""cape_map_union_holes beside cape_map_union and the cape_match_map_wide that feeds them, in the shape of profiles/map_union_rate.py:
the 4 096-frame room batch against the map of 64 planes, twice.  The first pass runs against the map as it was built (no plane has a
hole).  Then the served polygons of the holes call are applied to the map on the host -- frame 0's, and for a map plane that frame 0
gives no interior ring the first frame of the batch whose served polygon for it has one -- the map is uploaded again and the second
pass runs against it, so that map planes with holes really occur.  Per pass: the share of pairs per flag for both calls, the medians
of both calls beside the match (device events after warm-up, the three calls alternating round by round, cape_map_kalman untimed in
between), and the same pairs through 16 threads of the twin cape_host_map_union_holes.

    python profiles/map_union_holes_rate.py [--frames 4096] [--out profiles/map_union_holes_rate.txt]"""
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

NAMES = ("SERVED", "UNCHANGED", "DISJOINT", "HOST_MAP_HOLES", "HOST_NEW_HOLE", "HOST_CAPACITY", "HOST_AMBIGUOUS", "HOLES", "HOST_HOLE_CUT")


def host_holes_call(ca, arrays, match, fusion, rows_in, rings):
    """cape_host_map_union_holes, prepared: returns run() -> (served pairs, the arrays it keeps alive)"""
    L = ca._host_library()
    src, src_view = ca._map_arrays(arrays)
    match = np.ascontiguousarray(match, np.int32)
    fusion = np.ascontiguousarray(fusion, ca.PLANE_FUSION_DTYPE)
    rows_in = np.ascontiguousarray(rows_in, ca.PLANE_MEASUREMENT_DTYPE)
    world = np.ascontiguousarray(np.concatenate(list(rings) + [np.zeros((1, 2))]))
    rows = np.zeros(ca.MATCH_MAP_WIDE_MAX_PLANES, ca.PLANE_UNION_DTYPE)
    ring_rows = np.zeros(ca.MATCH_MAP_WIDE_MAX_PLANES, ca.PLANE_UNION_RINGS_DTYPE)
    slab = np.zeros((ca.MAP_UNION_FRAME_VERTICES, 2))

    def run():
        rc = L.cape_host_map_union_holes(C.byref(src_view), ca._as(match, C.c_int32), fusion.ctypes.data, rows_in.ctypes.data, world.ctypes.data,
                                         len(rows_in), rows.ctypes.data, ring_rows.ctypes.data, slab.ctypes.data)
        if rc != 0:
            raise ca.CapeError(f"cape_host_map_union_holes failed ({rc})")
        return int(np.count_nonzero(rows["flags"] & ca.UNION_SERVED)), (src, match, fusion, rows_in, world, rows, ring_rows, slab)

    return run


def shares(rows):
    pairs = rows[rows["map_plane"] >= 0]
    pairs = pairs[pairs["flags"] != 0]
    return len(pairs), ", ".join(f"{nm} {100.0 * np.count_nonzero(pairs['flags'] & (1 << k)) / max(len(pairs), 1):.2f} %" for k, nm in enumerate(NAMES)
                                 if np.count_nonzero(pairs["flags"] & (1 << k)))


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
    n, size = a.frames, 64
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
    # the 64-plane map of map_union_rate.py
    src = [(f, k, s) for f in range(0, n, max(1, n // 16)) for k, s in zip(*kept[f])]
    base = [lift(k, *c2w[f]) for f, k, _ in src]
    base_cov = [mrows[f, s]["covariance"].copy() for f, _, s in src]
    planes, covs = list(base[:size]), list(base_cov[:size])
    while len(planes) < size:
        at = int(rng.integers(len(base)))
        nw, d, x, y, c, ring, h = base[at]
        planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        covs.append(base_cov[at])
    tracks = np.zeros(size, cape_amd.MAP_TRACK_DTYPE)
    for j in range(size):
        tracks[j]["covariance"] = covs[j]
        tracks[j]["flags"] = cape_amd.MAP_TRACK_STAGED if j % 2 else 0
        tracks[j]["successive_matched"], tracks[j]["failed_tracking"] = j % 5, j % 3
    lines = [f"cape_map_union_holes beside cape_map_union and cape_match_map_wide, room stream, {n} frames, map of {size} planes, {a.rounds} rounds "
             f"of {a.reps} enqueues behind 3 warm-up calls"]
    for which in ("first pass, the map as built", "second pass, the first pass's polygons applied"):
        arrays = cape_amd.pack_map(planes)
        holed = sum(1 for p in planes if len(p[6]))
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.match_map_wide(n, W2C, None, 0, st)
        plain_ms, holes_ms, match_ms = [], [], []
        ex.map_kalman(n, st)
        for _ in range(3):
            ex.map_union(n, st)
            ex.map_union_holes(n, st)
        for _ in range(3):
            ex.match_map_wide(n, W2C, None, 0, st)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            ex.map_kalman(n, st)  # (untimed: the match of the round before invalidated its results)
            for out, call in ((plain_ms, lambda: ex.map_union(n, st)), (holes_ms, lambda: ex.map_union_holes(n, st)),
                              (match_ms, lambda: ex.match_map_wide(n, W2C, None, 0, st))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) / a.reps)
        ex.map_kalman(n, st)
        _, fusion, _ = ex.map_kalman_rows(n)
        _, match, _, _ = ex.map_matches_wide(n)
        ex.map_union(n, st)
        n_plain, plain_share = shares(ex.map_union_rows(n)[0])
        ex.map_union_holes(n, st)
        out = ex.map_union_polygons(n)
        hrows = np.stack([o[0] for o in out])
        n_holes, holes_share = shares(hrows)
        lines.append(f"{which}: {holed} of {size} map planes have interior rings")
        lines.append(f"  cape_map_union       {spread(plain_ms)}; {n_plain} pairs: {plain_share}")
        lines.append(f"  cape_map_union_holes {spread(holes_ms)}; {n_holes} pairs: {holes_share}; holes new / kept / covered "
                     f"{sum(int(o[1]['holes_new'].sum()) for o in out)} / {sum(int(o[1]['holes_kept'].sum()) for o in out)} / "
                     f"{sum(int(o[1]['holes_covered'].sum()) for o in out)}")
        lines.append(f"  cape_match_map_wide  {spread(match_ms)}; ratio of the medians (holes call / match) "
                     f"{statistics.median(holes_ms) / statistics.median(match_ms):.3f}, (holes call / plain call) "
                     f"{statistics.median(holes_ms) / statistics.median(plain_ms):.3f}")
        calls = []
        for f in range(n):
            rows_f = mrows[f, kept[f][1]]
            rings = [mver[f, r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]] for r in rows_f]
            calls.append(host_holes_call(cape_amd, arrays, match[f], fusion[f, :len(rows_f)], rows_f, rings))
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            res = list(pool.map(lambda run: run(), calls))
            host_ms = (time.perf_counter() - t0) * 1e3
        lines.append(f"  host route, 16 threads over cape_host_map_union_holes: {host_ms:9.1f} ms, {host_ms / statistics.median(holes_ms):7.1f}x the "
                     f"holes call; {sum(k for k, _ in res)} served (device: {int(np.count_nonzero(hrows['flags'] & 1))})")
        # the next pass's map: frame 0's served polygons, else the first holed one of the batch
        chosen = {}
        for f in range(n):
            rows, _, polys = out[f]
            for i in np.flatnonzero((rows["flags"] & cape_amd.UNION_SERVED) != 0):
                j = int(rows[i]["map_plane"])
                if (f == 0 and j not in chosen) or (len(polys[i]) > 1 and (j not in chosen or len(chosen[j][1]) == 1)):
                    chosen[j] = (rows[i], polys[i], fusion[f, i])
        for j, (row, poly, fu) in chosen.items():
            planes[j] = (fu["normal"].copy(), float(fu["d"]), row["x_axis"].copy(), row["y_axis"].copy(), row["center"].copy(), poly[0], list(poly[1:]))
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
