"""cape_map_union_cut beside cape_map_union_holes and the cape_match_map_wide that feeds them, in the shape of
profiles/map_union_holes_rate.py: the 4 096-frame room batch against the map of 64 planes.  The first pass only builds the second
pass's map -- the served polygons of the holes call applied on the host, by that script's rule, so that map planes with holes really
occur -- and is not timed.  The second pass: the share of pairs per flag for both calls, the pieces per cut hole, the medians of both
calls beside the match (device events after warm-up, the three calls alternating round by round, cape_map_kalman untimed in
between), and the host route for exactly the pairs cape_map_union_holes hands away as HOST_HOLE_CUT: 16 threads of
cape_host_map_union_cut over the frames that have such a pair, every other pair of those frames masked out of the fusion rows.  The two
comparisons the call has to win: its served share against the holes call's, and its time against the holes call plus that host
route.

    python profiles/map_union_cut_rate.py [--frames 4096] [--out profiles/map_union_cut_rate.txt]"""
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

NAMES = ("SERVED", "UNCHANGED", "DISJOINT", "HOST_MAP_HOLES", "HOST_NEW_HOLE", "HOST_CAPACITY", "HOST_AMBIGUOUS", "HOLES", "HOST_HOLE_CUT",
         "HOLE_PIECES")


def host_cut_call(ca, arrays, match, fusion, rows_in, rings):
    """cape_host_map_union_cut, prepared: returns run() -> (served pairs, the arrays it keeps alive)"""
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
        rc = L.cape_host_map_union_cut(C.byref(src_view), ca._as(match, C.c_int32), fusion.ctypes.data, rows_in.ctypes.data, world.ctypes.data,
                                       len(rows_in), rows.ctypes.data, ring_rows.ctypes.data, slab.ctypes.data)
        if rc != 0:
            raise ca.CapeError(f"cape_host_map_union_cut failed ({rc})")
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
    # ---- the first pass, untimed: the holes call's served polygons become the second pass's map (map_union_holes_rate.py's rule)
    ex.upload_map(cape_amd.pack_map(planes))
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, 0, st)
    ex.map_kalman(n, st)
    _, fusion, _ = ex.map_kalman_rows(n)
    ex.map_union_holes(n, st)
    out = ex.map_union_polygons(n)
    chosen = {}
    for f in range(n):
        rows, _, polys = out[f]
        for i in np.flatnonzero((rows["flags"] & cape_amd.UNION_SERVED) != 0):
            j = int(rows[i]["map_plane"])
            if (f == 0 and j not in chosen) or (len(polys[i]) > 1 and (j not in chosen or len(chosen[j][1]) == 1)):
                chosen[j] = (rows[i], polys[i], fusion[f, i])
    for j, (row, poly, fu) in chosen.items():
        planes[j] = (fu["normal"].copy(), float(fu["d"]), row["x_axis"].copy(), row["y_axis"].copy(), row["center"].copy(), poly[0], list(poly[1:]))
    # ---- the second pass
    arrays = cape_amd.pack_map(planes)
    holed = sum(1 for p in planes if len(p[6]))
    map_holes = [len(p[6]) for p in planes]
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, 0, st)
    holes_ms, cut_ms, match_ms = [], [], []
    ex.map_kalman(n, st)
    for _ in range(3):
        ex.map_union_holes(n, st)
        ex.map_union_cut(n, st)
    for _ in range(3):
        ex.match_map_wide(n, W2C, None, 0, st)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        ex.map_kalman(n, st)  # (untimed: the match of the round before invalidated its results)
        for ms, call in ((holes_ms, lambda: ex.map_union_holes(n, st)), (cut_ms, lambda: ex.map_union_cut(n, st)),
                         (match_ms, lambda: ex.match_map_wide(n, W2C, None, 0, st))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
    ex.map_kalman(n, st)
    _, fusion, _ = ex.map_kalman_rows(n)
    _, match, _, _ = ex.map_matches_wide(n)
    ex.map_union_holes(n, st)
    hout = ex.map_union_polygons(n)
    hrows = np.stack([o[0] for o in hout])
    n_holes, holes_share = shares(hrows)
    ex.map_union_cut(n, st)
    cout = ex.map_union_polygons(n)
    crows = np.stack([o[0] for o in cout])
    crings = np.stack([o[1] for o in cout])
    n_cut, cut_share = shares(crows)
    was_cut = (hrows["flags"] == cape_amd.UNION_HOST_HOLE_CUT)
    # (a pair served now that was handed away before moves every polygon behind it in its frame's slab: the rows are compared without
    #  their place in it, the polygons vertex for vertex)
    ha, cb = hrows.copy(), crows.copy()
    ha["vertex_offset"] = cb["vertex_offset"] = 0
    same = bool(np.all((ha.view(np.uint8).reshape(ha.shape + (-1,)) == cb.view(np.uint8).reshape(cb.shape + (-1,))).all(axis=-1)[~was_cut]))
    same = same and all(hout[f][1][i].tobytes() == cout[f][1][i].tobytes() and (hout[f][2][i] is None) == (cout[f][2][i] is None) and
                        (hout[f][2][i] is None or all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(hout[f][2][i], cout[f][2][i])))
                        for f, i in zip(*np.nonzero(~was_cut & (hrows["map_plane"] >= 0) & (hrows["flags"] != 0))))
    # pieces per cut hole: a served pair's interior rings are its new holes, its kept holes and the pieces; its cut holes are the map
    # plane's holes that were neither kept nor covered
    with_pieces = (crows["flags"] & cape_amd.UNION_HOLE_PIECES) != 0
    pieces = cut_holes = 0
    for f, i in zip(*np.nonzero(with_pieces)):
        q = crings[f, i]
        pieces += int(q["ring_count"]) - 1 - int(q["holes_new"]) - int(q["holes_kept"])
        cut_holes += map_holes[int(crows[f, i]["map_plane"])] - int(q["holes_kept"]) - int(q["holes_covered"])
    lines = [f"cape_map_union_cut beside cape_map_union_holes and cape_match_map_wide, room stream, {n} frames, map of {size} planes of which {holed} "
             f"have interior rings (the holes call's polygons of a first pass applied), {a.rounds} rounds of {a.reps} enqueues behind 3 warm-up calls",
             f"  cape_match_map_wide  {spread(match_ms)}",
             f"  cape_map_union_holes {spread(holes_ms)}; {n_holes} pairs: {holes_share}",
             f"  cape_map_union_cut   {spread(cut_ms)}; {n_cut} pairs: {cut_share}",
             f"  ratio of the medians (cut call / holes call) {statistics.median(cut_ms) / statistics.median(holes_ms):.3f}, (cut call / match) "
             f"{statistics.median(cut_ms) / statistics.median(match_ms):.3f}",
             f"  of the {int(was_cut.sum())} pairs the holes call hands away as HOST_HOLE_CUT the cut call serves {int((with_pieces & was_cut).sum())} with "
             f"HOLE_PIECES and hands away {int((was_cut & ~with_pieces).sum())} "
             f"(flags {sorted({hex(int(v)) for v in crows['flags'][was_cut & ~with_pieces]})}); every other row, rings row and polygon is the same in both calls (up to its place in the slab): {same}",
             f"  {pieces} pieces of {cut_holes} cut holes in {int(with_pieces.sum())} pairs: {pieces / max(cut_holes, 1):.3f} pieces per cut hole; n_nodes of a "
             f"row is its first arrangement's (largest {int(crows['n_nodes'][with_pieces].max()) if with_pieces.any() else 0} among these pairs): the "
             f"second arrangements' node counts are not reported by the device and were not measured here"]
    # the host route for the pairs the holes call hands away: cape_host_map_union_cut over those pairs alone
    calls = []
    for f in np.flatnonzero(was_cut.any(axis=1)):
        rows_f = mrows[f, kept[f][1]]
        rings = [mver[f, r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]] for r in rows_f]
        fu = fusion[f, :len(rows_f)].copy()
        fu["map_plane"][~was_cut[f, :len(rows_f)]] = -1
        calls.append(host_cut_call(cape_amd, arrays, match[f], fu, rows_f, rings))
    with ThreadPoolExecutor(16) as pool:
        t0 = time.perf_counter()
        res = list(pool.map(lambda run: run(), calls))
        host_ms = (time.perf_counter() - t0) * 1e3
    both = statistics.median(holes_ms) + host_ms
    lines.append(f"  host route, 16 threads over cape_host_map_union_cut for those {int(was_cut.sum())} pairs in {len(calls)} frames: {host_ms:9.1f} ms, "
                 f"{sum(k for k, _ in res)} served; holes call + host route {both:9.1f} ms against the cut call's {statistics.median(cut_ms):9.3f} ms: "
                 f"{both / statistics.median(cut_ms):7.1f}x")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
