"""cape_map_step_visible against the four calls it stands for -- cape_map_visibility(1, pose, moving), cape_copy_map_visibility (a wait of
its own), cape_map_step(words) with the caller keeping the moving words -- and against cape_map_step(skip = NULL), which prices the
visibility itself.  The batch is profiles/map_step_rate.py's (room stream, seed 11, frames 20, 25, .. 55).

1. Room frame 0 alone, on the room's own map.
2. The loop of eight frames on the same batch, no upload in between; a host clock around the eight frames, divided by eight.
3. One frame against a map of 1 024 planes: perturbed copies of the room's planes, every eighth with an outer ring of 512 vertices,
   every fourth moved off the screen, every seventh track MOVING -- where the shape of the classify kernel matters.
   Device time, from events around the calls on the same map: cape_map_visibility(1) (memset, cape_map_classify_kernel, the visible
   kernels), and cape_map_step_visible less cape_map_step(words) (memset, cape_map_classify_one_kernel, the visible kernels, the
   counters' copy): their difference is the two classify kernels' plus what the host adds between the launches.  --classify-only
   runs just these two calls on that map, for a kernel trace (rocprofv3 --kernel-trace --stats) that times the two kernels themselves.
Per repetition the map and tracks are uploaded again and the retired log is cleared, untimed; a host clock around the route; the routes
alternate repetition by repetition in one run; the figures are medians with their ranges.  The bytes the step and the four calls leave
(headers, map, tracks, log, words) are compared.

    python profiles/map_step_visible_rate.py [--reps 30] [--out profiles/map_step_visible_rate.txt]"""
import argparse
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from map_step_rate import measure, spread  # noqa: E402


def moving_words(ca, tracks):
    words = np.zeros((len(tracks) + 31) // 32, np.uint32)
    for j in np.flatnonzero(tracks["flags"] & ca.MAP_TRACK_MOVING):
        words[j >> 5] |= np.uint32(1 << (int(j) & 31))
    return words if len(words) and words.any() else None


def visible(ca, ex, st, f, T, flags, next_id, keep):
    result, next_id = ex.map_step_visible(f, T, ca.MATCH_ALLOW_INDEX0, flags, next_id, st)
    keep["words"] = None  # (read outside the clock: compared below)
    return result["step"]["commit"], result["step"]["maintain"], next_id


def four_calls(ca, ex, st, f, T, moving, flags, next_id, keep):
    ex.map_visibility(1, T[None], moving, st)
    words, _ = ex.map_visibility_words(1)
    result, next_id = ex.map_step(f, T, words[0] if words.shape[1] else None, ca.MATCH_ALLOW_INDEX0, flags, next_id, st)
    keep["words"] = words[0].copy()
    return result["commit"], result["maintain"], next_id


def no_words(ca, ex, st, f, T, flags, next_id):
    result, next_id = ex.map_step(f, T, None, ca.MATCH_ALLOW_INDEX0, flags, next_id, st)
    return result["commit"], result["maintain"], next_id


def large_map(ca, arrays, tracks, size, rng):
    """`size` perturbed copies of the planes of (arrays, tracks)"""
    P, R, V = arrays
    base = []
    for j in range(len(P)):
        r = R[P[j]["ring_first"]]
        base.append((P[j], V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]].copy()))
    planes, out = [], np.zeros(size, ca.MAP_TRACK_DTYPE)
    for j in range(size):
        at = int(rng.integers(len(base)))
        p, ring = base[at]
        ring = ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2)
        if j % 8 == 3:
            a = 0.1 + np.linspace(0, 2 * math.pi, 512, endpoint=False)
            ring = ring.mean(axis=0) + 0.5 * float(np.ptp(ring, axis=0).max()) * np.stack([np.cos(a), np.sin(a)], 1)
        if j % 4 == 1:
            ring = ring + np.array([60000.0, 0.0])
        planes.append((p["normal"], float(p["d"]) + float(rng.uniform(-120, 120)), p["x_axis"], p["y_axis"], p["center"], ring, []))
        out[j]["covariance"], out[j]["id"] = tracks[at]["covariance"], 5000 + j
        out[j]["flags"] = ca.MAP_TRACK_MOVING if j % 7 == 0 else 0
    return ca.pack_map(planes), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--classify-only", action="store_true",
                    help="only the 1 024-plane map, cape_map_visibility(1) and cape_map_step_visible alternating: for a kernel trace of the two classify kernels")
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
    add = ca.COMMIT_ADD_STAGED
    lines = [f"cape_map_step_visible against cape_map_visibility(1) + cape_copy_map_visibility + cape_map_step(words), and against cape_map_step(NULL): "
             f"room stream, frames {picks}, {a.reps} repetitions behind 3 warm-up repetitions, the routes alternating"]

    def one_frame(what, arrays, tracks, flags):
        keep, moving = {}, moving_words(ca, tracks)
        ms, left = measure(ca, ex, st, torch, arrays, tracks, a.reps, {
            "visible": lambda: visible(ca, ex, st, 0, W2C[0], flags, 1000, keep)[:2],
            "four": lambda: four_calls(ca, ex, st, 0, W2C[0], moving, flags, 1000, keep)[:2],
            "none": lambda: no_words(ca, ex, st, 0, W2C[0], flags, 1000)[:2]})
        assert left["visible"] == left["four"], what + ": the step and the four calls leave different bytes"
        # the words, once more outside the clock
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.clear_retired()
        visible(ca, ex, st, 0, W2C[0], flags, 1000, keep)
        words, n_map = ex.map_step_skip_words()
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        four_calls(ca, ex, st, 0, W2C[0], moving, flags, 1000, keep)
        assert np.array_equal(words, keep["words"]), what + ": the words differ"
        skipped = sum(bin(int(w)).count("1") for w in words)
        b, c, d = (statistics.median(ms[k]) for k in ("visible", "four", "none"))
        lines.append(f"{what}, a map of {n_map} planes of which {skipped} are skipped (headers, map, tracks, log and words equal byte for byte): "
                     f"cape_map_step_visible(0) {spread(ms['visible'])}; the four calls {spread(ms['four'])}; cape_map_step(0, NULL) {spread(ms['none'])}; "
                     f"four calls less the one call {(c - b) * 1e3:.1f} us, ratio {c / b:.2f}; the one call less the step without words {(b - d) * 1e3:.1f} us")

    if a.classify_only:
        big, big_tracks = large_map(ca, arrays, tracks, ca.MAP_MAX_PLANES, np.random.default_rng(5))
        moving = moving_words(ca, big_tracks)
        for rep in range(2 * a.reps):
            ex.upload_map(big)
            ex.upload_tracks(big_tracks)
            if rep % 2:
                ex.map_visibility(1, W2C[:1], moving, st)
            else:
                ex.map_step_visible(0, W2C[0], ca.MATCH_ALLOW_INDEX0, 0, 1000, st)
            torch.cuda.synchronize()
        ex.close()
        return

    # 1. one frame on the room's map
    one_frame("room frame 0 alone", arrays, tracks, add)

    # 2. the loop
    def loop(one):
        def run():
            next_id, last = 1000, None
            for f in range(n):
                *last, next_id = one(f, next_id)
            return last
        return run

    keep = {}
    ms, left = measure(ca, ex, st, torch, arrays, tracks, a.reps, {
        "visible": loop(lambda f, nid: visible(ca, ex, st, f, W2C[f], add, nid, keep)),
        "four": loop(lambda f, nid: four_calls(ca, ex, st, f, W2C[f], None, add, nid, keep)),
        "none": loop(lambda f, nid: no_words(ca, ex, st, f, W2C[f], add, nid))})
    assert left["visible"] == left["four"], "the two loops leave different bytes"
    per = {k: [v / n for v in ms[k]] for k in ms}
    b, c, d = (statistics.median(per[k]) for k in ("visible", "four", "none"))
    lines.append(f"the loop of eight frames (map, tracks and log equal byte for byte after it): period per frame by cape_map_step_visible(f) "
                 f"{spread(per['visible'])}; by the four calls {spread(per['four'])}; by cape_map_step(f, NULL) {spread(per['none'])}; four calls less the "
                 f"one call {(c - b) * 1e3:.1f} us, ratio {c / b:.2f}; the one call less the step without words {(b - d) * 1e3:.1f} us")

    # 3. the large map
    big, big_tracks = large_map(ca, arrays, tracks, ca.MAP_MAX_PLANES, np.random.default_rng(5))
    one_frame("one frame against 1 024 planes", big, big_tracks, 0)
    moving = moving_words(ca, big_tracks)
    ex.upload_map(big)
    ex.upload_tracks(big_tracks)
    ex.map_visibility(1, W2C[:1], moving, st)
    words = ex.map_visibility_words(1)[0][0].copy()
    dev_ms = {"batch": [], "visible": [], "words": []}
    for rep in range(3 * (a.reps + 3)):
        name = list(dev_ms)[rep % 3]
        ex.upload_map(big)
        ex.upload_tracks(big_tracks)
        ex.clear_retired()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if name == "batch":
            ex.map_visibility(1, W2C[:1], moving, st)
        elif name == "visible":
            ex.map_step_visible(0, W2C[0], ca.MATCH_ALLOW_INDEX0, 0, 1000, st)
        else:
            ex.map_step(0, W2C[0], words, ca.MATCH_ALLOW_INDEX0, 0, 1000, st)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 9:
            dev_ms[name].append(e0.elapsed_time(e1))
    b, v, w = (statistics.median(dev_ms[k]) for k in ("batch", "visible", "words"))
    lines.append(f"device time on the 1 024-plane map, events around the calls: cape_map_visibility(1) {spread(dev_ms['batch'])}; cape_map_step_visible "
                 f"{spread(dev_ms['visible'])}; cape_map_step(words) {spread(dev_ms['words'])}; the visibility inside the step {(v - w) * 1e3:.1f} us against "
                 f"{b * 1e3:.1f} us by the batch kernels: the one-frame classify kernel is {(b - (v - w)) * 1e3:.1f} us shorter than cape_map_classify_kernel "
                 f"with n_frames = 1")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
