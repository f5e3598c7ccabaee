"""cape_match_polygons_wide next to what it widens and what it replaces.

1. The 4 096-frame room batch, where every frame fits both paths: cape_match_polygons_wide against cape_match_polygons of the same
   build, the two calls alternating over --rounds rounds of --reps calls, device events, after a warm-up of both.  The ratio is the
   price of the wider tables.
2. A --host-frames batch of the 640 x 480 checkerboard of facets (more than 16 kept planes per frame: the frames cape_match_polygons
   flags): the wide call against the route those frames took before, 16 threads over cape_host_match_planes (Python wrappers
   included: that is the route as a caller of the binding takes it; the kept planes are fetched once, outside the clock).

    python profiles/wide_match_rate.py [--frames 4096] [--host-frames 64] [--rounds 5] [--reps 10] [--out FILE]
    python profiles/wide_match_rate.py --narrow-only [--tree OTHER_CHECKOUT] [--label NAME]

--narrow-only times cape_match_polygons alone; with --tree, that of another checkout's package and library on the same workload (the
A/B against the parent commit: alternate the two processes)."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(ms):
    return f"median {statistics.median(ms):8.3f} ms (min {min(ms):8.3f}, max {max(ms):8.3f} over {len(ms)} rounds)"


def checkerboard(width=640, height=480, tile=80, seed=3):
    """tilted facets in a checkerboard, a depth step between neighbours: every facet is a plane of its own (48 at 640 x 480)"""
    from cape_amd import synth

    intr = dict(synth.DEFAULT_INTRINSICS)
    X, Y = np.meshgrid((np.arange(width) - intr["cx"]) / intr["fx"], (np.arange(height) - intr["cy"]) / intr["fy"])
    tilts = [(0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (0.0, -0.5)]
    z = np.zeros((height, width))
    for ty in range(0, height, tile):
        for tx in range(0, width, tile):
            nx, ny = tilts[((tx // tile) % 2) + 2 * ((ty // tile) % 2)]
            d = 2000.0 + 120.0 * (((tx // tile) * 7 + (ty // tile) * 13) % 9)
            sl = (slice(ty, min(ty + tile, height)), slice(tx, min(tx + tile, width)))
            z[sl] = d / (1.0 + nx * X[sl] + ny * Y[sl])
    return z, intr, np.random.default_rng(seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host-frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--narrow-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "rgb-d-slam_amd", "python"))
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    st = torch.cuda.current_stream().cuda_stream

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def alternate(calls):
        for _ in range(3):
            for call in calls:
                call()
        torch.cuda.synchronize()
        ms = [[] for _ in calls]
        for _ in range(a.rounds):
            for k, call in enumerate(calls):
                ms[k].append(timed(call))
        return ms

    n = a.frames
    lines = [f"{a.label or 'wide_match_rate'}: {a.rounds} rounds of {a.reps} calls, device events, the calls of a pair alternating round by round"]
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)

    def narrow():
        ex.match_polygons(n, 0, st)

    def wide():
        ex.match_polygons_wide(n, None, 0, st)

    if a.narrow_only:
        (narrow_ms,) = alternate([narrow])
    else:
        narrow_ms, wide_ms = alternate([narrow, wide])
    got = ex.polygon_matches(n)
    lines.append(f"room stream, {n} frames: cape_match_polygons      {spread(narrow_ms)}, {int((got['match'] >= 0).sum())} matches, "
                 f"{int(np.count_nonzero(got['flags']))} frames flagged")
    if not a.narrow_only:
        frames, match, _, _ = ex.polygon_matches_wide(n)
        same = bool(np.array_equal(match[:, :cape_amd.MATCH_MAX_PLANES], got["match"]) and np.all(match[:, cape_amd.MATCH_MAX_PLANES:] == -1))
        lines.append(f"room stream, {n} frames: cape_match_polygons_wide {spread(wide_ms)}, {int(np.count_nonzero(frames['flags']))} frames flagged, "
                     f"matches equal to cape_match_polygons: {same}; ratio of the medians "
                     f"{statistics.median(wide_ms) / statistics.median(narrow_ms):.3f}")
    ex.close()
    del dev

    hn = 0 if a.narrow_only else a.host_frames
    if hn:
        z, intr, rng = checkerboard()
        batch = np.stack([np.round(z + rng.normal(0, 0.6, z.shape)).astype(np.float32) for _ in range(hn)])  # (the noise differs frame by frame)
        dev = torch.from_numpy(batch).cuda()
        ex = Extractor(640, 480, cylinders=False, max_batch=hn, **intr)
        ex.extract_device(dev.data_ptr(), hn, st)
        ex.build_polygons(hn, st)

        def wide_checker():
            ex.match_polygons_wide(hn, None, 0, st)

        (checker_ms,) = alternate([wide_checker])
        frames, match, _, _ = ex.polygon_matches_wide(hn)
        ex.match_polygons(hn, 0, st)
        narrow_flagged = int(np.count_nonzero(ex.polygon_matches(hn)["flags"]))
        kept = ex.kept_planes(hn)

        def host_route(f):
            return cape_amd.host_match_planes(kept[f - 1][0], kept[f][0], None, 0)

        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            out = list(pool.map(host_route, range(1, hn)))
            host_ms = (time.perf_counter() - t0) * 1e3
        agree = sum(1 for f in range(1, hn) if not frames[f]["flags"] and list(out[f - 1]) == list(match[f, : len(out[f - 1])]))
        lines.append(f"checkerboard, {hn} frames of {int(frames['n_cur'].min())}..{int(frames['n_cur'].max())} kept planes (cape_match_polygons flags "
                     f"{narrow_flagged}): cape_match_polygons_wide {spread(checker_ms)}, {int(np.count_nonzero(frames['flags']))} frames flagged, "
                     f"{int(frames['n_matched'].sum())} matches")
        lines.append(f"checkerboard, {hn} frames: host route, 16 threads over host_match_planes {host_ms:9.1f} ms, "
                     f"{host_ms / statistics.median(checker_ms):7.1f}x the wide call; decisions equal on {agree} of {hn - 1} frame pairs")
        ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
