"""cape_match_map_wide beside cape_match_map (device events after warm-up, the two calls alternating round by round in one run):

1. The 4 096-frame room batch with its true poses against a 64-plane and a 1 024-plane map (the maps of profiles/map_match_rate.py).
   Both calls serve every frame of that batch; the wide one differs by a doubled gate and select width.
2. A --host-frames batch of the 1280 x 960 checkerboard of facets (frames that continue in a spill record, which cape_match_map
   flags) against a map of the first frame's own kept planes: cape_match_map_wide against the host route, 16 threads over
   cape_host_match_map on the kept planes of the chains.

    python profiles/map_match_wide_rate.py [--frames 4096] [--host-frames 64] [--out profiles/r11_map_match_wide.txt]"""
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


def spread(ms):
    return f"median {statistics.median(ms):8.3f} ms (min {min(ms):8.3f}, max {max(ms):8.3f} over {len(ms)} rounds)"


def unit(v):
    return v / np.linalg.norm(v)


def lift(det, R, o):
    nn, d, x, y, c, ring, _ = det
    nw, cw = unit(R @ nn), o + R @ c
    return (nw, float(-(nw @ cw)), unit(R @ x), unit(R @ y), cw, ring, [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host-frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu
    from wide_match_rate import checkerboard

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
    kept = ex.kept_planes(n)
    base = [lift(k, *c2w[f]) for f in range(0, n, max(1, n // 16)) for k in kept[f][0]]
    rng = np.random.default_rng(0)
    T = np.zeros((n, 4, 4))
    for f in range(n):
        R, o = c2w[f]
        T[f, :3, :3], T[f, :3, 3], T[f, 3, 3] = R.T, -R.T @ o, 1.0
    lines = [f"cape_match_map_wide beside cape_match_map, room stream, {n} frames, {a.rounds} rounds of {a.reps} enqueues behind 3 warm-up calls"]
    for size in (64, 1024):
        planes = list(base[:size])
        while len(planes) < size:
            nw, d, x, y, c, ring, h = base[int(rng.integers(len(base)))]
            planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        ex.upload_map(cape_amd.pack_map(planes))
        narrow_ms, wide_ms = alternate([lambda: ex.match_map(n, T, None, 0, st), lambda: ex.match_map_wide(n, T, None, 0, st)])
        nf, nm = ex.map_matches(n)
        wf, wm, _, _ = ex.map_matches_wide(n)
        same = bool(np.array_equal(nm, wm) and np.array_equal(nf["flags"], wf["flags"]))
        lines.append(f"map of {size:4d} planes: cape_match_map {spread(narrow_ms)}; cape_match_map_wide {spread(wide_ms)}; ratio of the medians "
                     f"{statistics.median(wide_ms) / statistics.median(narrow_ms):.3f}; {int(np.count_nonzero(wf['flags']))} frames flagged, "
                     f"{int(wf['n_matched'].sum())} matches, decisions equal to cape_match_map: {same}")
    ex.close()
    del dev

    hn = a.host_frames
    if hn:
        Wd, Ht = 1280, 960
        z, intr, rng = checkerboard(Wd, Ht, 100)
        batch = np.stack([np.round(z + rng.normal(0, 0.6, z.shape)).astype(np.float32) for _ in range(hn)])  # (the noise differs frame by frame)
        dev = torch.from_numpy(batch).cuda()
        ex = Extractor(Wd, Ht, cylinders=False, max_batch=hn, **intr)
        ex.extract_device(dev.data_ptr(), hn, st)
        ex.build_polygons(hn, st)
        kept = ex.kept_planes(hn)
        eye = (np.eye(3), np.zeros(3))
        planes = [lift(k, *eye) for k in kept[0][0]]
        arrays = cape_amd.pack_map(planes)
        ex.upload_map(arrays)
        (checker_ms,) = alternate([lambda: ex.match_map_wide(hn, None, None, 0, st)])
        frames, match, _, _ = ex.map_matches_wide(hn)
        ex.match_map(hn, None, None, 0, st)
        narrow_flagged = int(np.count_nonzero(ex.map_matches(hn)[0]["flags"]))
        calls = [cape_amd.host_match_map_call(arrays, kept[f][0], None, None, 0) for f in range(hn)]
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            out = list(pool.map(lambda run: run(), calls))
            host_ms = (time.perf_counter() - t0) * 1e3
        agree = sum(1 for f in range(hn) if not frames[f]["flags"] and list(out[f][0]) == list(match[f]))
        lines.append(f"checkerboard 1280 x 960, {hn} frames of {int(frames['n_cur'].min())}..{int(frames['n_cur'].max())} kept planes against "
                     f"{len(planes)} map planes (cape_match_map flags {narrow_flagged}): cape_match_map_wide {spread(checker_ms)}, "
                     f"{int(np.count_nonzero(frames['flags']))} frames flagged, {int(frames['n_matched'].sum())} matches")
        lines.append(f"checkerboard, {hn} frames: host route, 16 threads over cape_host_match_map {host_ms:9.1f} ms, "
                     f"{host_ms / statistics.median(checker_ms):7.1f}x the wide call; decisions equal on {agree} of {hn} frames")
        ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
