"""cape_map_visibility on the poses of 4 096 room frames against a 64-plane and a 1 024-plane map (device events after warm-up), the
cape_match_map it feeds in the same run for scale (with the caller's skip = NULL and with CAPE_MATCH_MAP_DEVICE_SKIP), and the host
twin cape_host_map_visibility on 16 threads over the same frames -- the per-frame host work the device call replaces.  Also: the
share of (frame, plane) pairs the classify kernel settles without an intersection (non-finite, or the bounding box beside the
rectangle; restated in numpy on the host frames), the share of pairs skipped, and the undecided count.

    python profiles/map_visibility_rate.py [--frames 4096] [--host-frames 256] [--out profiles/r10_map_visibility.txt]

The maps are those of profiles/map_match_rate.py."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))


def settled_share(planes, T, W, H, fx, fy, cx, cy):
    """share of (frame, plane) pairs with a non-finite screen coordinate or a bounding box beside the open rectangle (float64 numpy,
    not the kernel's statement order: a figure, not a check)"""
    settled = total = 0
    R, t = T[:, :3, :3], T[:, :3, 3]
    for _, _, x, y, c, ring, _ in planes:
        pts = c[None, :] + ring[:, :1] * x[None, :] + ring[:, 1:2] * y[None, :]  # vertices x 3
        cam = np.einsum("fij,vj->fvi", R, pts) + t[:, None, :]
        with np.errstate(all="ignore"):
            u = (fx * cam[..., 0] + cx * cam[..., 2]) / cam[..., 2]
            v = (fy * cam[..., 1] + cy * cam[..., 2]) / cam[..., 2]
        bad = ~(np.isfinite(u).all(1) & np.isfinite(v).all(1))
        beside = (u.max(1) <= 1) | (u.min(1) >= W - 1) | (v.max(1) <= 1) | (v.min(1) >= H - 1)
        settled += int(np.count_nonzero(bad | beside))
        total += len(T)
    return settled / max(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    n = a.frames
    W, H, intr = 640, 480, synth.DEFAULT_INTRINSICS
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    c2w = synth_gpu._poses("room", 1, 0, n)
    ex = Extractor(W, H, cylinders=False, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    res = ex.results(n)
    pol, ver = ex.polygons(n)

    def kept(f):
        out = []
        for i, s in enumerate(res.segments(f)):
            p = pol[f, i]
            if s["is_output"] and (p["flags"] & cape_amd.POLY_VALID) and p["vertex_count"] >= 3:
                out.append((s["out_normal"].copy(), float(s["d"]), p["x_axis"].copy(), p["y_axis"].copy(), p["center"].copy(),
                            ver[f, p["vertex_offset"]: p["vertex_offset"] + p["vertex_count"]].copy(), float(p["area"])))
        return out

    def unit(v):
        return v / np.linalg.norm(v)

    base = []
    for f in range(0, n, max(1, n // 16)):
        R, o = c2w[f]
        for nn, d, x, y, c, ring, _ in kept(f):
            nw, cw = unit(R @ nn), o + R @ c
            base.append((nw, float(-(nw @ cw)), unit(R @ x), unit(R @ y), cw, ring, []))
    rng = np.random.default_rng(0)
    T = np.zeros((n, 4, 4))
    for f in range(n):
        R, o = c2w[f]
        T[f, :3, :3], T[f, :3, 3], T[f, 3, 3] = R.T, -R.T @ o, 1.0

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    lines = [f"cape_map_visibility, poses of the room stream, {n} frames, {a.reps} repetitions behind 3 warm-up calls"]
    for size in (64, 1024):
        planes = list(base[:size])
        while len(planes) < size:
            nw, d, x, y, c, ring, h = base[int(rng.integers(len(base)))]
            planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        arrays = cape_amd.pack_map(planes)
        ex.upload_map(arrays)
        vis_ms = timed(lambda: ex.map_visibility(n, T, None, st))
        words, undecided = ex.map_visibility_words(n)
        skipped = sum(int(np.count_nonzero((words >> k) & 1)) for k in range(32)) / (n * size)
        match_ms = timed(lambda: ex.match_map(n, T, None, 0, st))
        flag_ms = timed(lambda: ex.match_map(n, T, None, cape_amd.MATCH_MAP_DEVICE_SKIP, st))
        hn = min(a.host_frames, n)
        calls = [cape_amd.host_map_visibility_call(arrays, T[f], W, H, intr["fx"], intr["fy"], intr["cx"], intr["cy"]) for f in range(hn)]
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            out = list(pool.map(lambda run: run(), calls))
            host_s = time.perf_counter() - t0
        agree = sum(1 for f in range(hn) if np.array_equal(out[f], words[f]))
        host_ms = host_s * 1e3 * n / hn
        share = settled_share(planes, T[:hn], W, H, intr["fx"], intr["fy"], intr["cx"], intr["cy"])
        lines.append(f"map of {size:4d} planes: cape_map_visibility {vis_ms:8.3f} ms per {n} frames; cape_match_map {match_ms:8.3f} ms with "
                     f"skip = NULL, {flag_ms:8.3f} ms with CAPE_MATCH_MAP_DEVICE_SKIP (visibility / match = {vis_ms / match_ms:5.2f}); "
                     f"{100 * skipped:5.1f} % of the pairs skipped, {100 * share:5.1f} % settled without an intersection (first {hn} "
                     f"frames), {undecided} undecided; host twin, 16 native threads {host_ms:9.1f} ms per {n} frames (measured on {hn}), "
                     f"device/host speed-up {host_ms / vis_ms:6.1f}x; words equal on {agree} of {hn} host frames")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
