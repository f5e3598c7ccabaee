"""cape_match_map on 4 096 room frames against a 64-plane and a 1 024-plane map (device events after warm-up), and the host twin
cape_host_match_map on 16 threads over the same inputs -- the baseline the device path replaces.  The twin's arguments are packed
before its clock starts; the threads then spend their time in the native call (the C++ host class, GIL released).

    python profiles/map_match_rate.py [--frames 4096] [--host-frames 512] [--out FILE]

The map is built from the kept planes of a few frames of the stream, lifted to world with their true poses and padded with
perturbed copies.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python profiles/map_match_rate.py --reps 3`."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host-frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    n = a.frames
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    c2w = synth_gpu._poses("room", 1, 0, n)
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
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
    lines = [f"cape_match_map, room stream, {n} frames, {sum(len(kept(f)) for f in range(min(n, 256))) / min(n, 256):.2f} kept planes "
             f"per frame (first 256 frames)"]
    for size in (64, 1024):
        planes = list(base[:size])
        while len(planes) < size:
            nw, d, x, y, c, ring, h = base[int(rng.integers(len(base)))]
            planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        arrays = cape_amd.pack_map(planes)
        ex.upload_map(arrays)
        for _ in range(3):
            ex.match_map(n, T, None, 0, st)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ex.match_map(n, T, None, 0, st)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        frames, match = ex.map_matches(n)
        flagged = int(np.count_nonzero(frames["flags"] & cape_amd.MATCH_EXACT_OVERFLOW))
        # host twin, 16 threads, on the first host-frames frames
        hn = min(a.host_frames, n)
        # the arguments are packed beforehand: the 16 threads time the native calls only (ctypes releases the GIL for them)
        calls = [cape_amd.host_match_map_call(arrays, kept(f), T[f], None, 0) for f in range(hn)]
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            out = list(pool.map(lambda run: run(), calls))
            host_s = time.perf_counter() - t0
        agree = sum(1 for f in range(hn) if not (frames[f]["flags"] & 1) and list(out[f][0]) == list(match[f]))
        host_ms = host_s * 1e3 * n / hn
        lines.append(f"map of {size:4d} planes: device {ms:8.3f} ms per {n} frames ({n / ms * 1e3:10.0f} frames/s), "
                     f"{int(frames['n_matched'].sum())} matches, {flagged} frames flagged; host twin, 16 native threads "
                     f"{host_ms:9.1f} ms per {n} frames (measured on {hn}), device/host speed-up {host_ms / ms:6.1f}x; "
                     f"decisions equal on {agree} of {hn} host frames")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
