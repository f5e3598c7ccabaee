"""cape_match_map_shards on the 4 096-frame room batch packed as ONE shard, against maps of 64 and 1 024 planes, next to its two
baselines: cape_match_map on the same frames in the same process -- the two calls alternate over --rounds rounds of --reps calls,
device events, after a warm-up of both -- and the host route a map owner had before, 16 threads over cape_host_shard_frame +
cape_host_match_map on the shard's bytes (Python wrappers included: that is the route as a caller of the binding takes it).

    python profiles/shard_match_rate.py [--frames 4096] [--host-frames 256] [--rounds 5] [--reps 10] [--out FILE]
    python profiles/shard_match_rate.py --record-only [--tree OTHER_CHECKOUT]   # cape_match_map alone, e.g. of another revision

--record-only with --tree times cape_match_map of another checkout's package and library on the same workload (the A/B of a change
to the shared kernels: alternate the two processes).  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python profiles/shard_match_rate.py --rounds 1 --reps 3 --host-frames 0`."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host-frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--record-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "rgb-d-slam_amd", "python"))
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

    shards = not a.record_only
    if shards:
        _, _, most = ex.count_primitives(n)
        layout = ex.gather_configure(n, planes_per_frame=max(most, 1), polygons=True, vertices_per_frame=ex.boundary_capacity)  # nothing dropped
        ptr = ex.pack(n, 0, st)
        buf = ex.packed_host()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    lines = [f"{a.label or 'shard_match_rate'}: room stream, {n} frames as one shard, {a.rounds} rounds of {a.reps} calls, the two device "
             f"calls alternating round by round"]
    for size in (64, 1024):
        planes = list(base[:size])
        while len(planes) < size:
            nw, d, x, y, c, ring, h = base[int(rng.integers(len(base)))]
            planes.append((nw, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        arrays = cape_amd.pack_map(planes)
        ex.upload_map(arrays)

        def by_records():
            ex.match_map(n, T, None, 0, st)

        def by_shards():
            ex.match_map_shards(ptr, 1, layout, T, None, 0, st)

        for _ in range(3):
            by_records()
            if shards:
                by_shards()
        torch.cuda.synchronize()
        rec_ms, shard_ms = [], []
        for _ in range(a.rounds):
            rec_ms.append(timed(by_records))
            if shards:
                shard_ms.append(timed(by_shards))
        frames, match = ex.map_matches(n)
        lines.append(f"map of {size:4d} planes: cape_match_map        {spread(rec_ms)}, {int(frames['n_matched'].sum())} matches, "
                     f"{int(np.count_nonzero(frames['flags']))} frames flagged")
        if not shards:
            continue
        sframes, smatch = ex.shard_map_matches(n)
        same = bool(np.array_equal(frames, sframes) and np.array_equal(match, smatch))
        lines.append(f"map of {size:4d} planes: cape_match_map_shards {spread(shard_ms)}, results equal to cape_match_map: {same}; "
                     f"ratio of the medians {statistics.median(shard_ms) / statistics.median(rec_ms):.3f}")
        hn = min(a.host_frames, n)
        if hn:
            def host_route(k):
                det, _ = cape_amd.host_shard_frame(buf, layout, k)
                return cape_amd.host_match_map(arrays, [d[:7] for d in det], T[k], None, 0)

            with ThreadPoolExecutor(16) as pool:
                t0 = time.perf_counter()
                out = list(pool.map(host_route, range(hn)))
                host_s = time.perf_counter() - t0
            agree = sum(1 for k in range(hn) if not sframes[k]["flags"] and list(out[k][0]) == list(smatch[k]))
            host_ms = host_s * 1e3 * n / hn
            lines.append(f"map of {size:4d} planes: host route, 16 threads over host_shard_frame + host_match_map {host_ms:9.1f} ms per {n} "
                         f"frames (measured on {hn}), {host_ms / statistics.median(shard_ms):6.1f}x the shard call; decisions equal on "
                         f"{agree} of {hn} host frames")
    ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
