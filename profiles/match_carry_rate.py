"""The carried frame (cape_match_carry_save + CAPE_MATCH_CARRY) next to the call it extends.

(a) --flagless-only [--tree OTHER_CHECKOUT] [--label NAME]: the flagless cape_match_polygons_wide on the --frames room batch, alone:
    --rounds rounds of --reps calls, device events, after a warm-up.  With --tree, that of another checkout's package and library on
    the same workload: the A/B against the parent commit (alternate the two processes; run the parent twice to see the spread it shows
    against itself).
(b) default: on the same batch, the carried call (the batch's last frame saved as the carry: frame 0 gains a predecessor) against the
    flagless one, alternating round by round.
(c) default: a one-frame handle over --stream-frames room frames of the trajectory: per call cape_match_polygons_wide(1, CARRY) +
    cape_match_carry_save(0), device events around the pair and the host's wall clock around pair + synchronisation; and the same
    frame pairs through cape_host_match_planes (wall clock; the kept planes fetched outside the clock).

    python profiles/match_carry_rate.py [--frames 4096] [--stream-frames 32] [--rounds 5] [--reps 10] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v, unit="ms"):
    return f"median {statistics.median(v):9.3f} {unit} (min {min(v):9.3f}, max {max(v):9.3f} over {len(v)} rounds)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--stream-frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--flagless-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "rgb-d-slam_amd", "python"))
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    st = torch.cuda.current_stream().cuda_stream

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(calls, reps):
        for _ in range(3):
            for call in calls:
                call()
        torch.cuda.synchronize()
        ms = [[] for _ in calls]
        for _ in range(a.rounds):
            for k, call in enumerate(calls):
                ms[k].append(timed(call, reps))
        return ms

    n = a.frames
    lines = [f"{a.label or 'match_carry_rate'}: {a.rounds} rounds of {a.reps} calls, device events, the calls of a pair alternating round by round"]
    dev = synth_gpu.stream("room", 1, n, device="cuda")
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)

    def flagless():
        ex.match_polygons_wide(n, None, 0, st)

    if a.flagless_only:
        (flagless_ms,) = alternate([flagless], a.reps)
    else:
        ex.match_carry_save(n - 1, st)

        def carried():
            ex.match_polygons_wide(n, None, cape_amd.MATCH_CARRY, st)

        flagless_ms, carried_ms = alternate([flagless, carried], a.reps)
    flagless()
    frames, match, _, _ = ex.polygon_matches_wide(n)
    lines.append(f"room stream, {n} frames: cape_match_polygons_wide, flagless {spread(flagless_ms)}, {int((match >= 0).sum())} matches, "
                 f"{int(np.count_nonzero(frames['flags']))} frames flagged")
    if not a.flagless_only:
        carried()
        cframes, cmatch, _, _ = ex.polygon_matches_wide(n)
        lines.append(f"room stream, {n} frames: cape_match_polygons_wide, carried  {spread(carried_ms)}, frame 0: n_prev {int(cframes[0]['n_prev'])}, "
                     f"{int(cframes[0]['n_matched'])} matches; frames 1.. equal to the flagless call: {bool(np.array_equal(cmatch[1:], match[1:]))}; "
                     f"ratio of the medians {statistics.median(carried_ms) / statistics.median(flagless_ms):.3f}")
    ex.close()
    del dev

    sn = 0 if a.flagless_only else a.stream_frames
    if sn:
        numbers = list(range(sn))
        dev = synth_gpu.stream("room", 1, sn, device="cuda")
        T = np.ascontiguousarray(synth_gpu.relative_poses("room", 1, numbers)).reshape(sn, 1, 16)
        ex = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)
        kept, rows = [], []
        pair_us, wall_us = [], []

        def one(f, flags):
            ex.match_polygons_wide(1, T[f], flags, st)
            ex.match_carry_save(0, st)

        for rnd in range(a.rounds + 1):  # (round 0 warms up)
            dev_us, host_us = [], []
            for f in range(sn):
                ex.extract_device(dev[f:f + 1].data_ptr(), 1, st)
                ex.build_polygons(1, st)
                torch.cuda.synchronize()
                flags = cape_amd.MATCH_CARRY if f else 0
                t0 = time.perf_counter()
                ms = timed(lambda: one(f, flags), 1)
                host_us.append((time.perf_counter() - t0) * 1e6)
                dev_us.append(ms * 1e3)
                if rnd == 0:
                    kept.append(ex.kept_planes(1)[0])
                    rows.append(ex.polygon_matches_wide(1)[1][0].copy())
            if rnd:
                pair_us.append(statistics.median(dev_us[1:]))
                wall_us.append(statistics.median(host_us[1:]))
        lines.append(f"one-frame handle, {sn} room frames, per call match_polygons_wide(1, CARRY) + match_carry_save(0) (median over the calls of a "
                     f"round): device events {spread(pair_us, 'us')}")
        lines.append(f"one-frame handle, the same pair of calls, host wall clock to completion (launches + synchronisation): {spread(wall_us, 'us')}")
        host_round = []
        agree = 0
        for rnd in range(a.rounds):
            us = []
            for f in range(1, sn):
                t0 = time.perf_counter()
                m = cape_amd.host_match_planes(kept[f - 1][0], kept[f][0], T[f].reshape(4, 4), 0)
                us.append((time.perf_counter() - t0) * 1e6)
                if rnd == 0:
                    agree += int(list(m) == list(rows[f][: len(m)]))
            host_round.append(statistics.median(us))
        lines.append(f"one-frame handle, the same frame pairs through cape_host_match_planes (one thread, wall clock): {spread(host_round, 'us')}; "
                     f"decisions equal on {agree} of {sn - 1} pairs")
        ex.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
