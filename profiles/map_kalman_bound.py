"""How far a 1e-12 relative error in the measurement covariance R moves the Kalman step: the figure behind KALMAN_BOUND of
tests/test_gpu_map_kalman.py.  The device's R passes through ocml's pow, the host's through the C library's; the measurement test grants
the two 1e-12 relative.  Here the eight room frames of that test are extracted and matched against the test's map, and for every matched
pair the HOST's own R (cape_host_plane_covariance, cape_host_world_plane_covariance) goes through cape_host_map_kalman once as it is and
--draws times multiplied entry by entry by 1 + 1e-12 u, u a random symmetric matrix in [-1, 1]: the largest relative change of the new
plane and of the new covariance is reported, and whether any result bit or counter changed.  The matching runs on the device; the
algebra measured is the host's alone.

    python profiles/map_kalman_bound.py [--draws 200] [--out profiles/r12_map_kalman_bound.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rgb-d-slam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cape_amd as ca
    from test_gpu_map_kalman import _c2w, _tracks
    from test_gpu_map_match import _stream, _w2c
    from test_gpu_map_measure import _detected, _pose_covariances
    from test_map_update_host import _rel

    L = ca._host_library()
    vp = C.c_void_p
    L.cape_host_plane_covariance.argtypes = [vp, C.c_double, vp, vp]
    L.cape_host_world_plane_covariance.argtypes = [vp, C.c_double, vp, vp, vp, vp]
    p = lambda x: x.ctypes.data_as(vp)
    n = 8
    ex, st, c2w = _stream("room", 11, 20, 5, n)
    T = np.stack([_c2w(*c2w[f]) for f in range(n)])
    W2C = np.stack([_w2c(*c2w[f]) for f in range(n)])
    S = _pose_covariances(np.random.default_rng(21), n)
    ex.map_measure(n, T, S, st)
    meas = ex.map_measurements(n)
    source = next(f for f in range(n) if len(meas[f]) > 1)
    map_meas = [m for m in meas[source] if m["flags"] & ca.MEASURE_STAGEABLE]
    arrays, tracks = ca.pack_map([m["plane"] for m in map_meas]), _tracks(map_meas)
    ex.upload_map(arrays)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    _, match, _, _ = ex.map_matches_wide(n)
    det = _detected(ex, n)
    rng = np.random.default_rng(5)
    worst_x = worst_p = 0.0
    pairs = changed = 0
    for f in range(n):
        # the frame's rows from the host's algebra (the polygon bit is the device row's: that decision is the host's bit for bit)
        rows = np.zeros(len(det[f][0]), ca.PLANE_MEASUREMENT_DTYPE)
        for r, d, m in zip(rows, det[f][0], meas[f]):
            nn, dd, cov = np.ascontiguousarray(d[0]), float(d[1]), np.ascontiguousarray(d[7])
            planeCov, worldCov, z = np.zeros(16), np.zeros(16), np.zeros(4)
            ok = L.cape_host_plane_covariance(p(nn), dd, p(cov), p(planeCov)) and L.cape_host_world_plane_covariance(
                p(nn), dd, p(np.ascontiguousarray(T[f])), p(planeCov), p(np.ascontiguousarray(S[f])), p(worldCov))
            assert ok and m["flags"] & ca.MEASURE_KEPT
            L.cape_host_plane_to_world(p(nn), dd, p(np.ascontiguousarray(T[f])), p(z))
            r["normal"], r["d"], r["covariance"], r["flags"] = z[:3], z[3], worldCov.reshape(4, 4), m["flags"]
        _, base_rows, base_res = ca.host_map_kalman(arrays, tracks, match[f], rows)
        hit = [int(i) for i in match[f] if i >= 0 and base_rows[i]["flags"] & ca.FUSION_STATE]
        pairs += len(hit)
        for _ in range(a.draws):
            pert = rows.copy()
            for i in hit:
                u = rng.uniform(-1, 1, (4, 4))
                pert[i]["covariance"] = rows[i]["covariance"] * (1 + 1e-12 * (u + u.T) / 2)
            _, prow, pres = ca.host_map_kalman(arrays, tracks, match[f], pert)
            changed += int(pres.tobytes() != base_res.tobytes())
            for i in hit:
                worst_x = max(worst_x, _rel(np.append(prow[i]["normal"], prow[i]["d"]), np.append(base_rows[i]["normal"], base_rows[i]["d"])))
                worst_p = max(worst_p, _rel(prow[i]["covariance"], base_rows[i]["covariance"]))
    ex.close()
    lines = [f"cape_host_map_kalman under a 1e-12 relative perturbation of R: room stream (seed 11, frames 20, 25, ..), {n} frames, map of "
             f"{len(map_meas)} planes from frame {source}, {pairs} matched pairs with a new state, {a.draws} draws per frame",
             f"largest relative change of the new plane (normal, d) {worst_x:.3e}, of the new covariance {worst_p:.3e}",
             f"frames x draws whose result bits or counters changed: {changed} of {n * a.draws}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
