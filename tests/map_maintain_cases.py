"""The list maintenance of the map update (cape_map_maintain and its twin cape_host_map_maintain) restated as the reference's loops --
Feature_Map::update_local_map (feature_map.hpp:748-762) and update_staged_map (:805-830) with LocalMapPlane(const StagedMapPlane&)
(map_primitive.cpp:286-318) -- on Python lists, and the helpers that turn a map in pack_map's layout into such a list and back.
Shared by tests/test_map_maintain_host.py and tests/test_gpu_map_maintain.py.

Whether a staged plane's promotion would throw is NOT decided here: every test knows it from how it built the plane and passes it in
(`promotable`), so the restatement has no arithmetic either."""
import numpy as np

PROMOTE_MATCHES, DROP_MISSES, LOST_MISSES = 4, 2, 10

# the classes, named as csrc/cape_map_maintain.h names them
KEEP_LOCAL, PROMOTED, KEEP_STAGED, DROPPED, LOST, PROMOTE_REFUSED = range(6)


def entries_of(arrays, tracks):
    """a map in pack_map's layout as a list of entries: the plane record, its rings [outer, hole, ...] and its track"""
    P, R, V = arrays
    out = []
    for j in range(len(P)):
        rings = [V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]].copy()
                 for r in R[P[j]["ring_first"]: P[j]["ring_first"] + P[j]["ring_count"]]]
        out.append(dict(plane=P[j].copy(), rings=rings, track=tracks[j].copy()))
    return out


def arrays_of(ca, entries, base=None):
    """the entries laid out plane after plane, rings and vertices back to back -- behind `base` = ((P, R, V), T) if given, with
    ring_first and vertex_offset counting from the start of the joined arrays (the retired log)"""
    (P0, R0, V0), T0 = base if base is not None else ((np.zeros(0, ca.MAP_PLANE_DTYPE), np.zeros(0, ca.MAP_RING_DTYPE), np.zeros((0, 2))),
                                                       np.zeros(0, ca.MAP_TRACK_DTYPE))
    P, T = np.zeros(len(entries), ca.MAP_PLANE_DTYPE), np.zeros(len(entries), ca.MAP_TRACK_DTYPE)
    rings, verts, nr, nv = [], [], len(R0), len(V0)
    for j, e in enumerate(entries):
        P[j] = e["plane"]
        P[j]["ring_first"], P[j]["ring_count"] = nr, len(e["rings"])
        T[j] = e["track"]
        for ring in e["rings"]:
            rings.append((nv, len(ring)))
            verts.append(np.asarray(ring, np.float64).reshape(-1, 2))
            nr += 1
            nv += len(ring)
    R = np.array(rings, ca.MAP_RING_DTYPE) if rings else np.zeros(0, ca.MAP_RING_DTYPE)
    V = np.concatenate(verts) if verts else np.zeros((0, 2))
    return ((np.concatenate([P0, P]), np.concatenate([R0, R]), np.ascontiguousarray(np.concatenate([np.asarray(V0).reshape(-1, 2), V]))),
            np.concatenate([T0, T]))


def class_of(ca, track, promotable=True):
    """the reference's if / else chains on one plane's counters and flags"""
    if track["flags"] & ca.MAP_TRACK_STAGED:
        if track["successive_matched"] >= PROMOTE_MATCHES:  # should_add_to_local_map
            return PROMOTED if promotable else PROMOTE_REFUSED  # (the constructor throws: caught, the plane stays where it is)
        elif track["failed_tracking"] >= DROP_MISSES:  # should_remove_from_staged
            return DROPPED
        return KEEP_STAGED
    if track["failed_tracking"] >= LOST_MISSES:  # is_lost
        return LOST
    return KEEP_LOCAL


def class_of_result(ca, result_bits, staged):
    """the class the result bits of the update name (a refused promotion cannot be told from them: PROMOTED)"""
    if result_bits & ca.MAP_RESULT_PROMOTE:
        return PROMOTED
    if result_bits & ca.MAP_RESULT_DROP:
        return DROPPED
    if result_bits & ca.MAP_RESULT_LOST:
        return LOST
    return KEEP_STAGED if staged else KEEP_LOCAL


def reference_maintain(ca, entries, promotable, held=(0, 0, 0)):
    """One maintenance step on a list of entries.  promotable[j]: would LocalMapPlane(staged plane j) be constructed (read for a
    promote candidate only); held: what the retired log holds.  Returns (result: MAP_MAINTAIN_RESULT_DTYPE scalar, the new list or
    None unless DONE, the lost entries in list order -- to be appended to the log if DONE)."""
    local, staged, lost = [], [], []
    n_promoted = n_refused = n_dropped = 0
    for e, ok in zip(entries, promotable):
        cls = class_of(ca, e["track"], ok)
        if cls == PROMOTED:
            track = e["track"].copy()
            track["flags"] = int(track["flags"]) & ~ca.MAP_TRACK_STAGED
            track["failed_tracking"] = 0  # a new LocalMapPlane's; successive_matched, id, result, MOVING and covariance are kept
            local.append(dict(plane=e["plane"], rings=e["rings"], track=track))
            n_promoted += 1
        elif cls == PROMOTE_REFUSED:
            staged.append(e)
            n_refused += 1
        elif cls == DROPPED:
            n_dropped += 1
        elif cls == LOST:
            lost.append(e)
        elif cls == KEEP_STAGED:
            staged.append(e)
        else:
            local.append(e)
    new = local + staged  # the stable partition of the survivors
    full = len(lost) > 0 and held[0] + len(lost) > ca.MAP_RETIRED_MAX_PLANES
    due = n_promoted + n_dropped + len(lost) > 0
    done = due and not full
    count = lambda es: (len(es), sum(len(e["rings"]) for e in es), sum(len(r) for e in es for r in e["rings"]))  # noqa: E731
    size = count(new if done else entries)
    gone = count(lost) if done else (0, 0, 0)
    R = np.zeros(1, ca.MAP_MAINTAIN_RESULT_DTYPE)[0]
    R["flags"] = ca.MAINTAIN_LOG_FULL if full else (ca.MAINTAIN_DONE if due else ca.MAINTAIN_NOTHING)
    R["n_planes"], R["n_rings"], R["n_vertices"] = size
    R["n_local"], R["n_staged"] = len(local), len(staged)
    R["n_promoted"], R["n_promote_refused"], R["n_dropped"], R["n_lost"] = n_promoted, n_refused, n_dropped, len(lost)
    R["n_retired"], R["n_retired_rings"], R["n_retired_vertices"] = (h + g for h, g in zip(held, gone))
    return R, (new if done else None), lost


def same_map(got, want, what=""):
    (P, R, V), Tr = got
    (P2, R2, V2), Tr2 = want
    for name, a, b in (("planes", P, P2), ("rings", R, R2), ("vertices", V, V2), ("tracks", Tr, Tr2)):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what}: {name}"
