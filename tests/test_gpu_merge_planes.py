"""merge_planes in every grow instance, on frames that really merge.

merge_planes (fuse adjacent plane segments, refit the absorber, feed the merged mask into the boundary ring) exists three times on the
device: in grow_tail of cape_grow_common.h (the 32- and 64-segment instances of cape_grow.hip and the one-frame chain), in the cylinder
group kernel of cape_resume.hip, whose wave 0 runs the same grow_tail, and in cape_grow_general.hip with its multi-word adjacency
matrix.  The frames come from tests/merge_cases.py; tests/test_merge_cases.py pins on the CPU what each of them reaches (one root
absorbing two segments, an absorbed row expanding its absorber, a rejected pair beside a merged one, a group dropped for fewer than
three boundary points, merges across the 64-segment record border and across the adjacency words).  Every comparison is compare_frame
of test_gpu_parity.py -- segments, sums, merge labels, label grids, planes, covariances, boundary point sets, tolerance 0 -- and every
test asserts the routing it is about: the segment count (more than 32: the 64-segment redo), the spill records and the number of frames
through the general instance (Extractor.spill_info)."""
import numpy as np
import pytest

import merge_cases as M
from test_gpu_parity import compare_frame
from test_gpu_polygon import host_poly  # noqa: F401  (the fixture: the host polygon class through cape_host_polygon)

pytestmark = pytest.mark.gpu

SMALL_CASES = ["pair", "star", "chain", "chain_reject", "masked_ring", "lattice_6x4", "lattice_12x4", "lattice_8x8", "lattice_12x8",
               "lattice_12x8_lean", "lattice_cyl_900"]
REJECTED_LINE = "Could not find a correct boundary polygon, rejecting plane segment"


def _batch(names, grid, cyl, room=True):
    """(frames, oracle results) of the named cases, between two ordinary room frames"""
    frames, want = [M.case(nm)[0] for nm in names], [M.oracle(nm, cyl) for nm in names]
    if room:
        depth, r = M.room(grid[0], grid[1], cyl)
        frames, want = [depth] + frames + [depth], [r] + want + [r]
    return np.stack(frames), want


def _spilled(want):
    """(spill records, frames through the general instance) a batch of these frames needs when the fast instances serve the grid"""
    over = [len(r.segments) for r in want if len(r.segments) > 64]
    return sum((n - 1) // 64 for n in over), len(over)


def _assert_frame(ex, res, f, r):
    """frame f equals the oracle's r, its record chain is as long as r's segments demand and nothing was truncated"""
    hdr = res.records["header"]
    n = len(r.segments)
    assert int(hdr["n_plane_segments"][f]) == n and int(hdr["status"][f]) & 0x7 == 0, f"frame {f}"
    assert len(res.chain(f)) == max(1, (n + 63) // 64), f"frame {f}: {n} segments in {len(res.chain(f))} records"
    compare_frame(r, ex, res, f, check_cells=False)


@pytest.mark.parametrize("cyl", [False, True])
def test_batch_chain_640(oracle_mod, cyl):
    """One batch at 640 x 480: every small case, the lattices of 23 segments (the 32-segment instance), 46 and 62 (the 64-segment
    redo), 92 twice (the general instance and a spill record each), the lattice with a cylinder, room frames around them.  Twice on
    one handle.  The group of masked_ring that keeps two boundary points is reported through the log callback."""
    from cape_amd import Extractor

    frames, want = _batch(SMALL_CASES, M.SMALL, cyl)
    n = len(frames)
    counts = [len(r.segments) for r in want]
    assert sorted(c for c in counts if c > 32) == [46, 62, 92, 92] and counts[SMALL_CASES.index("lattice_6x4") + 1] == 23
    ex = Extractor(640, 480, cylinders=cyl, max_batch=n, **M.intrinsics(640))
    lines = []
    ex.set_log_callback(lambda level, msg, frame: lines.append((msg, frame)))
    first = None
    for rep in range(2):
        assert ex.extract_host(frames) == n
        res = ex.results(n)
        used, pool, general = ex.spill_info()
        assert (used, general) == _spilled(want) == (2, 2) and pool >= used
        for f in range(n):
            _assert_frame(ex, res, f, want[f])
        hdr = res.records["header"]
        if first is None:
            first = (hdr.copy(), res.plane_labels.copy())
        # (which spill record a frame continues in is decided by an atomic counter: the two 92-segment frames may swap theirs)
        differs = [(name, f) for name in hdr.dtype.names for f in range(n) if hdr[name][f] != first[0][name][f]]
        assert all(name == "next_record" and counts[f] > 64 for name, f in differs), f"the second call differs: {differs}"
        assert sorted(hdr["next_record"]) == sorted(first[0]["next_record"]) and np.array_equal(res.plane_labels, first[1])
    masked = SMALL_CASES.index("masked_ring") + 1
    dropped = [f for f, r in enumerate(want) for _ in range(M.classify(r, 640)["dropped_roots"])]
    assert masked in dropped
    assert sorted(ln[1] for ln in lines if ln[0] == REJECTED_LINE) == sorted(dropped * 2), "one line per dropped plane and call"
    assert not [ln for ln in lines if "capacity exceeded" in ln[0]]
    cyl_frame = SMALL_CASES.index("lattice_cyl_900") + 1
    assert int(res.records["header"]["n_cylinders"][cyl_frame]) == (1 if cyl else 0)
    ex.close()


@pytest.mark.parametrize("mode", ["strips", "bands"])
def test_one_frame_handles(oracle_mod, monkeypatch, mode):
    """max_batch = 1, one case per call: the one-frame chain (strips: the 64-segment instance on every frame) and the classic chain
    on such a handle (bands: the 32-segment kernel, the redo, the signal kernel).  The 92-segment frames hand over to the general
    kernel, whose last wave signals the host; an ordinary frame follows each of them."""
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_STAGE_A", mode)
    for cyl in (False, True):
        ex = Extractor(640, 480, cylinders=cyl, max_batch=1, **M.intrinsics(640))
        room, want_room = M.room(640, 480, cyl)
        for name in SMALL_CASES + ["lattice_12x8", "pair"]:
            r = M.oracle(name, cyl)
            assert ex.extract_host(M.case(name)[0]) == 1
            res = ex.results(1)
            _assert_frame(ex, res, 0, r)
            spilled = len(r.segments) > 64
            assert (int(res.records["header"]["next_record"][0]) >= 1) == spilled
            assert ex.spill_info()[::2] == ((1, 1) if spilled else (0, 0)), name
            if spilled:
                assert ex.extract_host(room) == 1
                _assert_frame(ex, ex.results(1), 0, want_room)
        ex.close()


@pytest.mark.parametrize("cyl", [False, True])
def test_general_instance_640(oracle_mod, monkeypatch, cyl):
    """CAPE_GROW=general: every case through the general instance's own merge loop, its adjacency rows of one word (up to 64
    segments) and of two (92 segments: columns on both sides of the word border, row 63 linked beyond it)."""
    from cape_amd import Extractor

    frames, want = _batch(SMALL_CASES + ["lattice_cyl_600", "lattice_cyl_1400"], M.SMALL, cyl)
    n = len(frames)
    monkeypatch.setenv("CAPE_GROW", "general")
    ex = Extractor(640, 480, cylinders=cyl, max_batch=n, **M.intrinsics(640))
    monkeypatch.delenv("CAPE_GROW")
    for rep in range(2):
        assert ex.extract_host(frames) == n
        res = ex.results(n)
        used, pool, general = ex.spill_info()
        assert general == n and used == _spilled(want)[0] == 2, "every frame went through the general instance"
        for f in range(n):
            _assert_frame(ex, res, f, want[f])
    ex.close()


@pytest.mark.parametrize("cyl", [False, True])
def test_u64_grid_1280(oracle_mod, cyl):
    """64 x 48 cells, rows of one 64-bit mask: 62 segments with 30 merges (the redo), 92 and 94 segments (the general instance), the
    leaning lattice with merge roots in its spill record."""
    from cape_amd import Extractor

    names = ["mid_8x8", "mid_12x8", "mid_12x8_lean"]
    frames, want = _batch(names, M.MID, cyl)
    n = len(frames)
    assert [len(r.segments) for r in want[1:-1]] == [62, 92, 94]
    ex = Extractor(1280, 960, cylinders=cyl, max_batch=n, **M.intrinsics(1280))
    for rep in range(2):
        assert ex.extract_host(frames) == n
        res = ex.results(n)
        assert ex.spill_info()[::2] == (2, 2)
        for f in range(n):
            _assert_frame(ex, res, f, want[f])
    ex.close()


@pytest.mark.parametrize("cyl", [False, True])
@pytest.mark.parametrize("instance", ["wide", "general"])
def test_mask128_grid_1920(oracle_mod, monkeypatch, instance, cyl):
    """96 x 54 cells, rows of two words (Mask128): 34 segments (the redo), 70 and 72 (handed to the general instance) -- and all of
    them through the general instance from the start."""
    from cape_amd import Extractor

    names = ["big_6x6", "big_9x8", "big_9x8_lean"]
    frames, want = _batch(names, M.BIG, cyl, room=False)
    n = len(frames)
    assert [len(r.segments) for r in want] == [34, 70, 72]
    if instance == "general":
        monkeypatch.setenv("CAPE_GROW", "general")
    ex = Extractor(1920, 1080, cylinders=cyl, max_batch=n, **M.intrinsics(1920))
    for rep in range(2):
        assert ex.extract_host(frames) == n
        res = ex.results(n)
        assert ex.spill_info()[::2] == (2, n if instance == "general" else 2)
        for f in range(n):
            _assert_frame(ex, res, f, want[f])
    ex.close()


@pytest.mark.parametrize("mode", ["wave", "group", "off"])
def test_resume_modes(oracle_mod, monkeypatch, mode):
    """CAPE_SCHEDULE=two with cylinders on: the plane-only pass parks the lattice frames at their cylinder candidate, and the finisher
    -- one wavefront, one workgroup (cape_resume.hip) or the cylinder kernel from scratch -- runs grow_tail with its seven merges."""
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_RESUME", mode)
    monkeypatch.setenv("CAPE_SCHEDULE", "two")
    names = ["lattice_cyl_600", "lattice_cyl_1400", "lattice_cyl_900"]
    frames, want = _batch(names, M.SMALL, True)
    n = len(frames)
    ex = Extractor(640, 480, cylinders=True, max_batch=n, **M.intrinsics(640))
    for rep in range(2):
        assert ex.extract_host(frames) == n
        res = ex.results(n)
        for f in range(n):
            _assert_frame(ex, res, f, want[f])
        assert list(res.records["header"]["n_cylinders"][1:-1]) == [1, 1, 1]
        assert all(int((r.merge_labels != np.arange(len(r.merge_labels))).sum()) == 7 for r in want[1:-1])
    ex.close()


@pytest.mark.parametrize("name", ["lattice_12x8", "lattice_12x8_lean"])
def test_downstream_of_a_merged_chain(host_poly, oracle_mod, name):  # noqa: F811
    """The 92-segment frames through cape_build_polygons: every output plane's polygon, in the frame's own record and in its spill
    record, equals the host class on the same boundary candidates bit for bit; the rows of absorbed segments stay empty; kept_planes
    lists exactly the oracle's output roots, in order -- among them a merge root with a member in the spill record."""
    from cape_amd import POLY_VALID
    from test_gpu_match_wide import _extract
    from test_gpu_polygon import _center, _same

    depth, intr = M.case(name)
    r = M.oracle(name, False)
    roots = r.planes[:, 19].astype(int).tolist()
    ml = r.merge_labels.astype(int)
    straddling = [k for k in roots if k < 64 and (ml[64:] == k).any()]
    assert straddling, "no output root of the first record has a member in the spill record"
    ex, st = _extract(np.stack([depth]), 640, 480, intr)
    res = ex.results(1)
    _assert_frame(ex, res, 0, r)
    assert ex.spill_info()[::2] == (1, 1)
    pol, ver = ex.polygons(1)
    spol, sver = ex.spill_polygons(0, 1)
    compared = []
    for part, (rec, slab) in enumerate(res.chain(0)):
        prow, vslab = (pol[0], ver[0]) if part == 0 else (spol[0], sver[0])
        n_seg = min(64, int(rec["header"]["n_plane_segments"]))
        for i in range(n_seg):
            s, p = rec["segments"][i], prow[i]
            if not s["is_output"]:
                assert not p["flags"] and not p["vertex_count"], f"record {part} segment {i}: a polygon for a segment that is no plane"
                continue
            pts = slab[int(s["boundary_offset"]): int(s["boundary_offset"]) + int(s["boundary_count"])]
            o, c = int(p["vertex_offset"]), int(p["vertex_count"])
            _same(p, vslab[o:o + c], host_poly(pts, s["normal"], _center(s)), f"record {part} segment {i} ({len(pts)} points)")
            assert p["flags"] & POLY_VALID and c >= 3
            compared.append(64 * part + i)
        assert not prow[n_seg:]["flags"].any() and not prow[n_seg:]["vertex_count"].any(), f"record {part}: rows beyond its segments"
    assert compared == roots
    kept = ex.kept_planes(1)
    assert kept[0][1] == roots, "the kept planes are the oracle's output roots, in order"
    assert set(straddling) <= set(kept[0][1])
    if name.endswith("_lean"):
        assert any(k >= 64 and (ml == k).sum() >= 2 for k in kept[0][1]), "a kept merge root of the spill record"
    ex.close()
