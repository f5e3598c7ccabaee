"""Frames with an exact number of plane segments, for the tests of the device's plane-count capacities: 16 kept planes in the
narrow polygon matchers, 32 segments in the everyday grow kernels, 64 segments per record (and 64 kept planes in cape_match_map and
its shard twin), 128 kept planes in the wide matchers, the carried frame and the map update's tables.

Two generators, both deterministic and CPU-only (the oracle counts):

  checker_with(n, W, H, tile)   the checkerboard of tilted facets of test_gpu_parity, tiles zeroed from the END of the tile list (row
                                major, so from the bottom right corner) until exactly n plane segments are left.  Every facet that
                                survives is a segment, an output plane and a kept plane of its own.
  lattice_with(n, W, H, a, b)   one fronto-parallel wall at 2000 mm behind a lattice: every (a+1)-th cell column and every (b+1)-th
                                cell row is zeroed, which leaves panes of a x b cells -- separate plane segments that are coplanar
                                but never merge (the zeroed cells keep them from being neighbours).  Panes are zeroed from the end
                                until n are left.  Every pair of such planes passes both gates of the matchers.

Both return (depth, intr, oracle_result) and raise CapacityCaseError if no drop count gives the target.  Results are cached: the
CPU test of the generators and the GPU tests share one oracle run per case.  The cached arrays are read-only.
"""
import functools

import numpy as np

CELL = 20  # pixels per cell side (the reference's depthMapPatchSize)

# (n_planes, W, H, tile): every checkerboard the GPU tests use
CHECKER_CASES = ([(n, 640, 480, 80) for n in (15, 16, 17, 31, 32, 33)]
                 + [(n, 1280, 960, 100) for n in (62, 63, 64, 65)]
                 + [(n, 1920, 1080, 120) for n in (127, 128, 129)])
# (n_planes, W, H, a, b): every lattice the GPU tests use (103: no pane dropped)
LATTICE_CASES = [(n, 1280, 960, 4, 5) for n in (64, 65, 103)]


class CapacityCaseError(RuntimeError):
    pass


def _intr(W):
    from cape_amd import synth

    return {k: v * (W / 640.0) for k, v in synth.DEFAULT_INTRINSICS.items()}


def _count(oracle, depth):
    res = oracle.run(depth)
    return len(res.segments), res


def _search(full, n_planes, regions, what):
    """Zero regions[-k:] for k = 0, 1, .. until the oracle counts n_planes segments.  A zeroed region removes at most the one
    segment it held, so the walk starts at k = (count of the whole frame) - n_planes and ends when the count falls below the
    target or the regions run out."""
    import cape_oracle_py

    H, W = full.shape
    oracle = cape_oracle_py.Oracle(W, H, cylinders=False, **_intr(W))
    whole, res = _count(oracle, full)
    if whole < n_planes:
        raise CapacityCaseError(f"{what}: the whole frame has {whole} plane segments, fewer than {n_planes}")
    for k in range(whole - n_planes, len(regions) + 1):
        depth = full.copy()
        for sl in regions[len(regions) - k:]:
            depth[sl] = 0.0
        got, res = _count(oracle, depth)
        if got == n_planes:
            depth.setflags(write=False)
            return depth, res
        if got < n_planes:
            break
    raise CapacityCaseError(f"{what}: no drop count leaves exactly {n_planes} plane segments")


def _tiles(W, H, tile):
    return [(slice(ty, min(ty + tile, H)), slice(tx, min(tx + tile, W))) for ty in range(0, H, tile) for tx in range(0, W, tile)]


@functools.lru_cache(maxsize=None)
def checker_with(n_planes, W, H, tile):
    from test_gpu_parity import _checkerboard_of_facets

    full, intr = _checkerboard_of_facets(W, H, tile=tile)
    assert intr == _intr(W)
    depth, res = _search(full, n_planes, _tiles(W, H, tile), f"checkerboard {W}x{H} tile {tile}")
    return depth, intr, res


def _spans(cells, pane):
    """the cell ranges between the zeroed lines: [0, pane), [pane + 1, 2 pane + 1), .."""
    return [(lo, min(lo + pane, cells)) for lo in range(0, cells, pane + 1)]


def lattice_wall(W, H, a, b, seed=5):
    """(depth, panes): the wall behind the lattice and the pixel slices of its panes, row major"""
    z = np.round(2000.0 + np.random.default_rng(seed).normal(0, 0.6, (H, W))).astype(np.float32)
    cols, rows = _spans(W // CELL, a), _spans(H // CELL, b)
    for _, hi in cols:
        z[:, hi * CELL:(hi + 1) * CELL] = 0.0
    for _, hi in rows:
        z[hi * CELL:(hi + 1) * CELL, :] = 0.0
    panes = [(slice(r0 * CELL, r1 * CELL), slice(c0 * CELL, c1 * CELL)) for r0, r1 in rows for c0, c1 in cols]
    return z, panes


@functools.lru_cache(maxsize=None)
def lattice_with(n_planes, W, H, a, b):
    full, panes = lattice_wall(W, H, a, b)
    depth, res = _search(full, n_planes, panes, f"lattice {W}x{H} panes of {a}x{b} cells")
    return depth, _intr(W), res


@functools.lru_cache(maxsize=None)
def checker_oracle(n_planes, W, H, tile, cylinders):
    """the oracle's result for checker_with(n_planes, W, H, tile), with or without the cylinder branch (the generator counts
    without it; tests/test_capacity_cases.py holds the count with it to the same target)"""
    import cape_oracle_py

    depth, intr, res = checker_with(n_planes, W, H, tile)
    return cape_oracle_py.Oracle(W, H, cylinders=True, **intr).run(depth) if cylinders else res


def pane_pitch_mm(W, a, z=2000.0):
    """the distance between two panes' left edges on the wall, in millimetres: (a + 1) cells seen at depth z"""
    return (a + 1) * CELL * z / _intr(W)["fx"]
