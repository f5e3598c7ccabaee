"""Frames whose plane segments really merge, for the tests of merge_planes in every grow instance.

Two parallel planes with a depth step between them either join while a region grows (step < 50 mm) or fail can_be_merged as
segments too (step > 50 mm).  What merges is a HINGE: a step of more than 50 mm at the shared border, which blocks every directed
cell edge, and a small tilt back towards the first plane, which brings the second segment's centroid within 50 mm of the first
segment's plane and its normal within 18 degrees.

  strips(W, H, edges, planes)           vertical strips, constant over the image rows: strip k spans the columns [edges[k], edges[k+1])
                                        and shows the plane z = a X + c, planes[k] = (a, c); z(u) = c / (1 - a (u - cx) / fx) in float64,
                                        cast to float32
  hinge(prev, u_border, step, tilt)     the (a, c) of the strip behind the border: `step` mm nearer there, turned by `tilt` degrees
  lattice(W, H, rows, per_row, ..)      `rows` horizontal bands of `per_row` strips; even strips frontal, odd strips hinged to them
  cylinder_patch(depth, ..)             a vertical cylinder written over a rectangle of a frame
  classify(r, W)                        what the oracle's merge loop did on a frame, from its result alone (structural: no can_be_merged)

CASES names the frames the tests use; case(name) builds one (read-only, cached) and oracle(name, cylinders) runs the CPU oracle on it
once for the CPU test of these generators (tests/test_merge_cases.py) and for the GPU tests (tests/test_gpu_merge_planes.py).
Importing this file needs neither a GPU nor pytest.

Not among the cases: a merge whose refit is no longer planar.  576 two-strip hinges (first strip at 1.2, 2 and 3 m, steps of 60 to
200 mm, tilts of 3 to 17 degrees, the border at column 160, 320 and 480) gave none on the CPU oracle: whatever can_be_merged accepts
refits to a plane.
"""
import functools

import numpy as np

CELL = 20  # pixels per cell side (the reference's depthMapPatchSize)


def intrinsics(W):
    from cape_amd import synth

    return {k: v * (W / 640.0) for k, v in synth.DEFAULT_INTRINSICS.items()}


def strips(W, H, edges, planes, intr=None):
    intr = intr or intrinsics(W)
    assert len(edges) == len(planes) + 1 and edges[0] == 0 and edges[-1] == W
    u = np.arange(W, dtype=np.float64)
    z = np.zeros(W, np.float64)
    for u0, u1, (a, c) in zip(edges[:-1], edges[1:], planes):
        z[u0:u1] = c / (1.0 - a * (u[u0:u1] - intr["cx"]) / intr["fx"])
    return np.repeat(z[None, :], H, axis=0).astype(np.float32)


def hinge(prev, u_border, step, tilt, intr):
    """the plane behind the border column u_border: `step` mm in front of `prev` there, turned by `tilt` degrees about the vertical"""
    a0, c0 = prev
    k = (u_border - intr["cx"]) / intr["fx"]
    z0 = c0 / (1.0 - a0 * k) - step
    a = np.tan(np.arctan(a0) + np.radians(tilt))
    return (a, z0 * (1.0 - a * k))


def lattice(W, H, rows, per_row, base=1500.0, band=150.0, pair=300.0, step=55.0, tilt=4.0, flat=(), lean=(), intr=None):
    """`rows` bands; band j at base + band * j mm, cut into per_row strips (a multiple of 20 px wide: anything else destroys the
    merges).  Even strips are frontal at the band's depth, every second pair `pair` mm behind it; odd strips are
    hinge(previous, border, step, tilt) -- tilt 0 in the bands listed in `flat`, whose pairs stay connected and unmerged.
    lean[j], degrees, turns the even strips of band j (and the odd ones with them): a frontal strip is an exact plane in float32, its
    MSE next to zero, and is seeded before every hinged one; a leaning one is seeded among them."""
    intr = intr or intrinsics(W)
    assert W % per_row == 0 and (W // per_row) % CELL == 0 and H % rows == 0 and (H // rows) % CELL == 0
    sw, bh = W // per_row, H // rows
    edges = list(range(0, W + 1, sw))
    z = np.zeros((H, W), np.float32)
    for j in range(rows):
        planes = []
        for k in range(per_row):
            if k % 2 == 0:
                a = np.tan(np.radians(lean[j])) if j < len(lean) else 0.0
                z0 = base + band * j + pair * ((k // 2) % 2)  # (the depth at the strip's left border)
                planes.append((a, z0 * (1.0 - a * (edges[k] - intr["cx"]) / intr["fx"])))
            else:
                planes.append(hinge(planes[-1], edges[k], step, 0.0 if j in flat else tilt, intr))
        z[j * bh:(j + 1) * bh] = strips(W, bh, edges, planes, intr)
    return z


def cylinder_patch(depth, rows, cols, radius, nearest, intr):
    """Overwrite depth[rows, cols] with a cylinder of this radius whose axis is vertical, behind the middle column of the patch, and
    whose nearest point lies `nearest` mm from the camera plane.  Columns whose rays pass beside the cylinder get depth 0."""
    u = np.arange(cols.start, cols.stop, dtype=np.float64)
    mid = 0.5 * (cols.start + cols.stop)
    zc = nearest + radius
    xc = (mid - intr["cx"]) / intr["fx"] * zc
    x = (u - intr["cx"]) / intr["fx"]
    # |(z x - xc, z - zc)| = radius
    qa, qb, qc = x * x + 1.0, x * xc + zc, xc * xc + zc * zc - radius * radius
    disc = qb * qb - qa * qc
    z = np.where(disc >= 0.0, (qb - np.sqrt(np.maximum(disc, 0.0))) / qa, 0.0)
    depth[rows, cols] = z.astype(np.float32)[None, :]
    return depth


# ---- the classifier -------------------------------------------------------------------------------------------------------------------

def connectivity(plane_labels, W):
    """get_connected_components_matrix on the oracle's label grid: sources exclude the last row and the last column of cells, links go
    to the right and below.  (n, n) bool, symmetric."""
    grid = np.asarray(plane_labels).reshape(-1, W // CELL)
    n = int(grid.max()) if grid.size else 0
    conn = np.zeros((n, n), bool)
    src = grid[:-1, :-1]
    for other in (grid[:-1, 1:], grid[1:, :-1]):
        m = (src > 0) & (other > 0) & (src != other)
        conn[src[m] - 1, other[m] - 1] = True
        conn[other[m] - 1, src[m] - 1] = True
    return conn


def classify(r, W):
    """Counts of what merge_planes did on the frame of width W whose OracleResult is r, from r.plane_labels, r.merge_labels,
    r.segments[:, 19] and r.planes[:, 19] alone."""
    ml = np.asarray(r.merge_labels).astype(np.int64)
    n = len(ml)
    conn = connectivity(r.plane_labels, W)
    assert conn.shape == (n, n)
    ids = np.arange(n)
    absorbed = np.flatnonzero(ml != ids)
    per_root = np.bincount(ml[absorbed], minlength=n) if n else np.zeros(0, np.int64)
    upper = np.triu(conn, 1)
    i, j = np.nonzero(upper)
    out_roots = set(r.planes[:, 19].astype(int).tolist()) if len(r.planes) else set()
    planar = r.segments[:, 19] != 0 if n else np.zeros(0, bool)
    return dict(
        segments=n,
        merged=len(absorbed),
        multi=int((per_root >= 2).sum()),
        through_absorbed=int(sum(1 for c in absorbed if not conn[ml[c], c])),
        absorbed_row_with_later_link=int(sum(1 for row in absorbed if upper[row].any())),
        rejected=int((ml[i] != ml[j]).sum()),
        straddle64=int(sum(1 for c in absorbed if c >= 64 and ml[c] < 64)),
        root_ge64=int((per_root[64:] > 0).sum()),
        row63_link=int(n > 64 and conn[63, 64:].any()),
        dropped_roots=int(sum(1 for k in range(n) if ml[k] == k and planar[k] and k not in out_roots)),
        nonplanar_roots=int(sum(1 for k in range(n) if per_root[k] and not planar[k])),
    )


# ---- the named cases ------------------------------------------------------------------------------------------------------------------

SMALL, MID, BIG = (640, 480), (1280, 960), (1920, 1080)
_A = (0.0, 2000.0)      # the first strip of the small cases: frontal at 2 m
_THIRDS = [0, 220, 420, 640]


def _pair(W, H, I):
    """two strips, one merge"""
    return strips(W, H, [0, 320, 640], [_A, hinge(_A, 320, 55.0, 3.0, I)], I)


def _star(W, H, I):
    """the middle strip absorbs its left and its right neighbour: the second test uses the stale normal and d with grown sums"""
    return strips(W, H, _THIRDS, [hinge(_A, 220, 55.0, -5.0, I), _A, hinge(_A, 420, 55.0, 5.0, I)], I)


def _chain(W, H, I):
    """C touches only B, which A absorbed: the row of an absorbed segment expands its absorber (planeId = mergeLabels[row] != row)"""
    b = hinge(_A, 220, 55.0, 4.0, I)
    return strips(W, H, _THIRDS, [_A, b, hinge(b, 420, 55.0, 3.0, I)], I)


def _chain_reject(W, H, I):
    """merge labels [0, 1, 0]: one merge and one rejected connected pair in one frame"""
    b = hinge(_A, 220, 55.0, 4.0, I)
    return strips(W, H, _THIRDS, [_A, b, hinge(b, 420, 55.0, 12.0, I)], I)


def ring_cells(rect, V, Hc):
    """the cells of dilate(3 x 3) minus erode(cross, zero border) of the cell rectangle rect = (row0, row1, col0, col1)"""
    r0, r1, c0, c1 = rect
    inner = lambda r, c: r0 < r < r1 - 1 and c0 < c < c1 - 1 and 0 < r < V - 1 and 0 < c < Hc - 1  # noqa: E731
    return [(r, c) for r in range(max(r0 - 1, 0), min(r1 + 1, V)) for c in range(max(c0 - 1, 0), min(c1 + 1, Hc)) if not inner(r, c)]


# (cell rectangle of a merged pair of the 6 x 4 lattice, ring cells that keep their centre pixel)
MASKED_RING = [((8, 12, 0, 16), [(8, 0), (8, 12)]),             # two boundary points left: the plane is dropped
               ((16, 20, 16, 32), [(16, 16), (16, 17), (16, 28)])]  # three left: the plane is output, with exactly these


def _masked_ring(W, H, I):
    """The 6 x 4 lattice with the centre pixel (20 row + 10, 20 col + 10) of the ring cells of two merged pairs zeroed: all but two
    for the first pair, all but three for the second.  A hole on the centre pixel is skipped by both continuity scans, so every cell
    stays planar and the segments and merges are those of the lattice."""
    z = lattice(W, H, 6, 4, intr=I)
    for rect, kept in MASKED_RING:
        for r, c in ring_cells(rect, H // CELL, W // CELL):
            if (r, c) not in kept:
                z[CELL * r + CELL // 2, CELL * c + CELL // 2] = 0.0
    return z


def _lattice(rows, per_row, **kw):
    return lambda W, H, I: lattice(W, H, rows, per_row, intr=I, **kw)


def _lattice_cyl(radius):
    def make(W, H, I):
        return cylinder_patch(lattice(W, H, 6, 4, intr=I), slice(320, 480), slice(160, 480), radius, 1800.0, I)
    return make


# The leaning lattices were searched for on the CPU oracle: 200 random draws of lean[j] from {0, 0, 2, 3, -2, -3, 5, -5} per grid,
# the first draw kept that gave straddle64, root_ge64 and row63_link at once, the same with and without the cylinder branch.  The
# band depths and pair offsets alone (60 draws per grid of base, band and pair) never put a root beyond segment 63: every frontal
# strip is seeded before the first hinged one.
LEAN = {SMALL: (0, 0, 3, 3, -3, 3, 3, -2, -3, 3, 0, 0), MID: (3, 0, -3, 3, -3, 3, 2, -2, -5, 2, -3, 0), BIG: (0, 3, 0, 2, -2, -5, -5, 0, -3)}

# name: (grid, builder)
CASES = {
    "pair": (SMALL, _pair), "star": (SMALL, _star), "chain": (SMALL, _chain), "chain_reject": (SMALL, _chain_reject),
    "masked_ring": (SMALL, _masked_ring),
    "lattice_6x4": (SMALL, _lattice(6, 4)), "lattice_12x4": (SMALL, _lattice(12, 4)), "lattice_8x8": (SMALL, _lattice(8, 8)),
    "lattice_12x8": (SMALL, _lattice(12, 8)), "lattice_12x8_lean": (SMALL, _lattice(12, 8, lean=LEAN[SMALL])),
    "lattice_cyl_600": (SMALL, _lattice_cyl(600.0)), "lattice_cyl_900": (SMALL, _lattice_cyl(900.0)),
    "lattice_cyl_1400": (SMALL, _lattice_cyl(1400.0)),
    "mid_8x8": (MID, _lattice(8, 8)), "mid_12x8": (MID, _lattice(12, 8)), "mid_12x8_lean": (MID, _lattice(12, 8, lean=LEAN[MID])),
    "big_6x6": (BIG, _lattice(6, 6)), "big_9x8": (BIG, _lattice(9, 8)), "big_9x8_lean": (BIG, _lattice(9, 8, lean=LEAN[BIG])),
}

# (segments, merged, output planes) of every lattice, with and without the cylinder branch
LATTICE_COUNTS = {
    "lattice_6x4": (23, 11, 12), "lattice_12x4": (46, 22, 24), "lattice_8x8": (62, 30, 32), "lattice_12x8": (92, 44, 48),
    "mid_8x8": (62, 30, 32), "mid_12x8": (92, 44, 48), "big_6x6": (34, 16, 18), "big_9x8": (70, 34, 36),
    "lattice_12x8_lean": (92, 26, 66), "mid_12x8_lean": (94, 27, 67), "big_9x8_lean": (72, 19, 53),
}


def grid(name):
    return CASES[name][0]


@functools.lru_cache(maxsize=None)
def case(name):
    """(depth, intr) of a named case; the frame is cached and read-only"""
    (W, H), make = CASES[name]
    intr = intrinsics(W)
    depth = make(W, H, intr)
    assert depth.dtype == np.float32 and depth.shape == (H, W)
    depth.setflags(write=False)
    return depth, intr


@functools.lru_cache(maxsize=None)
def oracle(name, cylinders):
    """the CPU oracle's result for a named case, computed once"""
    import cape_oracle_py

    depth, intr = case(name)
    return cape_oracle_py.Oracle(depth.shape[1], depth.shape[0], cylinders=cylinders, **intr).run(depth)


@functools.lru_cache(maxsize=None)
def room(W, H, cylinders):
    """(depth, oracle result) of the ordinary frame the batches put around the cases"""
    import cape_oracle_py
    from cape_amd import synth

    intr = intrinsics(W)
    depth = synth.room(seed=1, frame=0, width=W, height=H, intr=intr)
    depth.setflags(write=False)
    return depth, cape_oracle_py.Oracle(W, H, cylinders=cylinders, **intr).run(depth)
