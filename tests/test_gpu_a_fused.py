"""Stage A in one launch -- the lanes of A1 fit their cells' planes (CAPE_A2=fused) -- leaves the same bits as A1 and A2 as two
kernels (CAPE_A2=split).

Every eligible-grid case runs the same frames through both forms on the batch chain (CAPE_STAGE_A=bands, so that no handle takes
the strip kernel) and requires: every field of the cell statistics, the records (header status included) and both label grids equal
bit for bit between the two, and the fused run equal to the oracle.  CAPE_A2=fused refuses a handle it cannot serve, so a case
that creates one knows which kernel ran.  The cases are the inputs that steer the fit (invalid pixels, the in-order redo, cleared
cells next to planar ones, the scans' margins), the batch sizes at which the workgroup -> frame map matters, and the grids at which
a workgroup's tile changes shape: 16, 8, 4 and 1 cell rows per tile.  Grids whose workgroups are not whole tiles keep the split
kernels.
"""
import numpy as np
import pytest

from test_gpu_parity import _intr, _scan_boundary_frames, compare_frame
from test_gpu_scan_margin import _margin_frames

pytestmark = pytest.mark.gpu

CELL_FIELDS = ("sums", "point_count", "planar", "inorder", "tol", "bin", "normal", "d", "centroid", "mse", "score")


def _run(monkeypatch, a2, w, h, intr, frames, u16_scale=None, max_batch=None):
    """-> (extractor, results, [cell_stats per frame]) of one form; the caller closes the extractor"""
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_STAGE_A", "bands")
    if a2 is None:
        monkeypatch.delenv("CAPE_A2", raising=False)
    else:
        monkeypatch.setenv("CAPE_A2", a2)
    ex = Extractor(w, h, cylinders=False, max_batch=max_batch or max(9, len(frames)), **intr)
    n = ex.extract_host(frames) if u16_scale is None else ex.extract_host_u16(frames, u16_scale)
    assert n == len(frames)
    res = ex.results(n)
    return ex, res, [ex.cell_stats(f).copy() for f in range(n)]


def _check(monkeypatch, oracle_mod, w, h, intr, frames, u16_scale=None, want_inorder=False, max_batch=None):
    """-> the fused run's cell statistics"""
    frames = np.ascontiguousarray(frames)
    depth = frames if u16_scale is None else frames.astype(np.float32) * np.float32(u16_scale)
    exs, ress, css = _run(monkeypatch, "split", w, h, intr, frames, u16_scale, max_batch)
    exs.close()
    exf, resf, csf = _run(monkeypatch, "fused", w, h, intr, frames, u16_scale, max_batch)
    try:
        for f in range(len(frames)):
            for name in CELL_FIELDS:
                assert csf[f][name].tobytes() == css[f][name].tobytes(), f"frame {f}: cell_stats.{name} differs between fused and split"
            if want_inorder:
                assert csf[f]["inorder"].sum() > 0 and css[f]["inorder"].sum() > 0
        assert np.array_equal(resf.records["header"]["status"], ress.records["header"]["status"]), "header status"
        assert resf.records.tobytes() == ress.records.tobytes(), "records"
        assert np.array_equal(resf.plane_labels, ress.plane_labels), "plane label grids"
        assert np.array_equal(resf.cyl_labels, ress.cyl_labels), "cylinder label grids"
        orc = oracle_mod.Oracle(w, h, cylinders=False, **intr)
        for f in range(len(frames)):
            compare_frame(orc.run(depth[f]), exf, resf, f)
    finally:
        exf.close()
    return csf


def _both_batches(monkeypatch, oracle_mod, intr, frames, single, **kw):
    """the batch (15 workgroups for five frames: the workgroup -> frame map) and frame `single` alone on a one-frame handle"""
    _check(monkeypatch, oracle_mod, 640, 480, intr, frames, **kw)
    _check(monkeypatch, oracle_mod, 640, 480, intr, frames[single:single + 1], max_batch=1, **kw)


def _scene_frames():
    from cape_amd import synth

    return np.stack([synth.room(seed=3, frame=17), synth.tumlike(seed=2, frame=5), synth.tunnel(seed=4, frame=9),
                     synth.room(seed=6, frame=2), synth.tunnel(seed=1, frame=30)])


def _edge_frames():
    """the edge frames of test_gpu_a1_cells.py -- 35 % holes; NaN, negatives and 65535; a flat wall; stripes -- and a scene behind them"""
    from cape_amd import synth

    rng = np.random.default_rng(7)
    base = synth.tumlike(seed=3, frame=1)
    a = base.copy()
    a[rng.random(a.shape) < 0.35] = 0.0
    b = base.copy()
    b[100:140, 200:260] = np.nan
    b[300:330, 50:90] = -5.0
    b[10:12, :] = 65535.0
    c = np.full_like(base, 1500.0)
    d = base.copy()
    d[:, ::2] *= 1.6
    return np.stack([a, b, c, d, base])


def _to_raw(depth):
    """raw sensor units of 1/5 mm, as the datasets' PNG payload"""
    return np.clip(np.rint(np.nan_to_num(depth.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * 5.0), 0, 65535).astype(np.uint16)


INORDER_INTR = dict(fx=550.0, fy=550.0, cx=320.0000001, cy=240.0000001)  # near-zero column factors: the guard rejects cells on their ratio


def test_scene_frames(oracle_mod, monkeypatch):
    _both_batches(monkeypatch, oracle_mod, _intr("room"), _scene_frames(), single=0)


def test_edge_inputs(oracle_mod, monkeypatch):
    _both_batches(monkeypatch, oracle_mod, _intr("tumlike"), _edge_frames(), single=1)


def test_inorder_cells(oracle_mod, monkeypatch):
    """cells the exactness guard rejects are redone in pixel order by the lane that summed them, ahead of the barrier"""
    from cape_amd import synth

    frames = np.stack([synth.room(seed=9, frame=k) for k in (3, 4, 5, 6, 7)])
    _both_batches(monkeypatch, oracle_mod, INORDER_INTR, frames, single=1, want_inorder=True)


def test_scan_margin_frames(oracle_mod, monkeypatch):
    frames, verdicts = _margin_frames()
    assert 0.25 < verdicts.mean() < 0.75
    frames = np.concatenate([frames, _scan_boundary_frames()[:2]])
    assert len(frames) == 5
    _both_batches(monkeypatch, oracle_mod, _intr("room"), frames, single=2)


def test_uint16_frames(oracle_mod, monkeypatch):
    raw = _to_raw(np.concatenate([_scene_frames()[:2], _edge_frames()[:3]]))
    _both_batches(monkeypatch, oracle_mod, _intr("tumlike"), raw, single=3, u16_scale=0.2)


def test_uint16_inorder_cells(oracle_mod, monkeypatch):
    from cape_amd import synth

    raw = _to_raw(np.stack([synth.room(seed=9, frame=3), synth.room(seed=9, frame=4)]))
    _both_batches(monkeypatch, oracle_mod, INORDER_INTR, raw, single=0, u16_scale=0.2, want_inorder=True)


def test_cleared_tiles(oracle_mod, monkeypatch):
    """A workgroup's tile at 640x480 is 8 cell rows.  Whole tiles of cleared cells -- no points, fewer than half the points,
    discontinuous -- beside tiles of planar ones, and cleared blocks inside a tile: the sums go out as zeros, once, and the
    planar neighbours' edge predicates read the cleared planes."""
    from cape_amd import synth

    wall = synth.room(seed=3, frame=17).astype(np.float32)
    rng = np.random.default_rng(11)
    empty = wall.copy()
    empty[160:320, :] = 0.0                       # tile 1: no points at all
    sparse = wall.copy()
    sparse[0:160, :][rng.random((160, 640)) < 0.6] = 0.0  # tile 0: fewer than half the points
    striped = wall.copy()
    striped[320:480, ::2] *= 1.6                  # tile 2: a discontinuity on every scan step
    inside = wall.copy()
    inside[80:240, 160:480] = 0.0                 # cell rows 4..11 x columns 8..23: cleared cells with planar neighbours in both tiles
    frames = np.stack([empty, sparse, striped, inside])
    cs = _check(monkeypatch, oracle_mod, 640, 480, _intr("room"), frames)
    grid = lambda f, name: cs[f][name].reshape(24, 32, *cs[f][name].shape[1:])
    for f, rows in ((0, slice(8, 16)), (1, slice(0, 8)), (2, slice(16, 24))):
        assert not grid(f, "planar")[rows].any() and not grid(f, "point_count")[rows].any() and not grid(f, "sums")[rows].any()
        others = np.ones(24, bool)
        others[rows] = False
        assert grid(f, "planar")[others].sum() > 64, "the neighbouring tiles hold planar cells"
    assert not grid(3, "point_count")[4:12, 8:24].any() and grid(3, "planar")[4:12, :8].any() and grid(3, "planar")[:4, 8:24].any()


# width, height: cells per row x rows -- the workgroup's tile there
ELIGIBLE_GRIDS = [
    (320, 320),   # 16 x 16: one tile per frame, 16 rows per tile
    (160, 640),   # 8 x 32: one tile per frame, 32 rows: most edges are vertical and inside the tile
    (1280, 960),  # 64 x 48: 4 rows per tile, 12 tiles
    (5120, 20),   # 256 x 1: the widest grid cape_create accepts; one row per tile, every vertical edge left to stage B
]
INELIGIBLE_GRIDS = [
    (320, 240),   # 16 x 12 = 192 cells: a frame is not whole workgroups
    (660, 480),   # 33 cells wide: a workgroup is not whole cell rows
    (1300, 20),   # 65 x 1
]


def _grid_frames(w, h, intr):
    from cape_amd import synth

    frames = np.stack([synth.facets(seed=21, frame=1, width=w, height=h, intr=intr),
                       synth.tunnel(seed=5, frame=2, width=w, height=h, intr=intr)]).astype(np.float32)
    assert not np.array_equal(frames[0], frames[1])
    return frames


def _grid_intr(w, h):
    s = max(w, h) / 640.0
    return dict(fx=550.0 * s, fy=550.0 * s, cx=w / 2.0 + 0.25, cy=h / 2.0 - 0.5)


@pytest.mark.parametrize("w,h", ELIGIBLE_GRIDS)
def test_eligible_grid_shapes(oracle_mod, monkeypatch, w, h):
    intr = _grid_intr(w, h)
    _check(monkeypatch, oracle_mod, w, h, intr, _grid_frames(w, h, intr))


@pytest.mark.parametrize("w,h", INELIGIBLE_GRIDS)
def test_ineligible_grids_keep_the_split_kernels(oracle_mod, monkeypatch, w, h):
    from cape_amd import Extractor

    intr = _grid_intr(w, h)
    monkeypatch.setenv("CAPE_STAGE_A", "bands")
    monkeypatch.setenv("CAPE_A2", "fused")
    with pytest.raises(Exception, match=r"\(-1\).*CAPE_A2=fused"):  # CAPE_ERR_INVALID_ARGUMENT
        Extractor(w, h, cylinders=False, max_batch=9, **intr)
    frames = _grid_frames(w, h, intr)
    ex, res, _ = _run(monkeypatch, None, w, h, intr, frames)
    try:
        orc = oracle_mod.Oracle(w, h, cylinders=False, **intr)
        for f in range(len(frames)):
            compare_frame(orc.run(frames[f]), ex, res, f)
    finally:
        ex.close()


def test_band_instance_implies_split(oracle_mod, monkeypatch):
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_A1", "bands")
    frames = _scene_frames()[:2]
    ex, res, _ = _run(monkeypatch, None, 640, 480, _intr("room"), frames)
    try:
        orc = oracle_mod.Oracle(640, 480, cylinders=False, **_intr("room"))
        for f in range(len(frames)):
            compare_frame(orc.run(frames[f]), ex, res, f)
    finally:
        ex.close()
    monkeypatch.setenv("CAPE_A2", "fused")
    with pytest.raises(Exception, match=r"\(-1\).*CAPE_A2=fused"):
        Extractor(640, 480, cylinders=False, max_batch=9, **_intr("room"))


def test_unknown_form_is_an_error(monkeypatch):
    """CAPE_A2 is validated at cape_create like the other knobs: a value it does not know is an error, not a default"""
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_A2", "bogus")
    with pytest.raises(Exception, match="CAPE_A2"):
        Extractor(640, 480, cylinders=False, max_batch=16, **_intr("room"))
