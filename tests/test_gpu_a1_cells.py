"""Stage A1's two instances -- one lane per cell (CAPE_A1=cells) and one lane per float4 column of a band (CAPE_A1=bands) --
leave the same bits.

Every case runs the same frames through both instances on the batch chain (CAPE_STAGE_A=bands, so that no handle takes the strip
kernel) and requires: every field of the cell statistics, the records (header status included) and both label grids equal bit
for bit between the two, and the lane-per-cell run equal to the oracle.  The cases are the inputs that steer A1 -- invalid
and non-finite pixels, the exactness guard, every step of both continuity scans, steps within an f32 ulp of the scan's
threshold (the per-step f64 form) -- and the grids at which the lane <-> cell map changes shape: one lane, a partial wave over
two cell rows, waves that start and end inside a cell row, one wave per cell row, the widest grid.
"""
import numpy as np
import pytest

from test_gpu_parity import _intr, _scan_boundary_frames, compare_frame
from test_gpu_scan_margin import _margin_frames

pytestmark = pytest.mark.gpu

CELL_FIELDS = ("sums", "point_count", "planar", "inorder", "tol", "bin", "normal", "d", "centroid", "mse", "score")


def _run(monkeypatch, a1, w, h, intr, frames, u16_scale=None):
    """-> (extractor, results, [cell_stats per frame]) of one instance; the caller closes the extractor"""
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_STAGE_A", "bands")
    monkeypatch.setenv("CAPE_A1", a1)
    ex = Extractor(w, h, cylinders=False, max_batch=max(9, len(frames)), **intr)
    n = ex.extract_host(frames) if u16_scale is None else ex.extract_host_u16(frames, u16_scale)
    assert n == len(frames)
    res = ex.results(n)
    return ex, res, [ex.cell_stats(f).copy() for f in range(n)]


def _check(monkeypatch, oracle_mod, w, h, intr, frames, u16_scale=None, no_cell_oracle=(), want_inorder=False):
    frames = np.ascontiguousarray(frames)
    depth = frames if u16_scale is None else frames.astype(np.float32) * np.float32(u16_scale)
    exb, resb, csb = _run(monkeypatch, "bands", w, h, intr, frames, u16_scale)
    exb.close()
    exc, resc, csc = _run(monkeypatch, "cells", w, h, intr, frames, u16_scale)
    try:
        for f in range(len(frames)):
            for name in CELL_FIELDS:
                assert csc[f][name].tobytes() == csb[f][name].tobytes(), f"frame {f}: cell_stats.{name} differs between the instances"
            if want_inorder:
                assert csc[f]["inorder"].sum() > 0 and csb[f]["inorder"].sum() > 0
        assert np.array_equal(resc.records["header"]["status"], resb.records["header"]["status"]), "header status"
        assert resc.records.tobytes() == resb.records.tobytes(), "records"
        assert np.array_equal(resc.plane_labels, resb.plane_labels), "plane label grids"
        assert np.array_equal(resc.cyl_labels, resb.cyl_labels), "cylinder label grids"
        orc = oracle_mod.Oracle(w, h, cylinders=False, **intr)
        for f in range(len(frames)):
            r = orc.run(depth[f])
            if f in no_cell_oracle:
                # (+inf is a valid depth for the reference: its sums are inf / NaN, compared as labels and counts)
                assert np.array_equal(csc[f]["point_count"], r.n) and np.array_equal(csc[f]["planar"], r.planar)
                assert np.array_equal(resc.plane_labels[f], r.plane_labels)
            else:
                compare_frame(r, exc, resc, f)
    finally:
        exc.close()


def _scene_frames():
    from cape_amd import synth

    # one intrinsics set per batch: the tumlike frame under the room's is still a scene
    return np.stack([synth.room(seed=3, frame=17), synth.tumlike(seed=2, frame=5), synth.tunnel(seed=4, frame=9)])


def _edge_frames():
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
    return np.stack([a, b, c, d])


def _sparse_invalid_frames():
    from cape_amd import synth

    rng = np.random.default_rng(19)
    base = synth.room(seed=8, frame=3)
    frames = []
    for value, density in ((-1200.0, 0.02), (-0.0, 0.05), (np.nan, 0.01), (np.inf, 0.004), (-np.inf, 0.01)):
        f = base.copy()
        mask = rng.random(f.shape) < density
        mask[:, 10::20] = False
        mask[10::20, :] = False
        f[mask] = value
        frames.append(f)
    mixed = base.copy()
    for value in (-3.0, -0.0, np.nan):
        m = rng.random(mixed.shape) < 0.01
        m[:, 10::20] = False
        m[10::20, :] = False
        mixed[m] = value
    frames.append(mixed)
    return np.stack(frames).astype(np.float32)


def test_scene_frames(oracle_mod, monkeypatch):
    _check(monkeypatch, oracle_mod, 640, 480, _intr("room"), _scene_frames())


def test_edge_inputs(oracle_mod, monkeypatch):
    """NaN, negatives, huge depths, 35 % holes, a constant frame, a discontinuity in every cell"""
    _check(monkeypatch, oracle_mod, 640, 480, _intr("tumlike"), _edge_frames())


def test_sparse_invalid_patterns(oracle_mod, monkeypatch):
    """negatives, -0, NaN, +-inf sprinkled over cells that stay valid: the range guard sends them to the in-order pass"""
    _check(monkeypatch, oracle_mod, 640, 480, _intr("room"), _sparse_invalid_frames(), no_cell_oracle=(3,))


def test_inorder_guard(oracle_mod, monkeypatch):
    """near-zero column factors: the exactness guard rejects cells on their ratio alone, in both instances"""
    from cape_amd import synth

    intr = dict(fx=550.0, fy=550.0, cx=320.0000001, cy=240.0000001)
    frames = np.stack([synth.room(seed=9, frame=3), synth.room(seed=9, frame=4)])
    _check(monkeypatch, oracle_mod, 640, 480, intr, frames, want_inorder=True)


def test_scan_boundary_steps(oracle_mod, monkeypatch):
    """jumps and holes on the seeds, the first, the last and the ignored step of both scans"""
    _check(monkeypatch, oracle_mod, 640, 480, _intr("room"), _scan_boundary_frames())


def test_scan_steps_within_an_ulp_of_the_threshold(oracle_mod, monkeypatch):
    """one step per cell at, one f32 ulp below and one above 4 dq(z): f32 cannot call them, the wave redoes the step in f64"""
    frames, verdicts = _margin_frames()
    assert 0.25 < verdicts.mean() < 0.75
    _check(monkeypatch, oracle_mod, 640, 480, _intr("room"), frames)


# width, height: cells per row x rows -- what the lane <-> cell map does there
GRIDS = [
    (20, 20),     # 1 cell: one lane
    (60, 40),     # 3 x 2: one partial wave over two cell rows
    (660, 40),    # 33 x 2: wave 0 ends at lane 30 of cell row 1, wave 1 holds two cells
    (1300, 20),   # 65 x 1: the second wave holds one lane
    (1280, 60),   # 64 x 3: one wave per cell row
    (5120, 20),   # 256 x 1: the widest grid cape_create accepts
]


def _grid_frames(w, h, intr):
    """three distinct frames, so that a wrong frame offset shows"""
    from cape_amd import synth

    frames = np.stack([synth.facets(seed=21, frame=1, width=w, height=h, intr=intr),
                       synth.tunnel(seed=5, frame=2, width=w, height=h, intr=intr),
                       synth.facets(seed=4, frame=6, width=w, height=h, intr=intr)]).astype(np.float32)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], frames[2])
    return frames


def _grid_intr(w, h):
    s = max(w, h) / 640.0
    return dict(fx=550.0 * s, fy=550.0 * s, cx=w / 2.0 + 0.25, cy=h / 2.0 - 0.5)


@pytest.mark.parametrize("w,h", GRIDS)
def test_grid_shapes(oracle_mod, monkeypatch, w, h):
    intr = _grid_intr(w, h)
    _check(monkeypatch, oracle_mod, w, h, intr, _grid_frames(w, h, intr))


def _to_raw(depth):
    """raw sensor units of 1/5 mm, as the datasets' PNG payload"""
    return np.clip(np.rint(np.nan_to_num(depth.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * 5.0), 0, 65535).astype(np.uint16)


def test_uint16_scene_frames(oracle_mod, monkeypatch):
    from cape_amd import synth

    raw = _to_raw(np.stack([synth.room(seed=3, frame=17), synth.tumlike(seed=2, frame=5)]))
    _check(monkeypatch, oracle_mod, 640, 480, _intr("tumlike"), raw, u16_scale=0.2)


def test_uint16_grid_660x40(oracle_mod, monkeypatch):
    intr = _grid_intr(660, 40)
    _check(monkeypatch, oracle_mod, 660, 40, intr, _to_raw(_grid_frames(660, 40, intr)), u16_scale=0.2)


def test_unknown_instance_is_an_error(monkeypatch):
    """CAPE_A1 is validated at cape_create like the other knobs: a value it does not know is an error, not a default"""
    from cape_amd import Extractor

    monkeypatch.setenv("CAPE_A1", "lanes")
    with pytest.raises(Exception, match="CAPE_A1"):
        Extractor(640, 480, cylinders=False, max_batch=16, **_intr("room"))
