"""The continuity cross scan at its threshold: |z - last| against 4 * depth_quantization(z) (plane_segment.cpp:44-60).

The streaming kernel decides a scan step in f32 where f32 can decide it and falls back to the reference's f64 form inside a
margin around the threshold (cape_cell_acc.h: is_continuous_flat_f32).  These frames put one step of the centre row or of the
centre column of every cell AT the threshold (the farthest float32 depth that still passes), one float32 ulp below it and one
ulp above it, over the depth range of the scenes (0.5 .. 8 m), with zero and NaN samples in front of the step in some cells.
Every cell is a constant-depth patch with a one-pixel dent towards the camera, so the step INTO the dent sits at the threshold
and the step out of it passes with room (the tolerance grows with depth): the cell's planar flag follows the scan's verdict.
"""
import numpy as np
import pytest

from test_gpu_parity import _intr, compare_frame

CELL = 20
SIGMA_ERROR = 2.73 * ((1.0 / 1000.0) * (1.0 / 1000.0))
SIGMA_MULTIPLIER = 0.74 / 1000.0
SIGMA_MARGIN = -0.53


def _threshold(z):
    """4 * utils::get_depth_quantization(z) in the reference's f64 operation order"""
    d = float(z)
    q = SIGMA_MARGIN + SIGMA_MULTIPLIER * d + SIGMA_ERROR * (d * d)
    return 4.0 * (0.5 if q < 0.5 else q)


def _close(z, last):
    return float(np.abs(np.float32(z) - np.float32(last))) <= _threshold(z)


def _scan(samples):
    """is_cell_horizontal_continuous / is_cell_vertical_continuous over the samples the scan visits"""
    last = samples[1] if samples[0] < samples[1] else samples[0]
    if last <= 0:
        return False
    for z in samples[1:]:
        if z > 0:
            if not _close(z, last):
                return False
            last = z
    return True


def _cell_continuous(cell):
    return _scan([cell[10, c] for c in range(20)]) and _scan([cell[r, 10] for r in range(19)])


def _farthest_passing(zc):
    """the smallest float32 depth below zc whose step from zc still passes (positive floats order like their bit patterns)"""
    lo = np.float32(zc - 1.5 * _threshold(zc)).view(np.uint32)  # fails: the tolerance only shrinks towards the camera
    hi = np.float32(zc).view(np.uint32)                         # passes
    assert not _close(lo.view(np.float32), zc) and _close(hi.view(np.float32), zc)
    while hi - lo > 1:
        mid = np.uint32((int(lo) + int(hi)) // 2)
        if _close(mid.view(np.float32), zc):
            hi = mid
        else:
            lo = mid
    return hi


def _margin_frames(n_frames=3):
    frames, designed = [], []
    for f in range(n_frames):
        img = np.zeros((480, 640), np.float32)
        verdicts = np.zeros((24, 32), bool)
        for cy in range(24):
            for cx in range(32):
                i = cy * 32 + cx
                zc = np.float32(500.0 + 7500.0 * ((i * 37 + f * 11) % 768) / 767.0 + 0.37)
                at = _farthest_passing(zc)
                side = (i + f) % 3                      # 0: one ulp below the threshold, 1: at it, 2: one ulp above
                dent = np.uint32(int(at) + 1 - side).view(np.float32)
                cell = np.full((CELL, CELL), zc, np.float32)
                vertical = (i // 3 + f) % 2 == 1
                steps = [s for s in range(3, 19 if vertical else 20) if s not in (10, 11)]
                k = steps[(i // 6 + 5 * f) % len(steps)]
                r, c = (k, 10) if vertical else (10, k)
                cell[r, c] = dent
                if i % 7 == 3:                          # a hole in front of the step: `last` is carried over it
                    cell[(r - 1, c) if vertical else (r, c - 1)] = 0.0
                if i % 11 == 5:                         # a NaN sample there: not positive, the step passes
                    cell[(r - 1, c) if vertical else (r, c - 1)] = np.nan
                img[cy * CELL:(cy + 1) * CELL, cx * CELL:(cx + 1) * CELL] = cell
                verdicts[cy, cx] = _cell_continuous(cell)
                assert verdicts[cy, cx] == (side != 2), "the designed step decides the cell"
        frames.append(img)
        designed.append(verdicts)
    return np.stack(frames), np.stack(designed)


def test_margin_frames_have_mixed_verdicts(oracle_mod):
    """No GPU: the inputs sit where they are meant to, and the oracle's cell flags follow the scan's verdict on them."""
    frames, verdicts = _margin_frames(1)
    assert 0.25 < verdicts.mean() < 0.75, "verdicts are mixed"
    assert np.isnan(frames).any() and (frames == 0).any()
    orc = oracle_mod.Oracle(640, 480, cylinders=False, **_intr("room"))
    ref = orc.run(frames[0])
    planar = np.asarray(ref.planar).reshape(24, 32).astype(bool)
    assert np.array_equal(planar, verdicts[0]), "on these frames the oracle's planar flag is the scan's verdict"


@pytest.mark.gpu
@pytest.mark.parametrize("u16", [False, True])
def test_scan_margin_against_oracle(oracle_mod, u16):
    """Cell flags, sums and labels of the batch kernels against the oracle on the threshold frames."""
    from cape_amd import Extractor

    frames, verdicts = _margin_frames()
    intr = _intr("room")
    if u16:
        # raw sensor units: 1/5 mm steps cannot sit one float32 ulp from a threshold, but they put the steps of every cell
        # within a unit of it -- on both sides, for the uint16 launch of the same kernel
        raw = np.nan_to_num(frames * 5.0, nan=0.0).round().astype(np.uint16)
        frames = raw.astype(np.float32) * np.float32(0.2)
    orc = oracle_mod.Oracle(640, 480, cylinders=False, **intr)
    refs = [orc.run(f) for f in frames]
    planar = np.stack([np.asarray(r.planar).reshape(24, 32).astype(bool) for r in refs])
    assert planar.any() and not planar.all()
    if not u16:
        assert np.array_equal(planar, verdicts), "the planar flag is the scan's verdict"
    ex = Extractor(640, 480, cylinders=False, max_batch=16, **intr)
    if u16:
        n = ex.extract_host_u16(raw, 0.2)
    else:
        n = ex.extract_host(frames)
    res = ex.results(n)
    for i in range(n):
        compare_frame(refs[i], ex, res, i)
    ex.close()
