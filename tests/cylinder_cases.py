"""Depth frames that take cylinder_fitting to its cell-count edges and down its RANSAC branches, shared by the CPU test
(test_cylinder_cases.py: does the oracle's trace reach the edges each case claims) and the GPU test (test_gpu_cylinder_edges.py: is every
route of the device equal to the oracle on them).  numpy only; nothing here loads a library.

A case is (name, width, height, intrinsics scale, builder, edges): the builder returns the float32 depth frame, the intrinsics are
synth.DEFAULT_INTRINSICS times the scale, and `edges` are the names of REQUIRED (below) the case claims to reach.  `reached()` turns
an OracleResult's cyl_candidates / cyl_loops into the set of edge names the frame did reach.

Family A -- sizes.  Cell-aligned windows of synth.tunnel: the grown region is the window, so the one candidate has exactly N cells.
Up to 257 cells the windows are strips of the plain frame's left wall, two or more rows high (flatter or lower windows grow into a
plane, score > 100); from 383 cells on they are windows of the `vault`, the same tunnel rendered with the principal point below the
image, which has neither the floor chord nor pixels beyond the sensor range.  Odd sizes are a rectangle plus a partial row.  One
candidate, two wins, early stop, one cylinder label: what the tunnel scenes of the suite reach, at every N where a loop of the three
device implementations changes shape.

Family B -- branches.  Corrugated sheets, depth = z0 + A * w(u / P + tilt * v / P) with w a C1 wave of parabolic arcs (`arcs`) or
Bhaskara's rational stand-in for the sine (`bhaskara`), whole grid or windowed: ridges of different curvature that one cylinder
hypothesis cannot hold together, so the outer `while` runs many passes, hypotheses keep winning late, and planes compete.  Narrow
windows of a sheet fall apart into several small candidates: early stops at every depth, `best < 6`, the minimumCellActivated exit.

Unreachable edges: none.  Every name of REQUIRED is claimed by a case and confirmed by test_cylinder_cases.py (UNREACHABLE is empty).
Two readings the table fixes: "ended by minimumCellActivated" means the 10 % rule alone would have gone on (cells left > 10 % of N),
and the plane segments "beside" six cylinder labels count whether they were grown as planes or won inside a candidate.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name width height scale build edges")

CELL = 20
# kCylEnd* of oracle/cape_oracle.hpp
END_SCORE_GATE, END_MINIMUM_CELLS, END_TEN_PERCENT, END_BEST_UNDER_SIX = 0, 1, 2, 3
MAX_ITERATIONS = 43

A_SIZES_640 = (6, 7, 8, 31, 32, 33, 35, 36, 37, 63, 64, 65, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768)
A_SIZES_1280 = (769, 1535, 1536, 1537, 2305)
FIRST_M = (384, 385, 768, 769, 1536, 1537)

# every edge the table as a whole has to reach (the issue's list); "N=<n>" edges of family A are added below
REQUIRED = {
    "wins=1", "wins=2", "wins>=3", "wins>=6",
    "all 43 iterations, no stop",
    "stop at 2", "stop in 3..16", "stop in 17..42",
    "win at >=33",
    "sub-segments=2", "sub-segments>=4", "sub-segments>=8",
    "plane and cylinder win in one candidate",
    "best<6 break",
    "ended by minimumCellActivated",
    "candidates>=3",
    "cylinder labels>=6 beside plane segments>=2",
    "m steps across 768", "m steps across 384", "m steps across 64",
    "320x240 under one cache pass",
    "noisy sheet",
} | {"multi-pass first m=%d" % m for m in FIRST_M} | {"N=%d" % n for n in A_SIZES_640 + A_SIZES_1280}

# edges no case reaches, name -> what was tried (kept in step with the module docstring)
UNREACHABLE = {}


def intrinsics(case):
    from cape_amd import synth

    return {k: v * case.scale for k, v in synth.DEFAULT_INTRINSICS.items()}


# ---- what a frame reached --------------------------------------------------------------------------------------------------------

def reached(case, result):
    """The names of REQUIRED that `result` (an OracleResult with the cylinder trace) reaches on `case`."""
    got = set()
    cands, loops = result.cyl_candidates, result.cyl_loops
    for lp in loops:
        if lp.iterations == 0:
            continue
        got.add("wins=1" if lp.wins == 1 else "wins=2" if lp.wins == 2 else "wins>=3")
        if lp.wins >= 6:
            got.add("wins>=6")
        if lp.iterations == MAX_ITERATIONS and not lp.early_stop:
            got.add("all 43 iterations, no stop")
        if lp.early_stop:
            it = lp.iterations
            got.add("stop at 2" if it == 2 else "stop in 3..16" if it <= 16 else "stop in 17..42" if it <= 42 else "stop at 43")
        if any(w >= 33 for w in lp.win_iterations):
            got.add("win at >=33")
        if lp.best < 6:
            got.add("best<6 break")
    for k, c in enumerate(cands):
        mine = [lp for lp in loops if lp.candidate == k]
        if c.segments == 2:
            got.add("sub-segments=2")
        if c.segments >= 4:
            got.add("sub-segments>=4")
        if c.segments >= 8:
            got.add("sub-segments>=8")
        if any(c.plane_won) and not all(c.plane_won):
            got.add("plane and cylinder win in one candidate")
        left = c.n - sum(c.inliers)
        if c.score_passed and c.end == END_MINIMUM_CELLS and left > 0.1 * c.n:  # (the 10 % rule alone would have gone on)
            got.add("ended by minimumCellActivated")
        ms = [lp.m for lp in mine]
        for a, b in zip(ms, ms[1:]):
            for edge in (768, 384, 64):
                if a > edge >= b:
                    got.add("m steps across %d" % edge)
        if len(mine) >= 2 and c.segments >= 2 and ms[0] in FIRST_M:
            got.add("multi-pass first m=%d" % ms[0])
        if (case.width, case.height) == (320, 240) and c.score_passed and c.n == 192 and c.segments >= 2:
            got.add("320x240 under one cache pass")
    if len(cands) >= 3:
        got.add("candidates>=3")
    if int(result.cyl_labels.max()) >= 6 and len(result.segments) >= 2:  # (plane segments of either origin: grown, or won in a candidate)
        got.add("cylinder labels>=6 beside plane segments>=2")
    if case.name.startswith("A ") and len(cands) == 1 and cands[0].score_passed:
        got.add("N=%d" % cands[0].n)
    if "noisy" in case.name and any(c.segments >= 2 for c in cands):
        got.add("noisy sheet")
    return got


# ---- builders --------------------------------------------------------------------------------------------------------------------

def window(depth, x0, y0, cols, rows, extra=0):
    """`depth` with everything zeroed but the cells [x0, x0 + cols) x [y0, y0 + rows) and the first `extra` cells of the next row."""
    keep = np.zeros(depth.shape, bool)
    keep[y0 * CELL:(y0 + rows) * CELL, x0 * CELL:(x0 + cols) * CELL] = True
    keep[(y0 + rows) * CELL:(y0 + rows + 1) * CELL, x0 * CELL:(x0 + extra) * CELL] = True
    return np.where(keep, depth, np.float32(0))


@functools.lru_cache(maxsize=None)
def tunnel(width, seed, frame, vault=False):
    """synth.tunnel (read-only); vault=True: seen with the principal point 1.5 image heights down, the tunnel's vault over the whole frame."""
    from cape_amd import synth

    s = width / 640.0
    intr = dict(fx=550.0 * s, fy=550.0 * s, cx=320.0 * s, cy=720.0 * s) if vault else None
    d = synth.tunnel(seed=seed, frame=frame, width=width, height=width * 3 // 4, intr=intr)
    d.setflags(write=False)
    return d


def vault_window(width, n, cols, seed=0, frame=0, x0=0, y0=0):
    return lambda: window(tunnel(width, seed, frame, vault=True), x0, y0, cols, n // cols, n % cols)


def tunnel_window(width, n, cols, seed=0, frame=0, x0=0, y0=0):
    return lambda: window(tunnel(width, seed, frame), x0, y0, cols, n // cols, n % cols)


def arcs(x):
    """C1 wave of period 1 in [-1, 1] made of parabolic arcs."""
    f = x - np.floor(x)
    up = 1.0 - 16.0 * (f - 0.25) * (f - 0.25)
    down = 16.0 * (f - 0.75) * (f - 0.75) - 1.0
    return np.where(f < 0.5, up, down)


def bhaskara(x):
    """Bhaskara I's rational approximation of sin(2 pi x): flatter flanks than `arcs`, no libm call."""
    f = x - np.floor(x)
    h = np.where(f < 0.5, f, f - 0.5) * 2.0  # half-period phase in [0, 1)
    q = h * (1.0 - h)
    s = 16.0 * q / (5.0 - 4.0 * q)
    return np.where(f < 0.5, s, -s)


def sheet(width, height, z0, amp, period, tilt=0.0, wave=arcs, sigma=0.0, seed=0):
    """Corrugated sheet in millimetres; sigma > 0 adds seeded Gaussian noise."""
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    z = z0 + amp * wave(u / period + tilt * v / period)
    if sigma:
        z = z + sigma * np.random.default_rng(seed).standard_normal(z.shape)
    return z.astype(np.float32)


def sheet_case(width, height, window_spec=None, **kw):
    def build():
        z = sheet(width, height, **kw)
        return window(z, *window_spec) if window_spec else z
    return build


def islands(width, height, specs, **kw):
    """Several windows of one sheet in one frame: one candidate (or plane) per island."""
    def build():
        z = sheet(width, height, **kw)
        out = np.zeros_like(z)
        for spec in specs:
            out = np.maximum(out, window(z, *spec))
        return out
    return build


# ---- the table -------------------------------------------------------------------------------------------------------------------

def _a_cases():
    # Small windows are planes (score > 100) unless they are strips along the strongly curved left wall of the plain tunnel frame;
    # from 383 cells on the window needs the vault, which has no floor chord.  Positions and seeds found with the oracle's trace.
    out = []
    for n in A_SIZES_640:
        if n <= 8:
            build = tunnel_window(640, n, 3, x0=5, y0=14) if n == 6 else tunnel_window(640, n, 2, x0=7, y0=2)
        elif n <= 257:
            build = tunnel_window(640, n, 2 if n <= 37 else 3 if n <= 65 else 24 if n <= 193 else 32)
        else:
            build = vault_window(640, n, 32)
        out.append(Case("A 640 N=%d" % n, 640, 480, 1.0, build, {"N=%d" % n}))
    for n in A_SIZES_1280:
        build = tunnel_window(1280, n, 64) if n == 769 else vault_window(1280, n, 64, seed=4)
        out.append(Case("A 1280 N=%d" % n, 1280, 960, 2.0, build, {"N=%d" % n}))
    return out


# what every sheet reaches: loops that run all 43 iterations with three, and six, winning hypotheses, the last of them late
_SHEET = {"all 43 iterations, no stop", "win at >=33", "wins>=3", "wins>=6"}
_WINDOW = _SHEET | {"plane and cylinder win in one candidate", "sub-segments>=4", "sub-segments>=8"}
B_EDGES = {
    "B 640 flat sheet": _SHEET | {"m steps across 384", "multi-pass first m=768", "sub-segments>=4", "wins=1"},
    "B 640 tilted sheet": _SHEET | {"m steps across 384", "multi-pass first m=768", "sub-segments>=4", "sub-segments>=8", "wins=1", "wins=2"},
    "B 640 tilted bhaskara sheet": _SHEET | {"m steps across 384", "multi-pass first m=768", "plane and cylinder win in one candidate",
                                             "sub-segments>=4"},
    "B 640 noisy tilted sheet": _SHEET | {"m steps across 384", "multi-pass first m=768", "noisy sheet", "sub-segments>=4", "sub-segments>=8",
                                          "wins=2"},
    "B 640 sheet window 384": _WINDOW | {"m steps across 64", "multi-pass first m=384"},
    "B 640 sheet window 385": _WINDOW | {"cylinder labels>=6 beside plane segments>=2", "m steps across 384", "m steps across 64",
                                        "multi-pass first m=385", "wins=2"},
    "B 640 sheet strips 32x6+1": _SHEET | {"candidates>=3", "stop at 2", "stop in 3..16", "stop in 17..42", "sub-segments=2", "wins=1", "wins=2"},
    "B 640 sheet strips 32x8+1": _SHEET | {"best<6 break", "candidates>=3", "ended by minimumCellActivated", "stop at 2", "stop in 3..16",
                                           "sub-segments=2", "wins=2"},
    "B 640 sheet strips 16x4+1": _SHEET | {"best<6 break", "stop at 2", "sub-segments=2", "wins=2"},
    "B 1280 sheet window 768": _WINDOW | {"m steps across 384", "multi-pass first m=768", "wins=1", "wins=2"},
    "B 1280 sheet window 769": _WINDOW | {"cylinder labels>=6 beside plane segments>=2", "m steps across 384", "m steps across 768",
                                         "multi-pass first m=769", "wins=1", "wins=2"},
    "B 1280 sheet window 1536": _WINDOW | {"m steps across 384", "m steps across 768", "multi-pass first m=1536"},
    "B 1280 sheet window 1537": _WINDOW | {"m steps across 384", "m steps across 768", "multi-pass first m=1537", "wins=2"},
    "B 320 bhaskara sheet 192": _SHEET | {"320x240 under one cache pass", "m steps across 64", "plane and cylinder win in one candidate",
                                         "sub-segments>=4", "wins=2"},
}


def _b_cases():
    tilted = dict(z0=2000, amp=150, period=240, tilt=0.3)
    wide = dict(z0=2000, amp=150, period=480, tilt=0.3)
    rows = [
        ("flat sheet", 640, 480, sheet_case(640, 480, z0=3000, amp=300, period=400)),
        ("tilted sheet", 640, 480, sheet_case(640, 480, **tilted)),
        ("tilted bhaskara sheet", 640, 480, sheet_case(640, 480, wave=bhaskara, **tilted)),
        ("noisy tilted sheet", 640, 480, sheet_case(640, 480, sigma=4.0, seed=1, **tilted)),
        ("sheet window 384", 640, 480, sheet_case(640, 480, (0, 0, 32, 12, 0), **tilted)),
        ("sheet window 385", 640, 480, sheet_case(640, 480, (0, 0, 32, 12, 1), **tilted)),
        ("sheet strips 32x6+1", 640, 480, sheet_case(640, 480, (0, 0, 32, 6, 1), **tilted)),
        ("sheet strips 32x8+1", 640, 480, sheet_case(640, 480, (0, 0, 32, 8, 1), **tilted)),
        ("sheet strips 16x4+1", 640, 480, sheet_case(640, 480, (0, 0, 16, 4, 1), **tilted)),
        ("sheet window 768", 1280, 960, sheet_case(1280, 960, (0, 0, 64, 12, 0), **wide)),
        ("sheet window 769", 1280, 960, sheet_case(1280, 960, (0, 0, 64, 12, 1), **wide)),
        ("sheet window 1536", 1280, 960, sheet_case(1280, 960, (0, 0, 64, 24, 0), **wide)),
        ("sheet window 1537", 1280, 960, sheet_case(1280, 960, (0, 0, 64, 24, 1), **wide)),
        ("bhaskara sheet 192", 320, 240, sheet_case(320, 240, z0=1500, amp=150, period=160, tilt=0.3, wave=bhaskara)),
    ]
    return [Case("B %d %s" % (w, name), w, h, w / 640.0, build, B_EDGES["B %d %s" % (w, name)]) for name, w, h, build in rows]


CASES = _a_cases() + _b_cases()
SIZES = ((640, 480), (1280, 960), (320, 240))


def cases_of_size(width, height):
    return [c for c in CASES if (c.width, c.height) == (width, height)]
