"""The cases the loop-closure refinement's tests share (tests/test_closure_refine_host.py on the CPU,
tests/test_gpu_closure_refine.py on the GPU): the ten-scan graph and the query of
tests/test_gpu_closure.py's fixture rebuilt with synth, the candidates [4], [5, 6], [1, 2] (and two of wider grids), 100
beams, the resolutions 0.25 (power-of-two indexing) and 0.3 (divide), and per candidate two starts:
the scan's guess plus the oracle's lattice correction on that candidate's map, and the guess itself.

The synthetic room's walls lie 4 m from its centre and a candidate's grid reaches 4.75 m beyond its
scans' poses: no beam of the query falls into column 0 or the last row of a slot's grid.  DESIGNED
is a stored scan and a query made for that: the stored scan fills columns 0 and 1 and the two last
rows of its grid with six points a cell (they score), and column 2 with three a cell (n < 5: they
do not, next to cells that do); the query's beams land in column 0 and in the last row.  case()
asserts, once, what the GPU tests rely on.  Computed once, left unchanged."""
import numpy as np

import oracle_lib as O
import refine_restatement as R
from ndt_2d_amd import synth

WORLD = (4.0, 4.0, 0.25)
RANGE_MAX = 4.75
BEAMS = 100
SMALL = dict(search_angular_size=0.045, search_angular_resolution=0.02,
             search_linear_size=0.065, search_linear_resolution=0.02, laser_max_beams=BEAMS)
N_POINTS = (720, 360, 90, 181, 720, 97, 512, 720, 333, 720)
CANDIDATES = ([4], [5, 6], [1, 2])
# The grids of those three are all 39 x 39 cells at 0.25 (their poses lie within 0.2 m of each other:
# only the origins differ) and 32 x 32 or 33 x 33 at 0.3.  Two candidates whose scans lie further
# apart give the calls slots of other sizes: 46 x 41 and 41 x 40 at 0.25.
WIDE = ([0, 9], [3, 6])
RESOLUTIONS = (0.25, 0.3)
DESIGNED_ID = len(N_POINTS)          # the designed scan is stored behind the graph's
DESIGNED_START = np.array([0.02, -0.01, 0.005])

_GRAPH = []
_CASES = {}


def graph():
    """tests/test_gpu_closure.py's fixture: ten scans along a path through the room, 90 to 720
    points, and the scan to close loops for."""
    if not _GRAPH:
        w = synth.world_of(WORLD)
        poses, points = [], []
        for i, n in enumerate(N_POINTS):
            pose = (-0.9 + 0.2 * i, 0.35 - 0.08 * i + (0.11 if i % 2 else 0.0), 0.05 * i - 0.2)
            assert not synth.pose_blocked(w, pose[0], pose[1])
            poses.append(pose)
            points.append(synth.scan(w, pose, 7000 + i, n_beams=n))
        query = synth.scan(w, (0.13, -0.07, 0.031), 7100)
        _GRAPH.append(dict(world=w, poses=np.array(poses), points=points, query=query, guess=np.array([0.1, -0.05, 0.02])))
    return _GRAPH[0]


def designed(resolution):
    """(stored scan, query): the stored scan is taken at pose (0, 0, 0), so its points are world
    points and its grid is the square of int(2 range_max / resolution + 1) cells from (-range_max,
    -range_max); the query's 100 beams, seen from DESIGNED_START, land in the middle of cells of
    column 0 (48 of them) and of the last row (48), and in column 1 (4)."""
    n = int((RANGE_MAX - -RANGE_MAX) / resolution + 1)
    origin = -RANGE_MAX
    frac = np.array([(0.2, 0.3), (0.7, 0.25), (0.5, 0.8), (0.3, 0.6), (0.8, 0.7), (0.45, 0.45)])
    rng = np.random.default_rng(4242)
    stored = []

    def fill(gx, gy, count):
        f = np.clip(frac[:count] + rng.uniform(-0.05, 0.05, (count, 2)), 0.05, 0.95)
        stored.append(np.stack([origin + (gx + f[:, 0]) * resolution, origin + (gy + f[:, 1]) * resolution], axis=1))

    for gy in range(n):
        fill(0, gy, 6)
        fill(1, gy, 6)
        if gy < n - 2:
            fill(2, gy, 3)                 # n < 5: cannot score, beside column 1, which can
    for gx in range(2, n):
        fill(gx, n - 1, 6)
        fill(gx, n - 2, 6)
    stored = np.concatenate(stored)
    rows = np.linspace(2, n - 4, 48).astype(int)
    world = [(origin + 0.5 * resolution, origin + (gy + 0.5) * resolution) for gy in rows]
    world += [(origin + (gx + 0.5) * resolution, origin + (n - 0.5) * resolution) for gx in rows + 1]
    # ... and four in column 1, whose 3 x 3 holds cells of column 2: n < 5 beside cells that score
    world += [(origin + 1.5 * resolution, origin + (gy + 0.4) * resolution) for gy in (4, 9, 14, 19)]
    world = np.array(world)
    x, y, t = DESIGNED_START
    c, s = np.cos(t), np.sin(t)
    d = world - (x, y)
    query = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)   # R^T (p - t)
    return stored, query


def _own_cells(grid, beams, pose):
    c, s = R.cos_sin(pose[2])
    qx = c * beams[:, 0] - s * beams[:, 1] + pose[0]
    qy = s * beams[:, 0] + c * beams[:, 1] + pose[1]
    idx = grid.index(qx, qy)
    return idx[idx >= 0]


def case(resolution):
    """dict(params, slots = [dict(candidate = [(id, pose)], stored = the scans to add, ref = the
    oracle's matcher holding the candidate's map, grid = the restatement's, query, beams = the query
    as scorePoints subsamples it, starts[2])]): the three candidates of the graph, the two wide ones,
    then DESIGNED (slots[-1])."""
    if resolution in _CASES:
        return _CASES[resolution]
    g = graph()
    params = dict(SMALL, ndt_resolution=resolution, range_max=RANGE_MAX)
    stored, dquery = designed(resolution)
    slots = []
    for ids in list(CANDIDATES) + list(WIDE) + [[DESIGNED_ID]]:
        if ids == [DESIGNED_ID]:
            cand, scans, query, guess = [(DESIGNED_ID, np.zeros(3))], [(np.zeros(3), stored)], dquery, DESIGNED_START
        else:
            cand = [(i, g["poses"][i]) for i in ids]
            scans, query, guess = [(g["poses"][i], g["points"][i]) for i in ids], g["query"], g["guess"]
        ref = O.ScanMatcherNDT()
        ref.initialize(**params)
        ref.addScans(scans)
        won = ref.matchScan(guess, query)
        assert won["best_index"] != O.UINT64_MAX
        slots.append(dict(candidate=cand, ref=ref, grid=R.Grid.of_oracle(ref), query=query, beams=R.subsample(query, BEAMS),
                          starts=np.array([guess + won["pose"], guess])))
    # what the GPU tests rely on.  The slot grids of a call differ in their cell counts: at least
    # three sizes, of both parities (the closure's table is written two entries a store: entry
    # ncell is the first or the second of its pair) ...
    ncells = [s["grid"].size_x * s["grid"].size_y for s in slots]
    assert len(set(ncells)) >= 3 and {n % 2 for n in ncells} == {0, 1}, ncells
    # ... some beam's own cell lies in column 0 and some in the last row of its slot's grid (the
    # 3 x 3 clip is exercised on both sides): the synthetic scans give none, the designed ones do
    edge = []
    for s in slots:
        grid = s["grid"]
        own = np.concatenate([_own_cells(grid, s["beams"], p) for p in s["starts"]])
        edge.append((bool(np.any(own % grid.size_x == 0)), bool(np.any(own // grid.size_x == grid.size_y - 1))))
    assert edge[-1] == (True, True), edge
    # ... and the designed map has cells of n < 5 beside cells that score
    cells = slots[-1]["grid"].cells.reshape(slots[-1]["grid"].size_y, slots[-1]["grid"].size_x, 6)
    assert np.all(cells[:-2, 2, 5] == 3) and np.all(cells[:, 1, 5] >= 5) and np.all(cells[:, 0, 5] >= 5)
    _CASES[resolution] = dict(params=params, slots=slots, designed_scan=stored, ncells=ncells)
    return _CASES[resolution]

