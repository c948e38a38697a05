"""The window table of record addresses of the large lane search's compacted-records forms
(csrc/ndt2d_address_table.h; the staging and the launcher in csrc/ndt2d_match_lane.hip; the exact path
of lane_beams, csrc/ndt2d_lane_fn.h): a block stages one entry per cell of the padded map window -- the
LDS address of the cell's compacted record -- and an exact evaluation goes from the look-up's two cell
bytes to its record through it.  These are the places where a window-shaped table can be wrong while
the grid's own cell -> rank table was right: the window's origin, its clipping, the row stride, the
padding beyond the grid, the sentinel, and the near-boundary path's way into the same table.

Every case compares three things: every candidate's score of the `lane` variant with `lane-noskip`
(every term evaluated) bit for bit; scores, winner and record with a numpy expectation -- the cell by
getIndex, the term by exp of record_exponent, summed in beam order (tests/designed_grids.py, held to the
oracle's by tests/test_designed_grids.py), within the 1e-9 the lane search's parity tests use; and
scores and record, bit for bit, with the rank table's instantiation, which NDT2D_LANE_ADDRESS_TABLE=0
forces at run time, and with the table of one-byte ranks (NDT2D_LANE_ADDRESS_TABLE=1: what a search
takes whose image does not fit a CU twice with four-byte entries, for a grid of at most 255 cells that
can score; a grid of more then takes the rank table's instantiation).

Launches.  Grids are given as cell records (ndt2d_set_grid), 4 m cells, theta = 0, so a candidate's
point is beam + pose + offset.  The compacted six-wave form needs >= 256 beams (launch_match_lane:
dynamic items) and more (theta, 8 x 8 patch) items than four waves on every CU hold (n_items > 4 x CUs:
1,024 on 256 CUs); the smallest such lattice here is n_lin = 24 (9 patches) with 4 x CUs // 9 + 1 theta
steps (114 on 256 CUs: 1,026 items).  NDT2D_LANE_PARTS=1 keeps a lattice below 18,432 items unsplit;
without it the beams are cut into parts (match_lane_compact_parts_kernel).  Below 4,096 items the map
has one sub-cell per cell, from 4,096 on 4 x 4 (the table is per CELL either way).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import designed_grids as D

pytestmark = pytest.mark.gpu

CELL = 4.0
STEP = 0.25


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lds_per_block():
    import torch
    props = torch.cuda.get_device_properties(0)
    return int(getattr(props, "shared_memory_per_block", 160 * 1024))


def _steps_for(n_lin):
    p1 = (n_lin + 7) // 8
    n_th = 4 * _cus() // (p1 * p1) + 1
    assert 4 * _cus() < n_th * p1 * p1 < 4096
    return n_th


def _lattice(n_lin, step=STEP):
    return (np.arange(n_lin) - n_lin // 2) * step


class Grid:
    """size_x x size_y cells of 4 m from `origin`.  ONE: information 0, the term is exactly 1.0 anywhere
    in the cell; iso: isotropic, the mean near the cell, terms of every size."""

    def __init__(self, size_x, size_y, origin):
        self.size_x, self.size_y, self.origin = size_x, size_y, (float(origin[0]), float(origin[1]))
        self.cells6 = np.zeros((size_x * size_y, 6))

    def centre(self, gx, gy):
        return (self.origin[0] + CELL * (gx + 0.5), self.origin[1] + CELL * (gy + 0.5))

    def one(self, gx, gy):
        cx, cy = self.centre(gx, gy)
        self.cells6[gy * self.size_x + gx] = (cx, cy, 0.0, 0.0, 0.0, 5.0)

    def iso(self, gx, gy, rng):
        cx, cy = self.centre(gx, gy)
        i = 2.0 * rng.uniform(0.5, 90.0) / 16.0
        self.cells6[gy * self.size_x + gx] = (cx + rng.uniform(-8.0, 8.0), cy + rng.uniform(-8.0, 8.0), i, 0.0,
                                              i * rng.uniform(0.5, 2.0), 5.0)

    def fill(self, rng, share, cells=None):
        """`share` of the cells (or exactly the given flat indices) hold a distribution, one in eight of them ONE."""
        n = self.size_x * self.size_y
        chosen = np.flatnonzero(rng.random(n) < share) if cells is None else np.asarray(cells)
        for cell in chosen:
            gx, gy = int(cell % self.size_x), int(cell // self.size_x)
            if rng.random() < 0.125:
                self.one(gx, gy)
            else:
                self.iso(gx, gy, rng)

    @property
    def n_occ(self):
        return int((self.cells6[:, 5] >= 5.0).sum())

    @property
    def grid(self):
        return self.cells6, self.size_x, self.size_y, CELL, self.origin

    def terms(self, px, py):
        idx = D.get_index(px, py, self.size_x, self.size_y, CELL, self.origin)
        rec = self.cells6[np.maximum(idx, 0)]
        with np.errstate(under="ignore"):
            term = np.exp(D.record_exponent(rec, np.asarray(px), np.asarray(py)))
        return np.where((idx >= 0) & (rec[:, 5] >= 5.0), term, 0.0)


def expectation(grid, beams, pose, dlin):
    """Scores of one theta step, candidate (ix, iy) at ix * n_lin + iy: the terms added in beam order."""
    n = len(dlin)
    total = np.zeros(n * n)
    for b in beams:
        px, py = D.search_points(b, pose, 1.0, 0.0, dlin)
        total = total + grid.terms(np.repeat(px, n), np.tile(py, n))
    return -total


def window(grid, beams, pose, dlin):
    """lane_geometry's window of grid cells and border (csrc/ndt2d_lane_fn.h): (x0, y0, w, h, pad)."""
    reach = float(np.max(np.hypot(beams[:, 0], beams[:, 1]))) + float(np.max(np.abs(dlin)))
    out = []
    for p, o, size in ((pose[0], grid.origin[0], grid.size_x), (pose[1], grid.origin[1], grid.size_y)):
        lo = max(math.floor((p - reach - o) / CELL) - 1.0, 0.0)
        hi = min(math.floor((p + reach - o) / CELL) + 1.0, size - 1.0)
        assert lo <= hi
        out.append((int(lo), int(hi - lo) + 1))
    pad = int(2.0 * float(np.max(np.abs(dlin))) / CELL) + 3
    return out[0][0], out[1][0], out[0][1], out[1][1], pad


def _search(dev, variant, knob):
    """(scores, (best_score, best_index, the ten sums), kernel name); knob: NDT2D_LANE_ADDRESS_TABLE."""
    from ndt_2d_amd import _capi
    L, h = dev.L, dev.h
    before = os.environ.get("NDT2D_LANE_ADDRESS_TABLE")
    if knob is None:
        os.environ.pop("NDT2D_LANE_ADDRESS_TABLE", None)
    else:
        os.environ["NDT2D_LANE_ADDRESS_TABLE"] = knob
    assert L.ndt2d_set_variant(h, variant.encode()) == 0, variant
    try:
        sc = np.full(dev.n_th * dev.n_lin ** 2, 123.0)
        res = _capi.MatchResult()
        rc = L.ndt2d_match(h, 0, dev.n_th, _capi.dptr(sc), C.byref(res))
        assert rc == 0, (variant, rc, dev.error())
        assert res.n_candidates == len(sc)
        return sc, (res.best_score, int(res.best_index), tuple(res.acc)), L.ndt2d_last_variant(h).decode()
    finally:
        assert L.ndt2d_set_variant(h, b"auto") == 0
        if before is None:
            os.environ.pop("NDT2D_LANE_ADDRESS_TABLE", None)
        else:
            os.environ["NDT2D_LANE_ADDRESS_TABLE"] = before


def run(grid, beams, pose, dlin, n_th):
    from test_gpu_designed_grids import Device
    with Device() as dev:
        dev.install(grid.grid)
        dev.set_search(beams, pose, dlin, 1.0, 0.0, n_th=n_th)
        return {"lane": _search(dev, "lane", None), "noskip": _search(dev, "lane-noskip", None),
                "rank": _search(dev, "lane", "0"), "rank-noskip": _search(dev, "lane-noskip", "0"),
                "byte": _search(dev, "lane", "1"), "byte-noskip": _search(dev, "lane-noskip", "1")}


def check(tag, got, want, n_lin, n_th, parts=False):
    """The three comparisons of the module's docstring; returns the scores of one theta step."""
    lane, record, _ = got["lane"]
    print("\n%s: n_lin %d, %d theta steps, kernels %r" % (tag, n_lin, n_th, [got[k][2] for k in got]))
    for key in got:
        assert got[key][2].startswith("match/lane-per-candidate/lds-grid/compact-records"), (key, got[key][2])
        assert got[key][2].endswith("/pow2") and ("/beam-parts" in got[key][2]) == parts, (key, got[key][2])
    assert not np.isnan(lane).any()
    assert np.array_equal(lane, got["noskip"][0])
    # the rank table's instantiation: the same record for every point, so the same bits throughout
    assert np.array_equal(lane, got["rank"][0]) and np.array_equal(lane, got["rank-noskip"][0])
    assert np.array_equal(lane, got["byte"][0]) and np.array_equal(lane, got["byte-noskip"][0])
    assert record == got["rank"][1] == got["byte"][1], (record, got["rank"][1], got["byte"][1])
    assert got["noskip"][1] == got["rank-noskip"][1] == got["byte-noskip"][1]
    per = n_lin * n_lin
    for t in range(n_th):
        assert np.array_equal(lane[t * per:(t + 1) * per], lane[:per]), t
    err = float(np.max(np.abs(lane[:per] - want)))
    print("%s: max |score - expectation| = %.3e, scores %.6g .. %.6g" % (tag, err, lane[:per].min(), lane[:per].max()))
    assert err < 1e-9
    # a candidate all of whose points lie off the grid or in cells that cannot score: exactly zero
    assert np.all(lane[:per][want == 0.0] == 0.0)
    # winner and record
    best_score, best_index, acc = record
    if (lane < 0.0).any():
        assert best_score == lane.min() and best_index == int(np.argmin(lane))
        assert abs(want[best_index % per] - want.min()) < 1e-9 and abs(best_score - want.min()) < 1e-9
        total = math.fsum(lane)
        assert abs(acc[9] - total) <= 1e-12 * abs(total), (acc[9], total)
    else:
        assert best_score == 0.0 and not any(acc)
    return lane[:per]


# ---------------------------------------------------------------------------------------------
# where the window lies in the grid: 37 x 53 cells (size_x != size_y, both odd)
# ---------------------------------------------------------------------------------------------

_scenes = {}


def _odd_grid():
    if "odd" not in _scenes:
        g = Grid(37, 53, (-8.0, 12.0))
        g.fill(np.random.default_rng(5), 0.4)
        _scenes["odd"] = g
    return _scenes["odd"]


def _scene(place, n_beams=512):
    """Beams that end within 4 cells of the robot on either axis; the first four end on the robot, in a
    ONE cell put there, so that the candidates around the middle score at once and their skip levels rise."""
    key = ("scene", place)
    if key not in _scenes:
        g = _odd_grid()
        cell = {"far": (27, 40), "corner": (1, 1), "far-corner": (35, 51)}[place]
        pose = g.centre(*cell)
        rng = np.random.default_rng(11)
        beams = np.round(rng.uniform(-16.0, 16.0, (n_beams, 2)) * 64.0) / 64.0
        beams[:4] = 0.0
        grid = Grid(g.size_x, g.size_y, g.origin)
        grid.cells6 = g.cells6.copy()
        grid.one(*cell)
        _scenes[key] = (grid, beams, pose)
    return _scenes[key]


# case: (place, n_lin, theta steps or None = the smallest compacted launch, NDT2D_LANE_PARTS)
PLACES = {
    "far-from-origin": ("far", 24, None, "1"),
    "far-from-origin-strips": ("far", 26, None, "1"),
    "corner": ("corner", 24, None, "1"),
    "far-corner-strips": ("far-corner", 26, None, "1"),
    "far-from-origin-beam-parts": ("far", 24, None, None),
    # 9 patches x 456 steps = 4,104 items: the map at 4 x 4 sub-cells per cell, the beams in four parts
    "far-from-origin-fine-map-beam-parts": ("far", 24, 456, None),
}


@pytest.mark.parametrize("case", list(PLACES))
def test_window_anywhere_in_the_grid(case, monkeypatch):
    place, n_lin, n_th, parts = PLACES[case]
    if parts is None:
        monkeypatch.delenv("NDT2D_LANE_PARTS", raising=False)
    else:
        monkeypatch.setenv("NDT2D_LANE_PARTS", parts)
    grid, beams, pose = _scene(place)
    dlin = _lattice(n_lin)
    n_th = _steps_for(n_lin) if n_th is None else n_th
    x0, y0, w, h, pad = window(grid, beams, pose, dlin)
    print("\n%s: window (%d, %d) + %d x %d, pad %d, %d cells can score" % (case, x0, y0, w, h, pad, grid.n_occ))
    if place == "far":
        assert x0 > pad and y0 > pad and x0 + w < grid.size_x and y0 + h < grid.size_y
    elif place == "corner":
        assert x0 == 0 and y0 == 0                               # clipped on two sides
    else:
        assert x0 + w == grid.size_x and y0 + h == grid.size_y   # ... on the other two
    assert (n_lin % 8 in (1, 2, 3, 4)) == ("strips" in case)
    key = ("want", place, n_lin)
    if key not in _scenes:
        _scenes[key] = expectation(grid, beams, pose, dlin)
    got = run(grid, beams, pose, dlin, n_th)
    scores = check(case, got, _scenes[key], n_lin, n_th, parts=parts is None)
    assert (scores < 0.0).all() and np.all(scores.reshape(n_lin, n_lin)[6:18, 6:18] <= -4.0)
    assert len(np.unique(scores)) > n_lin * n_lin // 2


# ---------------------------------------------------------------------------------------------
# the grid's edges: 9 x 7 cells, the whole grid in the window, beams that end one cell outside
# ---------------------------------------------------------------------------------------------

def _edge_scene():
    """Every cell of the first and last row and column holds a distribution (ONE cells at the corners
    and every third cell between), the inside is empty.  Beams from the robot in the grid's middle end
    half a cell outside the grid on each of the four sides, opposite every edge cell, and half a cell
    inside it: with offsets up to 3 m either way a patch's candidates straddle the edge -- lanes in an
    edge cell beside lanes in the window's padding, whose entries must give exactly nothing."""
    rng = np.random.default_rng(17)
    g = Grid(9, 7, (12.0, -20.0))
    for gy in range(g.size_y):
        for gx in range(g.size_x):
            if gx in (0, g.size_x - 1) or gy in (0, g.size_y - 1):
                if (gx + gy) % 3 == 0 or (gx in (0, g.size_x - 1) and gy in (0, g.size_y - 1)):
                    g.one(gx, gy)
                else:
                    g.iso(gx, gy, rng)
    pose = g.centre(4, 3)
    ends = []
    for gx in range(g.size_x):
        x = g.centre(gx, 0)[0]
        for y in (g.origin[1] - 2.0, g.origin[1] + 2.0, g.origin[1] + CELL * g.size_y + 2.0, g.origin[1] + CELL * g.size_y - 2.0):
            ends.append((x, y))
    for gy in range(g.size_y):
        y = g.centre(0, gy)[1]
        for x in (g.origin[0] - 2.0, g.origin[0] + 2.0, g.origin[0] + CELL * g.size_x + 2.0, g.origin[0] + CELL * g.size_x - 2.0):
            ends.append((x, y))
    ends = np.array(ends)
    beams = np.tile(ends, (5, 1))[:320] - np.array(pose)       # 64 designed ends, repeated: 320 beams
    return g, beams, pose


def test_padding_beyond_each_edge_of_the_grid(monkeypatch):
    monkeypatch.setenv("NDT2D_LANE_PARTS", "1")
    n_lin = 24
    grid, beams, pose = _edge_scene()
    dlin = _lattice(n_lin)
    n_th = _steps_for(n_lin)
    x0, y0, w, h, pad = window(grid, beams, pose, dlin)
    assert (x0, y0, w, h) == (0, 0, grid.size_x, grid.size_y)
    want = expectation(grid, beams, pose, dlin)
    # points on both sides of every edge, in the reference's own arithmetic
    outside = inside = 0
    for b in beams[:64]:
        px, py = D.search_points(b, pose, 1.0, 0.0, dlin)
        idx = D.get_index(np.repeat(px, n_lin), np.tile(py, n_lin), grid.size_x, grid.size_y, CELL, grid.origin)
        outside += int((idx < 0).sum())
        inside += int((idx >= 0).sum())
    assert outside > 5000 and inside > 5000
    got = run(grid, beams, pose, dlin, n_th)
    scores = check("edges", got, want, n_lin, n_th)
    assert (scores < 0.0).all()

    # every beam ends a cell and a half outside: no candidate comes back in, every score is exactly zero
    far_out = beams.copy()
    ends = far_out + np.array(pose)
    ends[:, 0] = np.where(ends[:, 0] < grid.origin[0] + 3.0, grid.origin[0] - 6.0, ends[:, 0])
    ends[:, 0] = np.where(ends[:, 0] > grid.origin[0] + CELL * grid.size_x - 3.0, grid.origin[0] + CELL * grid.size_x + 6.0, ends[:, 0])
    ends[:, 1] = np.where(ends[:, 1] < grid.origin[1] + 3.0, grid.origin[1] - 6.0, ends[:, 1])
    ends[:, 1] = np.where(ends[:, 1] > grid.origin[1] + CELL * grid.size_y - 3.0, grid.origin[1] + CELL * grid.size_y + 6.0, ends[:, 1])
    far_out = ends - np.array(pose)
    want = expectation(grid, far_out, pose, dlin)
    assert not want.any()
    got = run(grid, far_out, pose, dlin, n_th)
    scores = check("all-outside", got, want, n_lin, n_th)
    assert not scores.any()


# ---------------------------------------------------------------------------------------------
# how many records: one, the most a byte ranks and one more, the most the table's image holds twice a CU and
# one more (the rank table's form)
# ---------------------------------------------------------------------------------------------

def _most_records_with_the_table(size_x, size_y, pad):
    """launch_match_lane: 2 x (map + table + records) <= LDS of a block; the window is the whole grid,
    one map sub-cell per cell.  Also whether one record more still fits with the rank table (the
    compacted form is then still taken, through the rank table's instantiation)."""
    rows, cols = size_y + 2 * pad, size_x + 2 * pad
    stride = 1
    while stride < cols:
        stride *= 2
    map_bytes = 256 * rows
    table_bytes = ((rows * stride + 1) * 4 + 15) // 16 * 16
    rank_bytes = 16 + ((size_x * size_y + 1) * 2 + 15) // 16 * 16
    half = _lds_per_block() // 2
    n = (half - map_bytes - table_bytes) // 48 - 1
    assert map_bytes + table_bytes + (n + 1) * 48 <= half < map_bytes + table_bytes + (n + 2) * 48
    assert map_bytes + rank_bytes + (n + 2) * 48 <= half
    return n


@pytest.mark.parametrize("which", ["one", "byte-most", "byte-most-plus-one", "most", "most-plus-one"])
def test_number_of_records(which, monkeypatch):
    monkeypatch.setenv("NDT2D_LANE_PARTS", "1")
    n_lin = 24
    dlin = _lattice(n_lin)
    size = 41
    rng = np.random.default_rng(23)
    g = Grid(size, size, (0.0, 0.0))
    pose = g.centre(20, 20)
    beams = np.round(rng.uniform(-84.0, 84.0, (256, 2)) * 64.0) / 64.0
    beams[:4] = 0.0
    beams[4] = (84.0, 84.0)
    x0, y0, w, h, pad = window(g, beams, pose, dlin)
    assert (x0, y0, w, h) == (0, 0, size, size)
    most = _most_records_with_the_table(size, size, pad)
    assert 1 < most < size * size - 1
    # (255 cells and the sentinel: the most ranks a byte holds; 256: the one-byte table is not taken)
    n_occ = {"one": 1, "byte-most": 255, "byte-most-plus-one": 256, "most": most, "most-plus-one": most + 1}[which]
    others = np.setdiff1d(np.arange(size * size), [20 * size + 20])
    g.fill(rng, 0.0, cells=rng.choice(others, n_occ - 1, replace=False))
    g.one(20, 20)
    assert g.n_occ == n_occ
    n_th = _steps_for(n_lin)
    want = expectation(g, beams, pose, dlin)
    got = run(g, beams, pose, dlin, n_th)
    print("\n%s: %d records (the table's image holds %d twice a CU)" % (which, n_occ, most))
    scores = check(which, got, want, n_lin, n_th)
    assert np.all(scores.reshape(n_lin, n_lin)[6:18, 6:18] <= -4.0)


# ---------------------------------------------------------------------------------------------
# next to cell boundaries: the near-boundary path ends in the same table
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["compact", "compact-strips", "beam-parts"])
def test_near_boundary_points_and_the_grids_edge(form, monkeypatch):
    """The checkerboard and the thirty designed beams of tests/test_gpu_near_bits.py (a lattice step 0,
    1, 3, 4 or 5 fixed-point units from a boundary on x, on y, on both), and four beams more: one unit
    below the grid's far edge on x and on y -- the exact cell is the last column (row), a ONE cell,
    while the look-up's cell, four units on, lies outside the grid -- and one unit below the grid's
    origin on x and on y: the exact cell is outside, the look-up's is the first column (row), in a ONE cell."""
    import test_gpu_near_bits as N
    n_lin, parts = N.FORMS[form]
    if parts is None:
        monkeypatch.delenv("NDT2D_LANE_PARTS", raising=False)
    else:
        monkeypatch.setenv("NDT2D_LANE_PARTS", parts)
    board = D.Checkerboard(4.0, (0.0, 0.0))
    dlin = N._lattice(n_lin)
    beams, placed = N._designed_beams(board, n_lin)
    kind = board.kind.reshape(board.size_y, board.size_x)
    free = [j for j in range(N.N_BEAMS) if j not in {p[0] for p in placed}][-4:]
    ix, iy = 5, n_lin - 3
    row = int(np.flatnonzero(kind[1:-1, 0] == 1)[0]) + 1        # a ONE cell of the first column
    col = int(np.flatnonzero(kind[0, 1:-1] == 1)[0]) + 1        # ... of the first row
    far = 4.0 * board.size_x
    beams[free[0]] = (far - N.UNIT - dlin[ix], 4.0 * row + 2.0 + 13 * N.UNIT)
    beams[free[1]] = (4.0 * col + 2.0 + 13 * N.UNIT, far - N.UNIT - dlin[iy])
    beams[free[2]] = (-N.UNIT - dlin[ix], 4.0 * row + 2.0 + 13 * N.UNIT)
    beams[free[3]] = (4.0 * col + 2.0 + 13 * N.UNIT, -N.UNIT - dlin[iy])
    want, classes = N._expectation(board, beams, dlin)
    for axis in ("x", "y", "both"):
        for d in N.DISTANCES:
            assert classes[(axis, d)] >= 1, (axis, d)
    # the four beams do what they are for, by the reference arithmetic alone
    n = len(dlin)
    for j, inside in ((free[0], True), (free[1], True), (free[2], False), (free[3], False)):
        px, py = D.search_points(beams[j], (0.0, 0.0), 1.0, 0.0, dlin)
        term = board.expected_terms(np.repeat(px, n), np.tile(py, n)).reshape(n, n)
        at = term[ix, :] if j in (free[0], free[2]) else term[:, iy]
        assert np.all(at[2:-2] == (1.0 if inside else 0.0)), (j, at)
    cus = _cus()
    p1 = (n_lin + 7) // 8
    n_th = 4 * cus // (p1 * p1) + 1
    assert 4 * cus < n_th * p1 * p1 < 4096
    grid = Grid(board.size_x, board.size_y, board.origin)
    grid.cells6 = board.cells6
    got = run(grid, beams, (0.0, 0.0), dlin, n_th)
    assert (n_lin % 8 in (1, 2, 3, 4)) == (form == "compact-strips")
    check(form, got, want, n_lin, n_th, parts=form == "beam-parts")
