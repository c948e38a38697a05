"""Points off the grid (include/ndt2d_hip.h, "Points off the grid") through every host index:
the oracle's getIndex, the numpy restatement's, and the host build's two loops (the side-by-side
quarters of HostNdt::add_scan and the sequential NDT2D_BUILD_SEQUENTIAL loop).  A NaN, +-inf,
1e300 or 2^32-cell point must do exactly what the finite off-grid point (1e6, 1e6) does: nothing
(tests/offgrid_cases.py)."""
import math

import numpy as np
import pytest

import offgrid_cases as G
import oracle_lib as O
from ndt_2d_amd import host_build_grid
from ndt_2d_amd.scan_matcher import BUILD_SEQUENTIAL
from test_oracle_independent import NumpyNDT


def _ndts(name):
    cell, range_max = G.MAPS[name]
    sx, sy, ox, oy = G.geometry(cell, range_max)
    o = O.NDT(cell, 2 * range_max, 2 * range_max, ox, oy)
    n = NumpyNDT(cell, 2 * range_max, 2 * range_max, ox, oy)
    assert (o.size_x, o.size_y) == (n.sx, n.sy) == (sx, sy)
    return o, n


def _oracle_cells(cell, range_max, scans):
    m = O.ScanMatcherNDT()
    m.initialize(ndt_resolution=cell, range_max=range_max)
    m.addScans(scans)
    return np.ascontiguousarray(m.ndt.cells6())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_the_maps_cover_both_builds_and_both_divides():
    seen = set()
    for name, (cell, range_max) in G.MAPS.items():
        sx, sy, _, _ = G.geometry(cell, range_max)
        large = sx * sy * G.HOST_CELL_BYTES > G.SIDE_BY_SIDE_MAX_BYTES
        pow2 = math.frexp(cell)[0] == 0.5
        seen.add((large, pow2))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert G.geometry(0.05, 4.75)[:2] == (191, 191)


@pytest.mark.parametrize("name", sorted(G.MAPS))
def test_get_index_known_answers(name):
    """-1 for every off-grid point, in both restatements; the reference's own cell for the
    finite neighbours of the edges."""
    cell, range_max = G.MAPS[name]
    sx, sy, ox, oy = G.geometry(cell, range_max)
    o, n = _ndts(name)
    for x, y, wrap in G.off_grid_points(cell, range_max):
        assert o.getIndex(x, y) == -1, (x, y)
        assert n.index(x, y) == -1, (x, y)
        if wrap is not None:
            # the reference's x86 conversion (cvttsd2si to 64 bits, low 32 kept) would put the
            # point into column / row k of cell 0's row / column: a cell of the grid
            axis, k = wrap
            f = (x - ox) / cell if axis == "x" else (y - oy) / cell
            assert int(f) % 2 ** 32 == k < min(sx, sy)
    inside = 0
    for x, y in G.edge_controls(cell, range_max):
        want = G.reference_index(cell, range_max, x, y)
        assert o.getIndex(x, y) == n.index(x, y) == want, (x, y)
        inside += want >= 0
    assert inside >= 3              # (ox, y0), (x0, oy), (ox, oy) at least
    assert o.getIndex(ox, oy) == 0 and o.getIndex(ox + (sx - 0.5) * cell, oy + (sy - 0.5) * cell) == sx * sy - 1


@pytest.mark.parametrize("n", G.SCAN_LENGTHS)
@pytest.mark.parametrize("name", sorted(G.MAPS))
def test_host_build_drops_off_grid_points_like_the_finite_substitute(name, n):
    """The host build three ways -- side by side (default), NDT2D_BUILD_SEQUENTIAL, the oracle --
    on the input with the off-grid points, against the oracle on the substitute input: the same
    64-bit patterns in every cell."""
    cell, range_max = G.MAPS[name]
    orig, subs = G.map_scans(name, n)
    want = _oracle_cells(cell, range_max, subs)
    sx, sy, _, _ = G.geometry(cell, range_max)
    # the maps hold what a misplaced point would change: every cell of column 0 and row 0
    counts = want[:, 5].reshape(sy, sx)
    assert (counts[:, 0] >= 5).all() and (counts[0, :] >= 5).all()
    assert not np.isnan(want[counts.reshape(-1) >= 5, 2:5]).any()
    for flags in (0, BUILD_SEQUENTIAL):
        cells, gx, gy, ox, oy = host_build_grid(cell, range_max, orig, flags)
        assert (gx, gy, ox, oy) == (sx, sy, -range_max, -range_max)
        assert np.array_equal(_bits(cells), _bits(want)), (name, n, flags)
    assert np.array_equal(_bits(_oracle_cells(cell, range_max, orig)), _bits(want)), (name, n)


@pytest.mark.parametrize("name", ["p2-small", "div-large"])
def test_host_scoring_of_off_grid_points_is_the_substitutes(name):
    """NDT::likelihood on the oracle (scorePoints / scoreScan) and the numpy restatement: an
    off-grid beam adds +0.0 to the likelihood (src/ndt_model.cpp:169), as the substitute does --
    the same bits."""
    cell, range_max = G.MAPS[name]
    orig, subs = G.map_scans(name, 33)
    m = O.ScanMatcherNDT()
    m.initialize(ndt_resolution=cell, range_max=range_max, laser_max_beams=1000)
    m.addScans(subs)
    for (pose, pts), (_, sub) in zip(orig[3:], subs[3:]):
        for p in ((0.0, 0.0, 0.0), (0.01, -0.02, 0.003)):
            a, b = m.scorePoints(pts, p), m.scorePoints(sub, p)
            assert not math.isnan(b) and b != 0.0
            assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
        assert m.scoreScan(pose, pts) == m.scoreScan(pose, sub)
    # the numpy restatement: the same cell counts from the original input, the same likelihoods
    o, nd = _ndts(name)
    for pose, pts in orig:
        nd.add_scan(pose, pts)
    assert np.array_equal(nd.n, m.ndt.cells6()[:, 5])
    nd.compute()
    for (_, pts), (_, sub) in zip(orig[3:], subs[3:]):
        with np.errstate(invalid="ignore", over="ignore"):
            a = nd.likelihood(pts[:, 0], pts[:, 1])
        assert a == nd.likelihood(sub[:, 0], sub[:, 1]) and a > 0.0
