"""The large lane search with the beam table's near_bits word (csrc/ndt2d_near_bits.h): a beam whose
bit for the tile's column and row is clear skips the per-lane near-boundary test, so a wrong bit
would send a lane within the guard band to the look-up's cell -- the cell ACROSS the boundary.

The checkerboard of tests/designed_grids.py (4 m cells: neighbours along an axis score 1.0 and
9e-14, a wrong cell is a gross error), 256 beams, a lattice of 2^-6 m steps at theta = 0 and the
robot at the origin, so that a candidate's point is beam + offset exactly.  The searches here hold
fewer than 4,096 work items, so the map has one sub-cell per cell and a fixed-point unit is
cell_size / 65536 = 2^-14 m: every coordinate below is a multiple of it and the distances are exact.
Thirty of the beams are moved so that one chosen lattice step lies 0, 1, 3, 4 or 5 units below or
above a cell boundary on x, on y, or on both (the band is -4 <= u < 4).

Three kernel forms (launch_match_lane, csrc/ndt2d_match_lane.hip): the six-wave compacted-records
kernel needs more work items than four waves on every CU hold (n_theta * ceil(n_lin / 8)^2 >
4 * CUs), without strips (n_lin = 32) and with them (n_lin = 33: a 1 x 64 strip on two sides);
NDT2D_LANE_PARTS=1 keeps those unsplit, and without it a lattice of so few items has its beams cut
into parts.  Every leg asserts the kernel's name.
"""
import numpy as np
import pytest

import designed_grids as D

pytestmark = pytest.mark.gpu

UNIT = 4.0 / 65536.0
STEP = 2.0 ** -6
N_BEAMS = 256
DISTANCES = (0, 1, 3, 4, 5)
FORMS = {"compact": (32, "1"), "compact-strips": (33, "1"), "beam-parts": (32, None)}

_cache = {}


def _lattice(n_lin):
    return (np.arange(n_lin) - n_lin // 2) * STEP


def _designed_beams(board, n_lin):
    """256 beam end points in cell interiors, thirty of them moved by whole units so that lattice
    step `ix` (or `iy`, or both) lands `u` units from a boundary between two cells of another kind:
    (beams, [(beam, axis, u)])."""
    dlin = _lattice(n_lin)
    size = board.size_x
    kind = board.kind.reshape(size, size)                       # [gy][gx]
    beams = np.zeros((N_BEAMS, 2))
    for j in range(N_BEAMS):
        gx, gy = 1 + (j * 3) % (size - 2), 1 + (j * 5) % (size - 2)
        beams[j] = (board.origin[0] + (gx + 0.5) * 4.0 + (j % 7) * 37 * UNIT,
                    board.origin[1] + (gy + 0.5) * 4.0 - (j % 5) * 91 * UNIT)
    # boundaries x = 4 gx between (gx - 1, gy) and (gx, gy) of different kinds, and the same on y
    x_sites = [(gx, gy) for gy in range(1, size - 1) for gx in range(2, size - 1) if kind[gy, gx - 1] != kind[gy, gx]]
    y_sites = [(gx, gy) for gx in range(1, size - 1) for gy in range(2, size - 1) if kind[gy - 1, gx] != kind[gy, gx]]
    placed = []
    k = 0
    for axis in ("x", "y", "both"):
        for d in DISTANCES:
            for sign in (-1, 1):
                u = sign * d
                j = k * 8 + (k * 3) % 8                        # spread over the chunks, the groups and the parts
                ix, iy = (7 * k + 3) % n_lin, (11 * k + n_lin - 1) % n_lin
                gx, gy = (x_sites if axis != "y" else y_sites)[(5 * k) % len(x_sites if axis != "y" else y_sites)]
                if axis in ("x", "both"):
                    beams[j, 0] = board.origin[0] + 4.0 * gx + u * UNIT - dlin[ix]
                    if axis == "x":
                        beams[j, 1] = board.origin[1] + (gy + 0.5) * 4.0 + 13 * UNIT
                if axis in ("y", "both"):
                    beams[j, 1] = board.origin[1] + 4.0 * gy + u * UNIT - dlin[iy]
                    if axis == "y":
                        beams[j, 0] = board.origin[0] + (gx + 0.5) * 4.0 + 13 * UNIT
                placed.append((j, axis, u))
                k += 1
    assert len({j for j, _, _ in placed}) == len(placed) == 30
    return beams, placed


def _signed_units(p, origin):
    """Distance of every coordinate from the nearest cell boundary in fixed-point units, exact here."""
    f = (p - origin) / 4.0 * 65536.0
    assert np.array_equal(f, np.rint(f))
    u = np.mod(f, 65536.0)
    return np.where(u < 32768.0, u, u - 65536.0)


def _expectation(board, beams, dlin):
    """Per candidate (ix, iy) of ONE theta step: the sum of the beams' terms in beam order, the cell
    by getIndex on the same doubles (held to the oracle's by tests/test_designed_grids.py); and per
    distance class how many (candidate, beam) points the reference arithmetic places in it."""
    n = len(dlin)
    total = np.zeros(n * n)
    classes = {}
    for b in range(len(beams)):
        px, py = D.search_points(beams[b], (0.0, 0.0), 1.0, 0.0, dlin)
        assert np.array_equal(px, beams[b, 0] + dlin)
        total = total + board.expected_terms(np.repeat(px, n), np.tile(py, n))
        ux = np.abs(np.repeat(_signed_units(px, board.origin[0]), n))
        uy = np.abs(np.tile(_signed_units(py, board.origin[1]), n))
        for d in DISTANCES:
            for axis, hit in (("x", (ux == d) & (uy > 5)), ("y", (uy == d) & (ux > 5)), ("both", (ux == d) & (uy == d))):
                classes[(axis, d)] = classes.get((axis, d), 0) + int(hit.sum())
    return -total, classes


def _case(form):
    if form in _cache:
        return _cache[form]
    import torch
    from test_gpu_designed_grids import Device
    n_lin, _ = FORMS[form]
    board = D.Checkerboard(4.0, (0.0, 0.0))
    dlin = _lattice(n_lin)
    beams, placed = _designed_beams(board, n_lin)
    want, classes = _expectation(board, beams, dlin)
    # more (theta, 8 x 8 patch) items than the four-wave blocks of every CU hold: the six-wave kernels
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p1 = (n_lin + 7) // 8
    n_th = 4 * cus // (p1 * p1) + 1
    assert 4 * cus < n_th * p1 * p1 < 4096          # (below 4,096 items: one map sub-cell per cell)
    with Device() as dev:
        dev.install(board.grid)
        dev.set_search(beams, (0.0, 0.0), dlin, 1.0, 0.0, n_th=n_th)
        lane, lane_name = dev.search("lane")
        noskip, noskip_name = dev.search("lane-noskip")
    c = dict(n_lin=n_lin, n_th=n_th, want=want, classes=classes, placed=placed, lane=lane, noskip=noskip,
             names=(lane_name, noskip_name))
    _cache[form] = c
    return c


@pytest.mark.parametrize("form", list(FORMS))
def test_scores_next_to_cell_boundaries(form, monkeypatch):
    if FORMS[form][1] is None:
        monkeypatch.delenv("NDT2D_LANE_PARTS", raising=False)
    else:
        monkeypatch.setenv("NDT2D_LANE_PARTS", FORMS[form][1])
    c = _case(form)
    # the reference arithmetic alone puts candidates in every designed class
    print("\n%s: n_lin %d, %d theta steps, kernels %r; (candidate, beam) points per class: %r" % (
        form, c["n_lin"], c["n_th"], c["names"], c["classes"]))
    for axis in ("x", "y", "both"):
        for d in DISTANCES:
            assert c["classes"][(axis, d)] >= 1, (axis, d)
    # the intended kernel ran
    for name in c["names"]:
        assert name.startswith("match/lane-per-candidate/lds-grid/compact-records") and name.endswith("/pow2"), name
        assert ("/beam-parts" in name) == (form == "beam-parts"), name
    assert (c["n_lin"] % 8 in (1, 2, 3, 4)) == (form == "compact-strips")
    # skip against no-skip: the same bits; both against the expectation
    assert np.array_equal(c["lane"], c["noskip"])
    per = c["n_lin"] ** 2
    for t in range(c["n_th"]):
        assert np.array_equal(c["lane"][t * per:(t + 1) * per], c["lane"][:per]), t
    err = float(np.max(np.abs(c["lane"][:per] - c["want"])))
    print("%s: max |score - expectation| = %.3e" % (form, err))
    assert err < 1e-9
