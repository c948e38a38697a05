"""The large lane search's pre-test against the wave's lowest skip level (csrc/ndt2d_pretest_level.h,
the chunk loop of csrc/ndt2d_match_lane.hip): a 64-beam chunk's flagged beams are tested again
against the least skip level of the wave's 64 lanes, and a group of eight beams none of which stays
flagged is not looked up.  A beam pruned wrongly would lose a lane a term that changes its sum, so
every case compares the `lane` variant with `lane-noskip` (every term evaluated) bit for bit on every
candidate, and with a numpy expectation (the cell by getIndex, the term by exp of record_exponent,
summed in beam order) within the 1e-9 the lane search's parity tests use.

Grids are given as cell records (ndt2d_set_grid), 4 m cells from the origin, theta = 0 and the robot
at the origin: a candidate's point is beam + offset exactly (all coordinates dyadic).  Every search
holds fewer than 4,096 work items, so the map has one byte per grid cell; with offsets 0.5 m (or
0.25 m) apart a patch's 64 points span 3.5 m and the pre-test's box is 2 x 2 cells from the cell of
the patch's first lane.  Three kinds of cell:
  ONE      information 0: the term is exactly 1.0 anywhere in the cell; the map makes no claim
           (level 63) for the cell and its eight neighbours;
  far(e)   isotropic, the mean 2^17 m to the left of the cell: the exponent is e (1 - 6e-5 .. 1)
           over the whole cell, and the byte's level is 63 + ceil(e);
  near(e)  isotropic, the mean 4 m outside the cell's left (or right) edge on the row's mid-line: the
           exponent bound over the cell's box is e (0.998 e after the box's widening), far lower
           inside, and below -62 (level 1) in the cells around it.
Skip levels: a lane whose sum lies in [2^k, 2^(k+1)) skips below T = k ln 2 - 38 and holds level
ceil(T) + 63 (sum 1: 25; sum 3: 26; sum in [2^-28, 2^-27): 6; in [2^-24, 2^-23): 9).
"""
import math

import numpy as np
import pytest

import designed_grids as D

pytestmark = pytest.mark.gpu

C = 4.0
SIZE = 32
FAR = 2.0 ** 17
ULP3 = 2.0 ** -51          # ulp of a sum in [2, 4)


# ---------------------------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------------------------

class Grid:
    def __init__(self):
        self.cells6 = np.zeros((SIZE * SIZE, 6))

    def _put(self, gx, gy, mean, info):
        assert 0 <= gx < SIZE and 0 <= gy < SIZE and self.cells6[gy * SIZE + gx, 5] == 0.0
        self.cells6[gy * SIZE + gx] = (mean[0], mean[1], info[0], info[1], info[2], 5.0)

    def one(self, gx, gy):
        self._put(gx, gy, (C * gx + 2.0, C * gy + 2.0), (0.0, 0.0, 0.0))

    def far(self, gx, gy, e):
        i = 2.0 * -e / (FAR * FAR)
        self._put(gx, gy, (C * gx - FAR, C * gy + 2.0), (i, 0.0, i))

    def near(self, gx, gy, e, side=-1):
        i = 2.0 * -e / 16.0
        self._put(gx, gy, (C * gx - 4.0 if side < 0 else C * gx + 8.0, C * gy + 2.0), (i, 0.0, i))

    @property
    def grid(self):
        return self.cells6, SIZE, SIZE, C, (0.0, 0.0)

    def terms(self, px, py):
        idx = D.get_index(px, py, SIZE, SIZE, C, (0.0, 0.0))
        rec = self.cells6[np.maximum(idx, 0)]
        with np.errstate(under="ignore"):
            term = np.exp(D.record_exponent(rec, np.asarray(px), np.asarray(py)))
        return np.where((idx >= 0) & (rec[:, 5] >= 5.0), term, 0.0)


def expectation(grid, beams, dlin):
    """Scores of one theta step, candidate (ix, iy) at ix * n_lin + iy: the terms added in beam order."""
    n = len(dlin)
    total = np.zeros(n * n)
    for b in beams:
        px, py = D.search_points(b, (0.0, 0.0), 1.0, 0.0, dlin)
        total = total + grid.terms(np.repeat(px, n), np.tile(py, n))
    return -total


def run(grid, beams, dlin, n_th=1):
    from test_gpu_designed_grids import Device
    with Device() as dev:
        dev.install(grid.grid)
        dev.set_search(beams, (0.0, 0.0), dlin, 1.0, 0.0, n_th=n_th)
        lane, lane_name = dev.search("lane")
        noskip, noskip_name = dev.search("lane-noskip")
    return lane, noskip, (lane_name, noskip_name)


# ---------------------------------------------------------------------------------------------
# designed cases: one 8 x 8 patch, 256 beams (four 64-beam chunks), beams uncut
# ---------------------------------------------------------------------------------------------

DLIN8 = (np.arange(8) - 4) * 0.5
NOWHERE = (C * 28 + 2.0, C * 28 + 2.0)          # an empty corner of the grid, empty cells all round


def _beams(placed, dlin):
    """256 beams that end nowhere, except: {beam: (x, y) of the patch's first lane, lane (0, 0)}."""
    beams = np.zeros((256, 2))
    beams[:] = (NOWHERE[0] - dlin[0], NOWHERE[1] - dlin[0])
    for b, (x, y) in placed.items():
        beams[b] = (x - dlin[0], y - dlin[0])
    return beams


def _inside(gx, gy):
    """First lane 0.25 m inside the cell's corner: all 64 lanes (3.5 m) in cell (gx, gy)."""
    return (C * gx + 0.25, C * gy + 0.25)


def case_lone_lane():
    """1.  Beam 0: lane (0, 0) in an empty cell, the other 63 in ONE cells across its corner: sums 1.0,
    level 25, and lane (0, 0) still at level 1.  Beam 64 (second chunk): all lanes in a near(-50.5)
    cell, level 13; lane (0, 0) sits 4.25 m from the mean on its mid-line: exponent -57.0, a term of
    1.7e-25 that IS its sum.  The wave's least level is 1 -- a maximum (25) would prune the beam."""
    g = Grid()
    g.one(5, 4), g.one(4, 5), g.one(5, 5)
    i = 2.0 * 50.5 / 16.0
    g._put(10, 4, (C * 10 - 4.0, C * 4 + 0.25), (i, 0.0, i))
    placed = {0: (C * 4 + 3.75, C * 4 + 3.75), 64: _inside(10, 4)}
    return g, placed


def case_or_of_two_levels():
    """2.  A box of levels 5 and 2 (bounds -58.4 and -61.4; the cells above them: level 1), whose
    bytes OR to level 7.  Beam 0: every lane's sum in [2^-28, 2^-27) -- level 6: the box is kept at
    beam 64 for the OR's sake although no byte reaches the level.  Beam 65: sums in [2^-24, 2^-23) --
    level 9: the same box at beam 128 is pruned.  Its terms (exponents below -140) change nothing."""
    g = Grid()
    g.far(4, 4, -18.9)
    g.far(8, 4, -16.3)
    g.near(12, 4, -58.5, -1)
    g.near(13, 4, -61.5, +1)
    box = (C * 12 + 2.25, C * 4 + 0.25)
    return g, {0: _inside(4, 4), 64: box, 65: _inside(8, 4), 128: box}


def case_rising_threshold():
    """3.  Beams 0 .. 2 (chunk 0): 1.0 each, sums 3.0, level 26.  Chunk 1: far cells at the level
    (exponent -37.5), one below (-38.5: pruned) and one above (-36.005: kept).  The last one's term,
    2.31e-16, is more than half an ulp of 3.0: every sum becomes 3 + 2^-51."""
    g = Grid()
    g.one(4, 4)
    g.far(8, 8, -37.5), g.far(12, 8, -38.5), g.far(16, 8, -36.005)
    return g, {0: _inside(4, 4), 1: _inside(4, 4), 2: _inside(4, 4),
               64: _inside(8, 8), 65: _inside(12, 8), 66: _inside(16, 8)}


def case_no_claim_in_the_box():
    """4.  Sums 3.0 (level 26) as in case 3, then a box of a level 5 cell and a ONE cell (level 63, and
    63 for the cells around it): the beam must stay, the lanes in the ONE cell reach 4.0."""
    g = Grid()
    g.one(4, 4)
    g.near(12, 4, -58.5, -1)
    g.one(13, 4)
    return g, {0: _inside(4, 4), 1: _inside(4, 4), 2: _inside(4, 4), 64: (C * 12 + 2.25, C * 4 + 0.25)}


CASES = {"lone-lane": case_lone_lane, "or-of-two-levels": case_or_of_two_levels,
         "rising-threshold": case_rising_threshold, "no-claim-in-the-box": case_no_claim_in_the_box}


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("case", list(CASES))
def test_designed_levels(case, descending, monkeypatch):
    """The four designed cases, and (5.) the same with a descending offset table: the search then has
    no pre-test at all, and a candidate's score does not depend on where its lane sits."""
    monkeypatch.setenv("NDT2D_LANE_PARTS", "1")
    grid, placed = CASES[case]()
    beams = _beams(placed, DLIN8)
    dlin = DLIN8[::-1].copy() if descending else DLIN8
    want = expectation(grid, beams, dlin)
    lane, noskip, names = run(grid, beams, dlin)
    print("\n%s: kernels %r" % (case, names))
    for name in names:
        assert name.startswith("match/lane-per-candidate/lds-grid") and "beam-parts" not in name, name
    assert np.array_equal(lane, noskip)
    err = float(np.max(np.abs(lane - want)))
    print("%s: max |score - expectation| = %.3e" % (case, err))
    assert err < 1e-9
    # what the design means the candidates to get (candidate (ix, iy) at 8 ix + iy; descending: mirrored)
    got = lane.reshape(8, 8)[::-1, ::-1] if descending else lane.reshape(8, 8)
    if case == "lone-lane":
        term = math.exp(-0.5 * (2.0 * 50.5 / 16.0) * 4.25 * 4.25)
        assert 1e-25 < term < 2e-25
        assert got[0, 0] < 0.0 and abs(got[0, 0] + term) < 1e-12 * term     # exactly the term: nothing else in the sum
        rest = got.ravel()[1:]
        assert np.all(rest == -1.0)
    elif case == "or-of-two-levels":
        s = math.exp(-18.9) + math.exp(-16.3)
        assert np.all(np.abs(got + s) < 2e-3 * s)           # (a far cell's exponent varies by 6e-5 of itself)
        assert 2.0 ** -28 < math.exp(-18.9) * (1 - 2e-3) and math.exp(-18.9) < 2.0 ** -27
        assert 2.0 ** -24 < s * (1 - 2e-3) and s < 2.0 ** -23
    elif case == "rising-threshold":
        assert np.all(got == -(3.0 + ULP3))
    else:
        assert np.all(got[:4] == -3.0) and np.all(got[4:] == -4.0)


# ---------------------------------------------------------------------------------------------
# lattices and kernel forms on one scene
# ---------------------------------------------------------------------------------------------

def scene(n_beams, seed=7):
    """A third of the cells isotropic with the mean inside the cell and exponents of 0 .. -90 at the
    cell's far corner (levels 1 .. 63 over the sub-boxes a patch meets); a few ONE cells; the first
    four beams on ONE cells, so that every lane scores at once and its level rises above the lowest;
    the other beams uniformly over the grid's middle."""
    rng = np.random.default_rng(seed)
    g = Grid()
    for gy in range(4, 28):
        for gx in range(4, 28):
            u = rng.random()
            if 12 <= gx < 16 and 12 <= gy < 16:
                g.one(gx, gy)
            elif u < 0.33:
                e = -rng.uniform(0.5, 90.0)
                mean = (C * gx + rng.uniform(-6.0, 10.0), C * gy + rng.uniform(-6.0, 10.0))
                i = 2.0 * -e / 16.0
                g._put(gx, gy, mean, (i, 0.0, i * rng.uniform(0.5, 2.0)))
            elif u < 0.35:
                g.one(gx, gy)
    beams = np.zeros((n_beams, 2))
    beams[:, 0] = np.round(rng.uniform(C * 6, C * 26, n_beams) * 64.0) / 64.0
    beams[:, 1] = np.round(rng.uniform(C * 6, C * 26, n_beams) * 64.0) / 64.0
    beams[:4] = (C * 14, C * 14)
    return g, beams


# form: (n_lin, theta steps or None = more items than four waves a CU hold, beams, NDT2D_LANE_PARTS,
#        NDT2D_LANE_RECORDS, what the kernel's name must hold, strip tiles)
FORMS = {
    "one-patch": (8, 1, 512, "1", None, "lds-grid", False),
    "four-patches": (16, 2, 512, "1", None, "lds-grid", False),
    "strip-tiles": (12, 3, 512, "1", None, "lds-grid", True),
    "beam-parts": (32, 3, 1024, None, None, "lds-grid/compact-records/beam-parts", False),
    "gather6-beam-parts": (32, 3, 1024, None, "global", "lds-map+global-records/beam-parts", False),
    "six-wave-compact": (32, None, 512, "1", None, "lds-grid/compact-records/pow2", False),
    "six-wave-compact-strips": (33, None, 512, "1", None, "lds-grid/compact-records/pow2", True),
}

_scenes = {}


@pytest.mark.parametrize("form", list(FORMS))
def test_lattices_and_kernel_forms(form, monkeypatch):
    n_lin, n_th, n_beams, parts, records, in_name, strips = FORMS[form]
    for key, value in (("NDT2D_LANE_PARTS", parts), ("NDT2D_LANE_RECORDS", records)):
        if value is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, value)
    if n_th is None:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        p1 = (n_lin + 7) // 8
        n_th = 4 * cus // (p1 * p1) + 1
        assert 4 * cus < n_th * p1 * p1 < 4096
    if n_beams not in _scenes:
        _scenes[n_beams] = scene(n_beams)
    grid, beams = _scenes[n_beams]
    dlin = (np.arange(n_lin) - n_lin // 2) * 0.25
    key = (n_beams, n_lin)
    if key not in _scenes:
        _scenes[key] = expectation(grid, beams, dlin)
    want = _scenes[key]
    lane, noskip, names = run(grid, beams, dlin, n_th=n_th)
    print("\n%s: n_lin %d, %d theta steps, %d beams, kernels %r" % (form, n_lin, n_th, n_beams, names))
    for name in names:
        assert name.startswith("match/lane-per-candidate/") and in_name in name, name
        assert ("beam-parts" in name) == ("beam-parts" in in_name), name
    assert (n_lin % 8 in (1, 2, 3, 4)) == strips
    assert np.array_equal(lane, noskip)
    per = n_lin * n_lin
    for t in range(n_th):
        assert np.array_equal(lane[t * per:(t + 1) * per], lane[:per]), t
    err = float(np.max(np.abs(lane[:per] - want)))
    # the scene does what it is for: every candidate scores with the first beams, and sums differ
    assert np.all(lane[:per] <= -4.0) and len(np.unique(lane[:per])) > per // 2
    print("%s: max |score - expectation| = %.3e, scores %.3f .. %.3f" % (form, err, lane[:per].min(), lane[:per].max()))
    assert err < 1e-9
