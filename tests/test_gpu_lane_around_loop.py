"""The work around the beam loop of the large lane search (csrc/ndt2d_match_lane.hip): the block's
start-up copies of the rank table, the compacted records and the map image, the table
pre-kernel's two-dimensional launch with the map image in blocks of its own, and the item
epilogue's transposed reduction of the ten sums (wave_ten_sums_to_rows, csrc/ndt2d_device_fn.h).

Every launch here is the smallest that still takes match_lane_compact_kernel<false> / <true>: at
least 256 beams (the dynamic-item forms), more than 4 x CU count patches (beyond the 256-thread
form), NDT2D_LANE_PARTS=1 (the beams are not cut into parts), the 41 x 41 cfg-1 map or grids of
its size installed through ndt2d_set_grid.  Lattice steps are powers of two, so that
`for (v = -size; v < size; v += res)` takes exactly n steps.

Tolerances.  Scores: 1e-9 of the oracle, as every parity test of the lane search has it, and
bit-equal to the unskipped control.  The ten sums: 1e-12 relative of math.fsum over the returned
scores times their monomials -- a sum of n terms added along any tree of depth d differs from
the exact sum by at most d * 2^-53 * sum |term|; here d < 40 (six wave levels, the slab's
records, the final reduction) and the terms of every asserted sum either share a sign or, for
the odd monomials, cancel by no more than a factor of a few hundred.
"""
import math

import numpy as np
import pytest

import oracle_lib as O
from ndt_2d_amd import ScanMatcherNDT, _capi, host_build_grid, synth
from ndt_2d_amd import dist as shard

pytestmark = pytest.mark.gpu

RES = 2.0 ** -6
ANG_RES = 2.0 ** -10
CELL = 0.25

_cache = {}


@pytest.fixture(autouse=True)
def _unsplit(monkeypatch):
    monkeypatch.setenv("NDT2D_LANE_PARTS", "1")


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _steps_for(n_lin, more=1):
    """Theta steps that give a launch more than `more` x 4 x CU count patches of 8 x 8 (even: 0 is a step)."""
    p1 = (n_lin + 7) // 8
    n = more * 4 * _cus() // (p1 * p1) + 2
    return n + (n & 1)


def _cfg1_grid():
    if "grid" not in _cache:
        cells, sx, sy, ox, oy = host_build_grid(CELL, synth.CONFIGS[1]["range_max"], synth.map_scans(1))
        assert (sx, sy) == (41, 41)
        _cache["grid"] = (np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 6), sx, sy, ox, oy)
    return _cache["grid"]


def _grid_with(n_occ):
    """The cfg-1 records with exactly n_occ cells that hold a distribution (n >= 5): the first n_occ
    of the map's own 236, or all of them plus copies of a neighbour's record, its mean moved along,
    in empty cells next to occupied ones."""
    cells, sx, sy, ox, oy = _cfg1_grid()
    out = cells.copy()
    occupied = np.flatnonzero(out[:, 5] >= 5.0)
    assert len(occupied) == 236
    if n_occ <= len(occupied):
        out[occupied[n_occ:], 5] = 0.0
    else:
        todo = n_occ - len(occupied)
        for cell in occupied:
            cx, cy = int(cell % sx), int(cell // sx)
            if todo and cx + 1 < sx and out[cell + 1, 5] < 5.0:
                out[cell + 1] = out[cell]
                out[cell + 1, 0] += CELL
                todo -= 1
        assert todo == 0
    assert int((out[:, 5] >= 5.0).sum()) == n_occ
    return out


def _nan_launch(gpu, launch, n):
    import torch
    d = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    launch(d.data_ptr())
    gpu.synchronize()
    rec = gpu.match_fetch()
    variant = gpu.last_variant()
    assert "lane-per-candidate" in variant and "beam-parts" not in variant, variant
    return d.cpu().numpy(), rec, variant


def _case(key, n_lin, n_th, cells=None, extra_scans=(), guess=None, pts=None):
    """One matcher, its skip and no-skip launches and the oracle's scores, shared by the tests."""
    if key in _cache:
        return _cache[key]
    params = synth.matcher_params(1, search_linear_size=n_lin * RES / 2, search_linear_resolution=RES,
                                  search_angular_size=n_th * ANG_RES / 2, search_angular_resolution=ANG_RES)
    scans = synth.map_scans(1) + list(extra_scans)
    q_guess, q_pts, _ = synth.query_scan(1)
    guess = q_guess if guess is None else guess
    pts = q_pts if pts is None else pts
    gpu = ScanMatcherNDT(0)
    gpu.initialize("around", **params)
    gpu.addScans(scans)
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    if cells is None:
        ref.addScans(scans)
    else:
        _, sx, sy, ox, oy = _cfg1_grid()
        assert _capi.lib().ndt2d_set_grid(gpu.device_handle, _capi.dptr(np.ascontiguousarray(cells)), sx, sy, CELL,
                                          ox, oy) == _capi.OK
        ref.setCells6(cells, sx, sy, CELL, (ox, oy))
    exp = ref.matchScan(guess, pts, want_scores=True, omp_threads=8)
    assert gpu.prepare_search(guess, pts) == (n_th, n_lin, len(pts))
    c = dict(gpu=gpu, n_lin=n_lin, n_th=n_th, per=n_lin * n_lin, oracle=exp["scores"], oracle_best=exp["best_index"],
             dlin=O.search_offsets(n_lin * RES / 2, RES), dth=O.search_offsets(n_th * ANG_RES / 2, ANG_RES))
    assert len(c["dlin"]) == n_lin and len(c["dth"]) == n_th
    gpu.set_variant("lane")
    c["scores"], c["record"], c["variant"] = _nan_launch(
        gpu, lambda p: gpu.match_launch(0, n_th, scores_ptr=p), n_th * c["per"])
    gpu.set_variant("lane-noskip")
    c["noskip"], c["noskip_record"], _ = _nan_launch(
        gpu, lambda p: gpu.match_launch(0, n_th, scores_ptr=p), n_th * c["per"])
    gpu.set_variant("lane")
    _cache[key] = c
    return c


def _check_scores(c, compact=True):
    if compact:
        assert "compact-records" in c["variant"], c["variant"]
    assert not np.isnan(c["scores"]).any() and not np.isnan(c["noskip"]).any()
    assert np.array_equal(c["scores"], c["noskip"])
    finite = np.isfinite(c["oracle"])
    assert np.array_equal(np.isneginf(c["scores"]), np.isneginf(c["oracle"]))
    err = float(np.max(np.abs(c["scores"][finite] - c["oracle"][finite])))
    print("max |score - oracle| = %.3e over %d candidates" % (err, len(c["scores"])))
    assert err < 1e-9


def _monomial_terms(c, s):
    n_lin, n_th = c["n_lin"], c["n_th"]
    dt = np.repeat(c["dth"], n_lin * n_lin)
    dx = np.tile(np.repeat(c["dlin"], n_lin), n_th)
    dy = np.tile(c["dlin"], n_th * n_lin)
    with np.errstate(invalid="ignore"):
        return [(dx * dx) * s, (dx * dy) * s, (dx * dt) * s, (dy * dy) * s, (dy * dt) * s, (dt * dt) * s,
                dx * s, dy * s, dt * s, s]


def _near_tie_expected(s):
    """merge_best's rule: the winner is marked iff another real candidate lies within 2^-36 (relative)."""
    best = s.min()
    if not best < 0.0:
        return False
    first = int(np.argmin(s))
    with np.errstate(invalid="ignore"):
        close = (np.ldexp(np.abs(s - best), 36) <= np.maximum(np.abs(s), abs(best))) & (s < 0.0)
    close[first] = False
    return bool(close.any())


def _check_record(c, rec):
    s = c["scores"]
    if not (s < 0.0).any():
        assert rec[0] == 0.0 and rec[1] == -1.0 and not rec[2:].any()
        return
    assert rec[0] == s.min() and math.floor(rec[1]) == int(np.argmin(s))   # (argmin: the first of equals)
    assert (rec[1] != math.floor(rec[1])) == _near_tie_expected(s)
    for k, term in enumerate(_monomial_terms(c, s)):
        if not np.isfinite(term).all():
            # a -inf score: the sums are -inf, +inf or NaN as the terms have it
            with np.errstate(invalid="ignore"):
                want = float(np.sum(term))
            assert (math.isnan(rec[2 + k]) and math.isnan(want)) or rec[2 + k] == want, (k, rec[2 + k], want)
            continue
        want = math.fsum(term)
        rel = abs(rec[2 + k] - want) / abs(want) if want != 0.0 else abs(rec[2 + k])
        print("acc[%d]: got %.17g want %.17g rel %.2e" % (k, rec[2 + k], want, rel))
        assert abs(rec[2 + k] - want) <= 1e-12 * abs(want), (k, rec[2 + k], want)


# -- staging ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_occ", [1, 255, 256, 257, "cfg1"])
def test_staged_image_whatever_the_number_of_records(n_occ):
    """The compacted records number 3 (n_occ + 1) units of 16 bytes: 6, exactly one pass of the
    768-thread block (768), one unit more than a pass (771), 774 -- and the cfg-1 map as addScans
    builds it, just under a pass (236 cells hold a distribution: 711 units)."""
    cells = None if n_occ == "cfg1" else _grid_with(n_occ)
    c = _case("occ%s" % n_occ, 20, _steps_for(20), cells=cells)
    _check_scores(c)
    assert (c["scores"] < 0).any()
    _check_record(c, c["record"])


def test_staged_map_at_its_finest_resolution():
    """From 4,096 patches on the map is kept at 4 x 4 sub-cells per cell: 196 rows of 256 bytes where the
    launches above stage 49 (the two map heights this grid and lattice give)."""
    n_lin = 20
    p1 = (n_lin + 7) // 8
    n_th = 4096 // (p1 * p1) + 2
    c = _case("fine", n_lin, n_th + (n_th & 1))
    _check_scores(c)
    _check_record(c, c["record"])


# -- table pre-kernel ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_beams", [257, 300])
def test_table_rows_of_shares_and_slabs(n_beams, monkeypatch):
    """Beams that do not fill their last block of 256, theta steps taken from a non-zero first step
    with stride 1 and 8, and three slabs the last of which is shorter: the same scores as the
    whole launch, and the combined record names the oracle's winner."""
    n_lin = 9                      # 4 patches a theta step: every share below still takes the compact kernel
    n_th = 8 * _steps_for(n_lin)
    _, pts, _ = synth.query_scan(1)
    c = _case("table%d" % n_beams, n_lin, n_th, pts=pts[:n_beams])
    _check_scores(c)
    gpu, per = c["gpu"], c["per"]
    assert math.floor(c["record"][1]) == c["oracle_best"]
    whole = shard.combine_match_records([c["record"]])
    # stride 1: [0, k) and [k, n_th)
    k = n_th // 2 + 3
    records = []
    for first, last in ((0, k), (k, n_th)):
        got, rec, variant = _nan_launch(gpu, lambda p: gpu.match_launch(first, last, scores_ptr=p), (last - first) * per)
        assert "compact-records" in variant
        assert np.array_equal(got, c["scores"][first * per:last * per])
        records.append(rec)
    best_score, best_index, acc = shard.combine_match_records(records)
    assert (best_score, best_index) == whole[:2] and best_index == c["oracle_best"]
    assert np.allclose(acc, whole[2], rtol=1e-11, atol=0)
    # stride 8, every first step
    records = []
    for rank in range(8):
        first, stride, count = shard.shard_strided(n_th, rank, 8)
        assert stride == 8 and first == rank
        got, rec, variant = _nan_launch(
            gpu, lambda p: gpu.match_launch_strided(first, stride, count, scores_ptr=p), count * per)
        assert "compact-records" in variant
        mine = np.concatenate([c["scores"][t * per:(t + 1) * per] for t in range(first, n_th, stride)])
        assert np.array_equal(got, mine)
        records.append(rec)
    best_score, best_index, acc = shard.combine_match_records(records)
    assert (best_score, best_index) == whole[:2] and best_index == c["oracle_best"]
    assert np.allclose(acc, whole[2], rtol=1e-11, atol=0)
    # three slabs, the last one shorter
    p1 = (n_lin + 7) // 8
    slab_th = (n_th * 2 + 4) // 5
    assert 2 * slab_th < n_th < 3 * slab_th
    monkeypatch.setenv("NDT2D_LANE_SLAB_ITEMS", str(slab_th * p1 * p1))
    got, rec, variant = _nan_launch(gpu, lambda p: gpu.match_launch(0, n_th, scores_ptr=p), n_th * per)
    assert "compact-records" in variant
    assert np.array_equal(got, c["scores"])
    assert (rec[0], rec[1]) == (c["record"][0], c["record"][1])
    assert np.allclose(rec[2:], c["record"][2:], rtol=1e-11, atol=0)


# -- item epilogue ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lin", [16, 17, 18, 19, 20])
def test_ten_sums_of_every_tile_shape(n_lin):
    """8 x 8 tiles only (16), then strips of 1 x 64, 2 x 32, 4 x 16 and 4 x 16 whose last tiles
    have shadow lanes."""
    c = _case("sums%d" % n_lin, n_lin, _steps_for(n_lin))
    _check_scores(c)
    for rec in (c["record"], c["noskip_record"]):
        _check_record(c, rec)


T_HIT = 40   # theta step, counted from the middle one, at which the one-cell case's beam points along x


def _one_cell_case(target):
    """One cell that holds a distribution, so narrow (information 2^27) that a point 2^-6 m from its
    mean scores exp(-16384) = 0, and 256 beams of which only the first can reach it: at the theta
    step where the beam's heading is exactly 0 exactly ONE candidate scores, (target, target) -- lane 0 or lane 63 of the first
    tile -- and with it exactly -1.  Every other item of that step, and most of the others, holds
    no candidate that scores."""
    n_lin, n_th = 16, _steps_for(16)
    _, sx, sy, ox, oy = _cfg1_grid()
    cells = np.zeros((sx * sy, 6))
    cx = cy = 20
    dlin = O.search_offsets(n_lin * RES / 2, RES)
    # the robot on a multiple of 2^-6 m, the mean where beam 0 of candidate (target, target) ends: every sum
    # that forms that point is exact, and the mean lies within 2^-6 m of the cell's centre
    gx = math.floor((ox + (cx + 0.5) * CELL - dlin[target] - 1.0) * 64.0) / 64.0
    gy = math.floor((oy + (cy + 0.5) * CELL - dlin[target]) * 64.0) / 64.0
    mean = (gx + 1.0 + dlin[target], gy + dlin[target])
    assert int((mean[0] - ox) / CELL) == cx and int((mean[1] - oy) / CELL) == cy
    cells[cy * sx + cx] = [mean[0], mean[1], 2.0 ** 27, 0.0, 2.0 ** 27, 5.0]
    # (the scan's heading is minus the offset of step T_HIT, not of the middle step: the scores are
    # symmetric about the step that hits, and sums odd in the angle offset would cancel to nothing there)
    dth = O.search_offsets(n_th * ANG_RES / 2, ANG_RES)
    guess = (gx, gy, -dth[n_th // 2 + T_HIT])
    pts = np.zeros((256, 2))
    pts[0] = (1.0, 0.0)
    pts[1:, 0] = -1.0 - np.arange(255) * 2.0 ** -7      # behind the robot, in cells that hold nothing
    c = _case("one%d" % target, n_lin, n_th, cells=cells, guess=guess, pts=pts)
    return c, n_lin, n_th


@pytest.mark.parametrize("target", [0, 7])
def test_items_without_a_score_and_with_one_in_the_first_or_last_lane(target):
    c, n_lin, n_th = _one_cell_case(target)
    _check_scores(c)
    s = c["scores"].reshape(n_th, n_lin, n_lin)
    t0 = n_th // 2 + T_HIT
    assert c["dth"][t0] == T_HIT * ANG_RES
    here = np.argwhere(s[t0] != 0.0)
    assert here.tolist() == [[target, target]] and s[t0, target, target] == -1.0
    # items none of whose candidates scores: every other patch of this step, and whole steps far from it
    assert not s[t0, 8:, :].any() and not s[t0, :, 8:].any()
    assert any(not s[t].any() for t in range(n_th))
    for rec in (c["record"], c["noskip_record"]):
        _check_record(c, rec)
        assert rec[0] == -1.0 and math.floor(rec[1]) == (t0 * n_lin + target) * n_lin + target


def test_one_score_of_minus_infinity():
    """The overflow cell of tests/test_gpu_overflow_cell.py inside the cfg-1 map: the -inf scores
    force the winner (the first of them in visiting order), and the sums are what IEEE makes of them."""
    from test_gpu_overflow_cell import overflow_cell_point
    x, y = overflow_cell_point()
    bad = ((0.0, 0.0, 0.0), np.tile([[x, y]], (6, 1)))
    c = _case("inf", 20, _steps_for(20), extra_scans=[bad])
    _check_scores(c)
    assert np.isneginf(c["scores"]).any() and not np.isneginf(c["scores"]).all()
    for rec in (c["record"], c["noskip_record"]):
        assert rec[0] == -np.inf and math.floor(rec[1]) == int(np.argmax(np.isneginf(c["scores"])))
        assert math.floor(rec[1]) == c["oracle_best"]
        _check_record(c, rec)
