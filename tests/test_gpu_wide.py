"""Wide search (csrc/wide/, ndt2d_wide_match): the exhaustive lattice's winner by tile bounds.

The yardstick throughout is ndt2d_starts_match with ONE start and all_scores on the same installed
grid, beams, dth and dlin: best_score bit for bit, the same index and the same near-tie mark; every
tile job's bound at least the largest raw sum inside its window; every job left out below
best_sum (1 - 2^-35).  The bound image is compared with the numpy restatement
(tests/wide_restatement.py) on a designed grid."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import designed_grids as D
import offgrid_cases
import oracle_lib as O
import wide_restatement as W
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, WideSearch, _capi, search_offsets, synth
from test_wide_restatement import LATTICE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_MAX = synth.CONFIGS[1]["range_max"]
NO_INDEX = 2 ** 64 - 1
STOP = 1.0 - 2.0 ** -35
# (linear size, linear resolution, tile steps): n_lin = 40 with T = 2, 4, 8; n_lin = 21 with T = 8
# (ragged tiles) and with T >= n_lin (one tile per theta step)
LATTICES = [(0.395, 0.02, 2), (0.395, 0.02, 4), (0.395, 0.02, 8), (0.205, 0.02, 8), (0.205, 0.02, 32)]
N_LIN = {0.395: 40, 0.205: 21}


def _matcher(resolution):
    m = ScanMatcherNDT(0)
    m.initialize("wide", ndt_resolution=resolution, range_max=RANGE_MAX)
    m.addScans(synth.map_scans(1))
    return m


def _yardstick(m, pose, beams, dth, dlin):
    """ndt2d_starts_match, one start, all_scores: (record[12], scores[n_th * n_lin * n_lin])."""
    L = _capi.lib()
    obj = C.c_void_p()
    assert L.ndt2d_starts_create(m.device_handle, 1, C.byref(obj)) == _capi.OK
    try:
        st = np.ascontiguousarray(pose, dtype=np.float64).reshape(1, 3)
        b = np.ascontiguousarray(beams, dtype=np.float64)
        record = np.zeros(12)
        scores = np.zeros(len(dth) * len(dlin) * len(dlin))
        rc = L.ndt2d_starts_match(obj, _capi.dptr(st), 1, _capi.dptr(b), len(b), _capi.dptr(dth), len(dth), _capi.dptr(dlin),
                                  len(dlin), _capi.dptr(record), _capi.dptr(scores))
        assert rc == _capi.OK, L.ndt2d_starts_last_error(obj)
        return record, scores
    finally:
        L.ndt2d_starts_destroy(obj)


def _same_record(got, record):
    """best_score bit for bit, the index and the mark."""
    assert int(got["record"][0:1].view(np.uint64)[0]) == int(record[0:1].view(np.uint64)[0]), (got["record"], record[:2])
    assert np.floor(got["record"][1]) == np.floor(record[1]), (got["record"], record[:2])
    assert got["record"][1] == record[1], (got["record"], record[:2])          # the near-tie mark too


def _dominance(got, scores, n_th, n_lin, tile_steps):
    with np.errstate(invalid="ignore"):
        best_in_tile = W.tile_maxima(-scores, n_th, n_lin, tile_steps)
    assert got["bounds"].shape == best_in_tile.shape == got["evaluated"].shape
    assert np.all(got["bounds"] >= best_in_tile)
    left_out = got["evaluated"] == 0
    assert np.all(got["bounds"][left_out] < -got["best_score"] * STOP)
    assert int(got["evaluated"].sum()) == got["tiles_scored"] and got["tiles_total"] == best_in_tile.size
    assert set(np.unique(got["evaluated"]).tolist()) <= {0, 1}


def _beams(kind, cell):
    """3, 100 or 1,030 beams of cfg-1's world seen from its query's true pose, NaN and off-grid
    points among them (offgrid_cases).  1,030: past kStageBeams, no multiple of four, C = 8."""
    guess, points, truth = synth.query_scan(1)
    if kind == 1030:
        beams = synth.scan(synth.world_of(1), truth, 4242, n_beams=1030)
    else:
        beams = W.subsample(points, 100)
    beams = np.array(beams, dtype=np.float64)
    bad = offgrid_cases.off_grid_points(cell, RANGE_MAX)
    if kind == 3:
        beams = beams[[10, 50, 90]]
        beams[1] = (offgrid_cases.NAN, beams[1, 1])
        return beams
    for i, (x, y, _) in enumerate(bad):
        beams[(7 * i + 3) % len(beams)] = (x, y)
    return beams


@pytest.mark.parametrize("n_beams", [3, 100, 1030])
@pytest.mark.parametrize("resolution", [0.25, 0.1])
def test_record_and_dominance_against_the_exhaustive_search(resolution, n_beams):
    """The cfg-1 grid (41 x 41, power-of-two cells) and a 0.1 m-cell grid (the true divide)."""
    m = _matcher(resolution)
    assert m.grid()[1:3] == ((41, 41) if resolution == 0.25 else (101, 101))
    pose = np.array(synth.query_scan(1)[0], dtype=np.float64)
    beams = _beams(n_beams, resolution)
    assert len(beams) == n_beams
    wide = WideSearch(m, max_tiles=256)
    for angular in ((0.001, 0.002), (0.045, 0.02)):             # n_th = 1 and 5
        dth = search_offsets(*angular)
        for size, res, tile_steps in LATTICES:
            dlin = search_offsets(size, res)
            assert len(dth) in (1, 5) and len(dlin) == N_LIN[size]
            record, scores = _yardstick(m, pose, beams, dth, dlin)
            wide.set_tile(tile_steps=tile_steps)
            got = wide.match(pose, beams, dth, dlin, want_bounds=True)
            print("cells %.2f, %d beams, n_th %d, n_lin %d, T %d: score %.17g index %r, %d of %d tiles"
                  % (resolution, n_beams, len(dth), len(dlin), tile_steps, got["best_score"], got["record"][1],
                     got["tiles_scored"], got["tiles_total"]))
            _same_record(got, record)
            _dominance(got, scores, len(dth), len(dlin), tile_steps)
            assert got["tiles_total"] == len(dth) * (-(-len(dlin) // tile_steps)) ** 2
            if n_beams >= 100:
                assert record[0] < 0.0 and got["best_index"] >= 0
    wide.close()


def _designed_cells():
    """6 x 5 cells of 0.25 m at (-0.7, 0.3): records made by designed_grids.records_for (isotropic
    and rank-1), an ordinary correlated cell, a cell whose eigenvalue the reference clamps, a NaN
    cell and a cell with n = 4; the rest empty."""
    size_x, size_y, cell, origin = 6, 5, 0.25, (-0.7, 0.3)
    cells = np.zeros((size_x * size_y, 6))

    def centre(cx, cy, fx=0.5, fy=0.5):
        return origin[0] + (cx + fx) * cell, origin[1] + (cy + fy) * cell

    iso = D.records_for(np.array([-40.0, -3.5]), 0.0, 0.0, "iso")
    rank1 = D.records_for(np.array([-12.0, 2.0]), 0.0, 0.0, "rank1")
    for rec, (cx, cy, fx, fy) in zip(list(iso) + list(rank1), [(0, 0, 0.3, 0.6), (2, 1, 0.9, 0.1), (4, 3, 0.5, 0.5), (1, 3, 0.2, 0.8)]):
        rec[0], rec[1] = centre(cx, cy, fx, fy)
        cells[cy * size_x + cx] = rec
    cells[2 * size_x + 3] = (*centre(3, 2, 0.4, 0.7), 310.0, -45.0, 120.0, 9.0)
    # six nearly collinear points: Cell::compute clamps the small eigenvalue (src/ndt_model.cpp:88-96)
    c = O.Cell()
    x0, y0 = centre(5, 0, 0.1, 0.5)
    for k in range(6):
        c.addPoint(x0 + 0.03 * k, y0 + 1e-7 * (k % 2))
    c.compute()
    info = np.asarray(c.information, dtype=np.float64).reshape(2, 2)
    mean = np.asarray(c.mean, dtype=np.float64).reshape(2)
    cells[0 * size_x + 5] = (mean[0], mean[1], info[0, 0], info[0, 1], info[1, 1], 6.0)
    cells[4 * size_x + 0] = (float("nan"), centre(0, 4)[1], 100.0, 0.0, 100.0, 12.0)
    cells[4 * size_x + 2] = (*centre(2, 4), 200.0, 0.0, 200.0, 4.0)
    return cells, size_x, size_y, cell, origin


@pytest.mark.parametrize("tile_steps,pixels_per_tile", [(4, 1), (8, 2), (3, 4)])
def test_the_image_is_the_restatements(tile_steps, pixels_per_tile):
    cells, size_x, size_y, cell, origin = _designed_cells()
    info = cells[5, 2:5]
    assert max(abs(info)) > 500.0 * min(abs(info[0]), abs(info[2]))          # the clamped cell is ill-conditioned
    m = ScanMatcherNDT(0)
    m.initialize("designed", ndt_resolution=cell, range_max=RANGE_MAX)
    c6 = np.ascontiguousarray(cells)
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(c6), size_x, size_y, cell, origin[0], origin[1]) == _capi.OK
    wide = WideSearch(m)
    wide.set_tile(tile_steps, pixels_per_tile)
    dlin, dth = search_offsets(0.1, 0.01), search_offsets(0.001, 0.002)
    beams = np.array([[0.1, 0.9], [0.4, 0.5]])
    got = wide.match((0.0, 0.0, 0.0), beams, dth, dlin, want_bounds=True)
    g, raw, data = W.image(cells, size_x, size_y, cell, origin, W.window_of(dlin, tile_steps), pixels_per_tile)
    info, image = wide.read_image()
    for key in ("nx", "ny", "origin_x", "origin_y", "pitch", "window", "guard"):
        assert info[key] == g[key], key
    assert image.shape == data.shape == (g["ny"], g["nx"])
    assert np.all(np.isfinite(image)) and image.max() > 1.0 and (image == 0.0).any()
    assert np.all(np.abs(image - data) <= 1e-12 * data)                     # 1e-12 relative
    assert np.all(image >= raw)                                             # never below the uninflated value
    # the bounds are the restatement's too (sums of a few pixels in another order)
    bounds = W.tile_bounds(g, image, (0.0, 0.0, 0.0), beams, dth, dlin, tile_steps)
    assert np.allclose(got["bounds"], bounds, rtol=1e-14, atol=0.0)
    record, scores = _yardstick(m, (0.0, 0.0, 0.0), beams, dth, dlin)
    _same_record(got, record)
    _dominance(got, scores, len(dth), len(dlin), tile_steps)
    wide.close()


def test_designed_tie_across_tiles():
    """Two cells with identical records exactly 0.25 m apart, one beam, dyadic offsets: candidates
    (dx, dy) = (0, 0) and (0.25, 0) hit the two means exactly and score bit-equal -1.0 in different
    tiles, scored in different rounds (one tile a round).  The lower flat index wins, marked."""
    size_x, size_y, cell = 8, 2, 0.25
    dlin = np.arange(-4, 8, dtype=np.float64) / 16.0
    dth = np.zeros(1)
    beam = np.array([[0.375, 0.125]])
    m = ScanMatcherNDT(0)
    m.initialize("tie", ndt_resolution=cell, range_max=RANGE_MAX)
    wide = WideSearch(m, max_tiles=1)
    wide.set_tile(2, 2)
    for second in (True, False):
        cells = np.zeros((size_x * size_y, 6))
        cells[1] = (0.375, 0.125, 200.0, 0.0, 200.0, 5.0)
        if second:
            cells[2] = (0.625, 0.125, 200.0, 0.0, 200.0, 5.0)
        assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), size_x, size_y, cell, 0.0, 0.0) == _capi.OK
        record, scores = _yardstick(m, (0.0, 0.0, 0.0), beam, dth, dlin)
        s = scores.reshape(12, 12)
        assert s[4, 4] == -1.0 and (s[8, 4] == -1.0) == second and np.sum(s == -1.0) == (2 if second else 1)
        got = wide.match((0.0, 0.0, 0.0), beam, dth, dlin, want_bounds=True)
        _same_record(got, record)
        assert got["best_score"] == -1.0 and got["best_index"] == 4 * 12 + 4
        assert got["near_tie"] == second and (record[1] != np.floor(record[1])) == second
        assert got["evaluated"][0, 2, 2] == 1 and got["evaluated"][0, 4, 2] == (1 if second else 0)
        _dominance(got, scores, 1, 12, 2)
    wide.close()


def test_a_map_without_cells_scores_every_tile():
    m = ScanMatcherNDT(0)
    m.initialize("empty", ndt_resolution=0.25, range_max=RANGE_MAX)
    cells = np.zeros((12 * 9, 6))
    assert _capi.lib().ndt2d_set_grid(m.device_handle, _capi.dptr(cells), 12, 9, 0.25, -1.0, -1.0) == _capi.OK
    wide = WideSearch(m, max_tiles=100)
    wide.set_tile(8, 2)
    dlin, dth = search_offsets(0.205, 0.02), search_offsets(0.045, 0.02)
    beams = W.subsample(synth.query_scan(1)[1], 100)
    got = wide.match((0.2, 0.1, 0.3), beams, dth, dlin, want_bounds=True)
    assert got["best_index"] == -1 and got["record"][1] == -1.0 and got["best_score"] == 0.0 and not got["near_tie"]
    assert got["tiles_scored"] == got["tiles_total"] == 5 * 3 * 3 and np.all(got["evaluated"] == 1) and np.all(got["bounds"] == 0.0)
    record, _ = _yardstick(m, (0.2, 0.1, 0.3), beams, dth, dlin)
    _same_record(got, record)
    wide.close()


def test_pruning_determinism_and_the_kept_image():
    """The CPU test's case (tests/test_wide_restatement.py): fewer than half the tiles are scored."""
    m = _matcher(0.25)
    pose, points = synth.query_scan(1)[:2]
    beams = W.subsample(points, 100)
    dth = search_offsets(LATTICE["search_angular_size"], LATTICE["search_angular_resolution"])
    dlin = search_offsets(LATTICE["search_linear_size"], LATTICE["search_linear_resolution"])
    wide = WideSearch(m)
    wide.set_tile(2, 2)
    a = wide.match(pose, beams, dth, dlin, want_bounds=True)
    print("tiles scored %d of %d" % (a["tiles_scored"], a["tiles_total"]))
    assert a["tiles_total"] == 40 * 20 * 20 and a["tiles_scored"] < a["tiles_total"] / 2
    record, scores = _yardstick(m, pose, beams, dth, dlin)
    _same_record(a, record)
    _dominance(a, scores, 40, 40, 2)
    b = wide.match(pose, beams, dth, dlin, want_bounds=True)
    kept = wide.match(pose, beams, dth, dlin, reuse_image=True, want_bounds=True)
    for other in (b, kept):
        assert np.array_equal(other["record"].view(np.uint64), a["record"].view(np.uint64))
        assert np.array_equal(other["evaluated"], a["evaluated"])
        assert np.array_equal(other["bounds"].view(np.uint64), a["bounds"].view(np.uint64))
    # the stages can be timed, and timing changes nothing
    wide.set_timing(True)
    timed = wide.match(pose, beams, dth, dlin, reuse_image=True)
    assert np.array_equal(timed["record"].view(np.uint64), a["record"].view(np.uint64))
    ms = wide.last_ms()
    print("image %.3f ms (kept), bounds %.3f, sort %.3f, exact rounds %.3f" % ms)
    assert len(ms) == 4 and all(v >= 0.0 for v in ms)
    wide.close()


def test_match_wide_is_the_c_calls_record():
    m = _matcher(0.25)
    pose, points = synth.query_scan(1)[:2]
    dth = search_offsets(LATTICE["search_angular_size"], LATTICE["search_angular_resolution"])
    dlin = search_offsets(LATTICE["search_linear_size"], LATTICE["search_linear_resolution"])
    wide = WideSearch(m)
    wide.set_tile(tile_steps=2)
    want = wide.match(pose, W.subsample(points, 100), dth, dlin)
    wide.close()
    before = m.matchScan(pose, points)
    for call in range(2):                                           # the second call keeps the image
        got = m.matchWide(pose, points, LATTICE["search_linear_size"], LATTICE["search_linear_resolution"],
                          LATTICE["search_angular_size"], LATTICE["search_angular_resolution"], tile_steps=2)
        assert got["score"] == want["best_score"] / 100 and got["best_index"] == want["best_index"]
        assert got["near_tie"] == want["near_tie"]
        ith, rem = divmod(want["best_index"], 1600)
        assert np.array_equal(got["pose"], [dlin[rem // 40], dlin[rem % 40], dth[ith]])
        assert (got["tiles_scored"], got["tiles_total"]) == (want["tiles_scored"], want["tiles_total"])
    # a new NDT: the image is made again (the result is the new map's), and matchScan is as it was
    after = m.matchScan(pose, points)
    assert after["score"] == before["score"] and after["best_index"] == before["best_index"]
    m.addScans(synth.map_scans(1)[:5])
    fewer = m.matchWide(pose, points, 1.0, 0.05, 0.2, 0.01, tile_steps=2)
    w2 = WideSearch(m)
    w2.set_tile(tile_steps=2)
    want2 = w2.match(pose, W.subsample(points, 100), dth, dlin)
    w2.close()
    assert fewer["score"] == want2["best_score"] / 100 and fewer["best_index"] == want2["best_index"]
    assert fewer["score"] != got["score"]
    # no NDT: score 0.0, nothing else
    m.reset()
    none = m.matchWide(pose, points, 1.0, 0.05, 0.2, 0.01)
    assert none["score"] == 0.0 and none["best_index"] == NO_INDEX and none["tiles_total"] == 0


def test_refusals_name_the_remedy_and_launch_nothing():
    m = _matcher(0.25)
    pose, points = synth.query_scan(1)[:2]
    beams = W.subsample(points, 100)
    dth, dlin = search_offsets(0.045, 0.02), search_offsets(0.205, 0.02)
    wide = WideSearch(m)
    good = wide.match(pose, beams, dth, dlin)

    def refused(code, text, *args, **kw):
        with pytest.raises(Ndt2dError) as ei:
            wide.match(*args, **kw)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    refused(_capi.ERR_INVALID, "not finite", (0.0, float("nan"), 0.0), beams, dth, dlin)
    refused(_capi.ERR_INVALID, "strictly ascending", pose, beams, dth, dlin[::-1])
    refused(_capi.ERR_INVALID, "strictly ascending", pose, beams, dth, np.concatenate([dlin[:3], dlin[2:]]))
    refused(_capi.ERR_INVALID, "bad argument (n_beams)", pose, np.zeros((0, 2)), dth, dlin)
    refused(_capi.ERR_INVALID, "bad argument (lattice)", pose, beams, np.zeros(0), dlin)
    # a tile of 32 steps of 0.1 m: its box spans more than 8 x 8 cells of 0.25 m
    wide.set_tile(32, 1)
    refused(_capi.ERR_INVALID, "ndt2d_wide_set_tile: fewer tile steps", pose, beams, dth, search_offsets(1.6, 0.1))
    # ... and eight pixels per quarter cell over 257 x 257 cells: more than 2^26 pixels
    big = ScanMatcherNDT(0)
    big.initialize("big", ndt_resolution=0.25, range_max=RANGE_MAX)
    cells = np.zeros((257 * 257, 6))
    assert _capi.lib().ndt2d_set_grid(big.device_handle, _capi.dptr(cells), 257, 257, 0.25, -32.0, -32.0) == _capi.OK
    w2 = WideSearch(big)
    w2.set_tile(1, 8)
    with pytest.raises(Ndt2dError) as ei:
        w2.match(pose, beams, dth, dlin)
    assert ei.value.code == _capi.ERR_INVALID and "2^26 pixels" in str(ei.value) and "fewer pixels per tile" in str(ei.value)
    w2.set_tile(1, 4)
    assert w2.match(pose, beams, dth, dlin)["best_index"] == -1
    w2.close()
    for bad in ((0, 2), (33, 2), (8, 0), (8, 9)):
        with pytest.raises(Ndt2dError):
            wide.set_tile(*bad)
    assert wide.tile() == (32, 1)
    bare = ScanMatcherNDT(0)
    bare.initialize("bare", ndt_resolution=0.25, range_max=RANGE_MAX)
    nothing = WideSearch(bare)
    with pytest.raises(Ndt2dError) as ei:
        nothing.match(pose, beams, dth, dlin)
    assert ei.value.code == _capi.ERR_NO_GRID
    with pytest.raises(Ndt2dError) as ei:
        nothing.read_image()
    assert ei.value.code == _capi.ERR_STATE
    nothing.close()
    # afterwards the object works and gives what it gave
    wide.set_tile(16, 4)
    again = wide.match(pose, beams, dth, dlin)
    assert np.array_equal(again["record"].view(np.uint64), good["record"].view(np.uint64))
    wide.close()


def test_the_plugin_mirror_equals_the_c_calls_record(tmp_path):
    """WideSearchHip::matchWide from a plain C++ program with a matcher of its own."""
    src = os.path.join(ROOT, "tests", "cpp", "wide_mirror_check.cpp")
    exe = str(tmp_path / "wide_mirror_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "ndt_2d_amd", "plugin"), src, "-o", exe, "-L", libdir, "-lndt2d_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scans = synth.map_scans(1)
    pose, points = synth.query_scan(1)[:2]
    pts = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for _, p in scans]
    offsets = np.zeros(len(scans) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in pts])
    query = np.ascontiguousarray(points, dtype=np.float64)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<QQQ", len(scans), int(offsets[-1]), len(query)))
        f.write(struct.pack("<9d", 0.25, RANGE_MAX, 1.0, 0.05, 0.2, 0.01, *pose))
        f.write(offsets.tobytes())
        f.write(np.ascontiguousarray([s[0] for s in scans], dtype=np.float64).tobytes())
        f.write(np.concatenate(pts).tobytes())
        f.write(query.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    m = _matcher(0.25)
    want = m.matchWide(pose, points, 1.0, 0.05, 0.2, 0.01, tile_steps=2)
    blob = open(tmp_path / "out.bin", "rb").read()
    assert len(blob) == 2 * (7 * 8 + 5 * 8)
    for call in range(2):
        d = struct.unpack_from("<7d", blob, call * 96)
        u = struct.unpack_from("<5Q", blob, call * 96 + 56)
        assert d[0] == want["score"] and list(d[1:4]) == list(want["pose"])
        assert list(d[4:7]) == [want["pose"][k] + pose[k] for k in range(3)]
        assert u == (want["best_index"], int(want["near_tie"]), 1, want["tiles_scored"], want["tiles_total"])
