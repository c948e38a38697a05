"""The wide search without a GPU: the numpy restatement (tests/wide_restatement.py) against the CPU
oracle's exhaustive matchScan on cfg-1's map -- every tile's bound dominates the best exact sum in
the tile, the walk finds the oracle's winner, and most tiles are never scored -- and the plain-C++
header of the bound image in a program of its own (plainly and under the sanitizers) against long
double dense sampling."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import wide_restatement as W
from ndt_2d_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_DIR = os.path.join(ROOT, "ndt_2d_amd", "csrc", "wide")

# the pruning case: cfg-1's map and query, +-1.0 m / 0.05 m, +-0.2 rad / 0.01 rad, 100 beams
LATTICE = dict(search_linear_size=1.0, search_linear_resolution=0.05, search_angular_size=0.2,
               search_angular_resolution=0.01, laser_max_beams=100)

_CASE = {}


def case():
    """The oracle's exhaustive search of the pruning case, computed once and left unchanged."""
    if not _CASE:
        ref = O.ScanMatcherNDT()
        ref.initialize(**dict(LATTICE, ndt_resolution=0.25, range_max=synth.CONFIGS[1]["range_max"]))
        ref.addScans(synth.map_scans(1))
        pose, points = synth.query_scan(1)[:2]
        want = ref.matchScan(pose, points, want_scores=True)
        ndt = ref.ndt
        _CASE.update(pose=np.asarray(pose, dtype=np.float64), beams=W.subsample(points, 100), want=want,
                     sums=-want["scores"], cells6=ndt.cells6(), size=(ndt.size_x, ndt.size_y), cell_size=ndt.cell_size,
                     origin=ndt.origin, dth=O.search_offsets(0.2, 0.01), dlin=O.search_offsets(1.0, 0.05))
    return _CASE


def walk(c, tile_steps, pixels_per_tile):
    window = W.window_of(c["dlin"], tile_steps)
    g, raw, data = W.image(c["cells6"], c["size"][0], c["size"][1], c["cell_size"], c["origin"], window, pixels_per_tile)
    bounds = W.tile_bounds(g, data, c["pose"], c["beams"], c["dth"], c["dlin"], tile_steps)
    return bounds, W.rounds(bounds, c["sums"], len(c["dth"]), len(c["dlin"]), tile_steps)


@pytest.mark.parametrize("tile_steps,pixels_per_tile", [(2, 1), (2, 2), (4, 2), (8, 1), (8, 4), (7, 2)])
def test_every_bound_dominates_and_the_winner_is_the_oracles(tile_steps, pixels_per_tile):
    c = case()
    n_th, n_lin = len(c["dth"]), len(c["dlin"])
    assert (n_th, n_lin) == (40, 40) and c["size"] == (41, 41) and np.all(np.diff(c["dlin"]) > 0.0)
    bounds, got = walk(c, tile_steps, pixels_per_tile)
    best_in_tile = W.tile_maxima(c["sums"], n_th, n_lin, tile_steps)
    assert bounds.shape == best_in_tile.shape
    slack = bounds - best_in_tile
    print("T = %d, %d pixels per tile: smallest bound - best sum %.3g, share scored %.4f"
          % (tile_steps, pixels_per_tile, slack.min(), got["tiles_scored"] / bounds.size))
    assert np.all(bounds >= best_in_tile)
    assert got["best_index"] == c["want"]["best_index"]
    assert got["best_sum"] == -c["want"]["scores"][c["want"]["best_index"]]
    # what was left out could not have won, nor come within the near-tie tolerance
    assert np.all(bounds[~got["evaluated"]] < got["best_sum"] * W.STOP)
    assert np.all(best_in_tile[~got["evaluated"]] < got["best_sum"] * (1.0 - W.NEAR_TIE))


def test_fewer_than_half_the_tiles_are_scored():
    c = case()
    bounds, got = walk(c, 2, 2)
    print("tiles scored %d of %d" % (got["tiles_scored"], bounds.size))
    assert bounds.size == 40 * 20 * 20
    assert got["tiles_scored"] < bounds.size / 2
    assert got["best_index"] == c["want"]["best_index"]


def test_the_order_and_the_rounds_on_a_lattice_by_hand():
    """Two theta steps of 3 x 3 candidates, T = 2: four tiles a step (the last row and column
    ragged).  Equal bounds keep their job order; equal sums go to the lower flat index; a
    candidate within 2^-36 of the winner marks it."""
    bounds = np.array([[[5.0, 1.0], [1.0, 0.5]], [[5.0, 0.25], [3.0, 0.0]]])
    assert W.order(bounds).tolist() == [0, 4, 6, 1, 2, 3, 5, 7]
    sums = np.zeros((2, 3, 3))
    sums[0, 1, 1] = 2.0
    sums[1, 0, 1] = 2.0
    sums[1, 2, 0] = 2.5
    got = W.rounds(bounds, sums.reshape(-1), 2, 3, 2, max_tiles=1)     # one tile a round
    assert got["best_index"] == 9 + 6 and got["best_sum"] == 2.5 and not got["near_tie"]
    assert got["evaluated"].reshape(-1).tolist() == [True, False, False, False, True, False, True, False]
    sums[1, 2, 0] = 0.0
    got = W.rounds(bounds, sums.reshape(-1), 2, 3, 2, max_tiles=1)
    assert got["best_index"] == 4 and got["near_tie"] and got["tiles_scored"] == 3
    sums[1, 0, 1] = 2.0 * (1.0 - 2.0 ** -30)
    assert not W.rounds(bounds, sums.reshape(-1), 2, 3, 2, max_tiles=1)["near_tie"]
    # no winner: every tile is scored
    got = W.rounds(bounds, np.zeros(18), 2, 3, 2)
    assert got["best_index"] == -1 and got["best_sum"] == 0.0 and got["tiles_scored"] == 8


def test_plain_cpp_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/wide_fn_check.cpp over csrc/wide/ndt2d_wide_fn.h: built with the host compiler,
    plainly and with -fsanitize=address,undefined (the runtime linked into the program), run
    directly.  Its own checks: the box maximum is never below a long double dense sample of the
    rectangle -- definite, indefinite, zero and non-finite records; the mean inside, on an edge and
    outside -- and for definite records it exceeds the true maximum by rounding only.  Here: its
    printed pixels equal the restatement's."""
    src = os.path.join(ROOT, "tests", "cpp", "wide_fn_check.cpp")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", WIDE_DIR, src]
    plain, sanitized = os.path.join(str(tmp_path), "wide_check"), os.path.join(str(tmp_path), "wide_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stdout[-2000:] + done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    print("\n".join(line for line in outputs[0].splitlines() if line.startswith("excess")))
    # the program's grid (3 x 2 cells of 0.25 m at (-0.3, 0.1)), through the restatement
    cells6 = np.array([[float.fromhex(t) for t in line.split()[1:]] for line in outputs[0].splitlines() if line.startswith("C ")])
    assert cells6.shape == (6, 6)
    pixels = [line.split() for line in outputs[0].splitlines() if line.startswith("P ")]
    g, raw, data = W.image(cells6, 3, 2, 0.25, (-0.3, 0.1), 0.07, 2)
    assert len(pixels) == g["nx"] * g["ny"] > 50
    for r in pixels:
        i, j, got = int(r[1]), int(r[2]), float.fromhex(r[3])
        want = float(data[j, i])
        assert abs(got - want) <= 1e-13 * want and got >= float(raw[j, i]), (i, j, got, want)
