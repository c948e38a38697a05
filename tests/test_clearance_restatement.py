"""The clearance map's yardstick (tests/clearance_restatement.py) pinned: the separable form against
the brute force over all obstacles, against scipy's exact Euclidean transform where scipy imports,
and against closed forms; min_d2 against its table.  And csrc/clearance/ndt2d_clearance_fn.h, the
arithmetic the kernels run, in a host program of its own (tests/cpp/clearance_fn_check.cpp), plainly
and under the sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import clearance_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEARANCE_DIR = os.path.join(ROOT, "ndt_2d_amd", "csrc", "clearance")


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_separable_is_the_brute_force_and_scipy(name):
    grid = R.SHAPES[name]()
    for unknown in (False, True):
        sep = R.d2_separable(grid, unknown)
        assert sep.dtype == np.uint32 and sep.shape == grid.shape
        assert np.array_equal(sep, R.d2_brute(grid, unknown))
        obs = R.obstacles(grid, unknown)
        assert np.array_equal(sep == 0, obs)
        try:
            from scipy import ndimage
        except ImportError:
            continue
        if obs.any():
            edt = ndimage.distance_transform_edt(~obs)
            assert np.array_equal(np.rint(edt * edt).astype(np.uint32), sep)
        else:
            assert np.all(sep == R.FAR)


def test_the_sparse_map_reaches_far():
    """300 x 300 at 0.0002: the longest outward scan of the GPU tests is over a hundred steps."""
    sep = R.d2_separable(R.SHAPES["300x300 sparse"]())
    assert (sep != R.FAR).all() and int(sep.max()) > 100 * 100


def test_closed_forms():
    # a single obstacle: dx^2 + dy^2
    grid = np.zeros((23, 31), dtype=np.int8)
    grid[9, 12] = 100
    ys, xs = np.mgrid[0:23, 0:31]
    want = ((ys - 9) ** 2 + (xs - 12) ** 2).astype(np.uint32)
    assert np.array_equal(R.d2_separable(grid), want) and np.array_equal(R.d2_brute(grid), want)
    # 3-4-5: an obstacle at offset (3, 4) gives 25; kept at min_d2 = 25, dropped at 26
    assert want[9 + 4, 12 + 3] == 25
    cell = (9 + 4) * 31 + (12 + 3)
    assert cell in R.cleared_table(grid, want, 25) and cell not in R.cleared_table(grid, want, 26)
    assert R.mask(grid, want, 25)[13, 15] == 0 and R.mask(grid, want, 26)[13, 15] == R.INSCRIBED
    # the obstacle itself, and every non-free byte, is never masked
    grid[0, 0] = -1
    grid[22, 30] = 50
    d2 = R.d2_separable(grid)
    m = R.mask(grid, d2, 10 ** 9)
    assert m[9, 12] == 100 and m[0, 0] == -1 and m[22, 30] == 50 and d2[22, 30] == 0 and d2[0, 0] > 0
    assert np.all(m[grid == 0] == R.INSCRIBED)
    assert np.array_equal(R.mask(grid, d2, 0), grid)
    # unknown cells: obstacles only on request
    assert R.d2_separable(grid, True)[0, 0] == 0 and R.d2_separable(grid, True)[0, 1] == 1
    # no obstacle: FAR everywhere, which has every clearance
    empty = np.zeros((4, 5), dtype=np.int8)
    assert np.all(R.d2_separable(empty) == R.FAR) and np.all(R.d2_brute(empty) == R.FAR)
    assert len(R.cleared_table(empty, R.d2_separable(empty), 2 ** 31)) == 20
    # stray bytes are obstacles
    stray = np.array([[1, 0, 50, 0, -2, 0, 99, 0, -1, 0]], dtype=np.int8)
    assert R.d2_separable(stray)[0].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 4, 9]
    # the cap: equality is kept, one more is FAR
    row = np.zeros((1, 12), dtype=np.int8)
    row[0, 0] = 100
    capped = R.d2_separable(row, max_cells=5)[0].tolist()
    assert capped[:6] == [0, 1, 4, 9, 16, 25] and capped[6:] == [R.FAR] * 6
    # a region restricts the table, not the transform
    assert R.cleared_table(row, R.d2_separable(row), 4, region=(1, 0, 3, 1)).tolist() == [2, 3]


def test_min_d2_table():
    assert [R.min_d2(c, r) for c, r in ((0.25, 0.05), (0.3, 0.05), (0.3, 0.1), (0.15, 0.05), (1.0, 0.02))] == \
        [25, 36, 9, 9, 2500]
    assert R.min_d2(0.0, 0.05) == 0


def test_the_library_min_d2_is_the_restatements():
    """ndt2d_clearance_min_d2 is host arithmetic: it runs without a GPU."""
    from ndt_2d_amd import _capi
    from ndt_2d_amd.clearance import min_d2_of
    rng = np.random.default_rng(5)
    pairs = [(0.25, 0.05), (0.3, 0.05), (0.3, 0.1), (0.15, 0.05), (1.0, 0.02), (0.0, 0.05)]
    pairs += [(float(c), float(r)) for c, r in zip(rng.random(200) * 3.0, rng.choice([0.02, 0.025, 0.05, 0.1, 0.25], 200))]
    for c, r in pairs:
        assert min_d2_of(c, r) == R.min_d2(c, r), (c, r)
    assert min_d2_of(0.3, 0.05, 6) == 36
    for bad in ((-0.1, 0.05, 0), (float("nan"), 0.05, 0), (float("inf"), 0.05, 0), (0.3, 0.0, 0), (0.3, float("nan"), 0),
                (0.3, 0.05, -1), (0.3, 0.05, 5), (46341.0, 1.0, 0)):
        with pytest.raises(_capi.Ndt2dError) as ei:
            min_d2_of(*bad)
        assert ei.value.code == _capi.ERR_INVALID
    assert _capi.lib().ndt2d_clearance_min_d2(0.3, 0.05, 0, None) == _capi.ERR_INVALID


def test_plain_cpp_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/clearance_fn_check.cpp built with the host compiler, plainly and with
    -fsanitize=address,undefined (the runtime linked into the program), and run directly: both end
    with "ok", write nothing to stderr and print the same.  Nothing is loaded into Python."""
    src = os.path.join(ROOT, "tests", "cpp", "clearance_fn_check.cpp")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CLEARANCE_DIR, src]
    plain, sanitized = str(tmp_path / "clearance_fn_check"), str(tmp_path / "clearance_fn_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                    "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, (done.stdout[-2000:], done.stderr)
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    assert "min_d2 0.3 / 0.05 = 36" in outputs[0] and "largest d2 2147352578" in outputs[0]
