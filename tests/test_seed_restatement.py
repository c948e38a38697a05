"""Global localisation without a GPU: the numpy restatement of the seeder (tests/seed_restatement.py)
pinned to the Random123 known answers and to designed words at both ends of every uniform; the
property that a sampled position falls back into its cell; the plain-C++ header in a program of its
own (plainly and under the sanitizers), bit for bit against the restatement; RecoveryAverages
against a sequence computed by hand; and what holds the unit in the build, the header and the
bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

import noise_restatement as N
import seed_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")
SEED_DIR = os.path.join(CSRC, "seed")

ZERO = np.zeros((1, 4), dtype=np.uint64)
ONES = np.full((1, 4), 0xffffffff, dtype=np.uint64)
# (origin_x, origin_y, resolution): the occupancy tests' kinds, 0.05 and negative origins among them
GEOMETRIES = [(0.0, 0.0, 1.0), (-3.35, 1.7, 0.05), (-10.25, -10.25, 0.05), (1.7, -0.3, 0.1), (-47.5, -47.5, 0.25),
              (12.345, -0.3, 0.025)]


def test_the_words_are_the_known_answers():
    """Block A of particle `first` at (seed, step) and block B (step + 1) are Random123's
    philox4x32-10 of those counters."""
    for (seed, step, first), (_, _, out) in zip(N.KAT_STREAM, N.KAT):
        a, _ = S.words(seed, step, first, 1)
        assert tuple(int(v) for v in a[0]) == out
    # block B is block A of the next step, and the step wraps at 2^64
    _, b = S.words(7, 5, 11, 3)
    assert np.array_equal(b, N.philox_words(7, 6, 11, 3))
    _, b = S.words(7, (1 << 64) - 1, 11, 3)
    assert np.array_equal(b, N.philox_words(7, 0, 11, 3))


def test_designed_words_at_both_ends_of_each_uniform():
    assert S.uniform53(0, 0) == 0.0 and S.uniform53(31, 63) == 0.0             # the low bits are dropped
    assert S.uniform53(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert S.uniform53(32, 0) == 2.0 ** -27 and S.uniform53(0, 64) == 2.0 ** -53
    assert S.uniform24(0) == 2.0 ** -25 and S.uniform24(255) == 2.0 ** -25     # the smallest: never 0
    assert S.uniform24(0xffffffff) == 1.0 - 2.0 ** -25                         # the largest: never 1
    assert S.uniform24(256) == 3.0 * 2.0 ** -25
    assert float(S.heading(np.float64(0.5))) == 0.0
    assert -np.pi < float(S.heading(S.uniform24(0))) and float(S.heading(S.uniform24(0xffffffff))) < np.pi
    # all-zero words: the first free cell, the low corner of it; all-one words: the last, the high corner
    table = np.array([5, 9, 13, 22], dtype=np.uint32)
    for ox, oy, res in GEOMETRIES:
        lo, v_lo, k_lo = S.from_words(ZERO, ZERO, table, 6, ox, oy, res)
        hi, v_hi, k_hi = S.from_words(ONES, ONES, table, 6, ox, oy, res)
        assert int(k_lo[0]) == 0 and int(k_hi[0]) == len(table) - 1               # k at both ends
        assert float(v_lo[0]) == 0.0 and float(v_hi[0]) == 1.0 - 2.0 ** -53
        assert lo[0, 0] == np.float64(ox) + (np.float64(5.0) + np.float64(2.0 ** -25)) * np.float64(res)
        assert lo[0, 1] == np.float64(oy) + (np.float64(0.0) + np.float64(2.0 ** -25)) * np.float64(res)
        assert hi[0, 0] == np.float64(ox) + (np.float64(4.0) + np.float64(1.0 - 2.0 ** -25)) * np.float64(res)
        assert hi[0, 1] == np.float64(oy) + (np.float64(3.0) + np.float64(1.0 - 2.0 ** -25)) * np.float64(res)
        assert lo[0, 2] == -np.pi + (2.0 * np.pi) * 2.0 ** -25 and hi[0, 2] == -np.pi + (2.0 * np.pi) * (1.0 - 2.0 ** -25)
        assert -np.pi < lo[0, 2] < hi[0, 2] < np.pi


def test_the_pick_is_clamped_to_the_last_cell():
    """k = min(F - 1, trunc(u F)): all-one words give F - 1 for every F, and the clamp holds where a
    product could round up to F (u = 1 stands for it: no word gives it)."""
    u_max = S.uniform53(0xffffffff, 0xffffffff)
    for f in (1, 2, 3, 5, 63, 64, 65, 1000, 90000, 641601, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1):
        assert int(S.pick(u_max, f)) == f - 1
        assert int(S.pick(np.float64(1.0), f)) == f - 1
        assert int(S.pick(np.float64(0.0), f)) == 0
        # against Python's integers: the double product is the exact one rounded to 53 bits
        rng = np.random.default_rng(f)
        bits = rng.integers(0, 1 << 53, size=2000, dtype=np.uint64)
        got = S.pick(bits.astype(np.float64) * S.INV53, f)
        for b, k in zip(bits.tolist(), got.tolist()):
            want = min(f - 1, int(float(b) * 2.0 ** -53 * float(f)))      # Python floats are IEEE doubles
            assert k == want
            assert abs(k - (b * f >> 53)) <= 1 and k < f


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_every_sampled_position_falls_back_into_its_cell(geometry):
    """int((p - origin) / resolution), the occupancy grid's own rule, gives the cell the sample
    was drawn for: for random words, for the ends of the offsets, in the corners of a large map."""
    ox, oy, res = geometry
    width, height = 801, 640
    rng = np.random.default_rng(5)
    grid = np.where(rng.random((height, width)) < 0.4, 0, 100).astype(np.int8)
    grid[0, 0] = grid[0, -1] = grid[-1, 0] = grid[-1, -1] = 0
    table = S.free_table(grid)
    assert np.array_equal(table, np.flatnonzero(grid.reshape(-1) == 0))
    n = 20000
    a, b = S.words(3, 9, 0, n)
    # the first particles: designed offsets in the four corner cells (k through designed words)
    ends = [0, 255, 256, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffffff]
    j = 0
    for corner in (0, width - 1, (height - 1) * width, height * width - 1):
        k = int(np.searchsorted(table, corner))
        assert table[k] == corner
        # words whose uniform53 picks k: the middle of [k / F, (k + 1) / F)
        bits = ((2 * k + 1) << 52) // len(table)
        for wx in ends:
            for wy in ends:
                a[j] = (((bits >> 26) << 5) & 0xffffffff, ((bits & ((1 << 26) - 1)) << 6) & 0xffffffff, wx, wy)
                j += 1
    poses, v, k = S.from_words(a, b, table, width, ox, oy, res)
    cell = table[k.astype(np.int64)].astype(np.int64)
    assert set(cell[:j].tolist()) == {0, width - 1, (height - 1) * width, height * width - 1}
    assert np.array_equal(S.cell_of(poses[:, 0], ox, res), cell % width)
    assert np.array_equal(S.cell_of(poses[:, 1], oy, res), cell // width)
    assert np.all(grid.reshape(-1)[cell] == 0)
    assert np.all((poses[:, 2] > -np.pi) & (poses[:, 2] < np.pi)) and np.all((v >= 0.0) & (v < 1.0))
    # uniformity over the table, loosely: every decile of the table is hit about n / 10 times
    hist = np.bincount((10 * k[j:].astype(np.int64)) // len(table), minlength=10)
    assert hist.min() > 0.8 * (n - j) / 10 and hist.max() < 1.2 * (n - j) / 10


def test_inject_restated():
    table = np.arange(0, 600, 7, dtype=np.uint32)
    before = np.full((5000, 3), -0.0)
    fresh = S.sample(4, 2, 100, 5000, table, 30, -1.0, 2.0, 0.05)
    for p in (0.0, 0.25, 1.0):
        after, take = S.inject(before, p, 4, 2, 100, table, 30, -1.0, 2.0, 0.05)
        assert np.array_equal(after[take], fresh[take])
        assert np.all(np.signbit(after[~take])) and np.all(after[~take] == 0.0)       # -0.0 kept
        if p == 0.0:
            assert not take.any()
        elif p == 1.0:
            assert take.all()
        else:
            assert 0.2 * 5000 < take.sum() < 0.3 * 5000
    # a shard draws what the whole set would
    assert np.array_equal(S.sample(4, 2, 100 + 2500, 2500, table, 30, -1.0, 2.0, 0.05), fresh[2500:])


def test_free_table_regions():
    grid = np.array([[0, 1, 0, -1], [100, 0, 0, -128], [0, 0, 127, 0]], dtype=np.int8)
    assert S.free_table(grid).tolist() == [0, 2, 5, 6, 8, 9, 11]
    assert S.free_table(grid, (1, 1, 2, 2)).tolist() == [5, 6, 9]
    assert S.free_table(grid, (3, 0, 1, 2)).tolist() == []


def _check_outputs(tmp_path, name):
    """tests/cpp/<name> built with the host compiler, plainly and with -fsanitize=address,undefined
    (the runtime linked into the program), and run directly: both end with "ok", write nothing to
    stderr and print the same."""
    src = os.path.join(ROOT, "tests", "cpp", name)
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", SEED_DIR, "-I", CSRC, src]
    stem = os.path.join(str(tmp_path), os.path.splitext(name)[0])
    plain, sanitized = stem, stem + "_san"
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    return outputs


def test_the_compaction_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/compact_fn_check.cpp over csrc/particles/ndt2d_compact_fn.h: the ranks of a lane
    against the builtin popcount, the scan's chunks (they tile [0, n_tiles) up to 2^32 - 1), the
    compaction against a plain loop."""
    _check_outputs(tmp_path, "compact_fn_check.cpp")


def test_plain_cpp_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/seed_fn_check.cpp over csrc/seed/ndt2d_seed_fn.h: built with the host compiler,
    plainly and with -fsanitize=address,undefined (the runtime linked into the program), run
    directly.  Its own checks: Philox's known answers, the uniforms and the pick against integers,
    the coordinates against long double and the cell rule.  Here: every printed sample equals the restatement's bit for bit."""
    outputs = _check_outputs(tmp_path, "seed_fn_check.cpp")
    rows = [line.split() for line in outputs[0].splitlines() if line.startswith("P ")]
    assert len(rows) == 32
    width, height = 37, 23
    grid = np.array([[100 if (x * 7 + y * 13) % 5 == 0 else 0 for x in range(width)] for y in range(height)], dtype=np.int8)
    table = S.free_table(grid)
    for r in rows:
        seed, step, index = int(r[1]), int(r[2]), int(r[3])
        a, b = S.words(seed, step, index, 1)
        pose, v, _ = S.from_words(a, b, table, width, -3.35, 1.7, 0.05)
        got = [float.fromhex(t) for t in r[4:8]]
        want = [float(pose[0, 0]), float(pose[0, 1]), float(pose[0, 2]), float(v[0])]
        assert got == want, (r, want)
    assert (0, 0, 0) in [(int(r[1]), int(r[2]), int(r[3])) for r in rows]


def test_recovery_averages_against_a_sequence_by_hand():
    """alpha_slow = 0.1, alpha_fast = 0.5; w_avg = 4, 4, 2, 1, 4:
         slow: 4, 4, 3.8, 3.52, 3.568      fast: 4, 4, 3, 2, 3
         share = max(0, 1 - fast / slow): 0, 0, 0.8 / 3.8, 1.52 / 3.52, 0.568 / 3.568"""
    from ndt_2d_amd import RecoveryAverages
    r = RecoveryAverages(0.1, 0.5)
    got = [r.update(w) for w in (4.0, 4.0, 2.0, 1.0, 4.0)]
    want = [0.0, 0.0, 0.8 / 3.8, 1.52 / 3.52, 0.568 / 3.568]
    assert np.allclose(got, want, rtol=1e-14, atol=0.0), (got, want)
    assert abs(r.w_slow - 3.568) < 1e-14 and abs(r.w_fast - 3.0) < 1e-14
    # the reference's scores are negated likelihoods: the same shares for the negated sequence
    r = RecoveryAverages(0.1, 0.5)
    assert np.allclose([r.update(-w) for w in (4.0, 4.0, 2.0, 1.0, 4.0)], want, rtol=1e-14, atol=0.0)
    # weights that improve never ask for an injection; nor does a filter without any weight
    r = RecoveryAverages(0.05, 0.5)
    assert [r.update(w) for w in (1.0, 2.0, 3.0, 3.0)] == [0.0, 0.0, 0.0, 0.0]
    assert RecoveryAverages(0.1, 0.5).update(0.0) == 0.0
    with pytest.raises(ValueError):
        RecoveryAverages(0.5, 0.1)


def test_the_unit_is_built_hashed_bound_and_declared():
    from ndt_2d_amd import _capi, build
    assert "seed/ndt2d_seed.hip" in build.SOURCES
    assert os.path.join(SEED_DIR, "ndt2d_seed_fn.h") in build.HEADERS
    assert sorted(n for n in os.listdir(SEED_DIR) if n.endswith((".hip", ".h"))) == ["ndt2d_seed.hip", "ndt2d_seed_fn.h"]
    names = sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_seed_"))
    assert names == sorted("ndt2d_seed_" + n for n in (
        "create", "destroy", "last_error", "set_map", "set_map_device", "free_count", "read_table", "launch",
        "inject_launch", "set_timing", "last_ms"))
    assert "ndt2d_occmap_device_map" in _capi.SIGNATURES
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    assert "#define NDT2D_ABI_VERSION 4" in header and "Global localisation" in header     # new symbols only
    unit = open(os.path.join(SEED_DIR, "ndt2d_seed.hip")).read()
    code = re.sub(r"//[^\n]*", "", unit)
    # every extern "C" body that can throw sits between the guards (last_error returns a stored string)
    assert code.count("NDT2D_C_TRY") == code.count("NDT2D_C_CATCH") == 10
    # no read-modify-write atomics: the compaction and the count are ballots, popcounts and fixed folds
    assert not re.search(r"atomic(Add|Min|Max|CAS|Or|And|Exch|Inc)|__hip_atomic_fetch", code)
    assert code.count("__global__") == 6 and "__ballot(" in code and "__popcll(" in code
    # the arithmetic is plain C++: no HIP header and no HIP type in the header the kernels share
    fn = open(os.path.join(SEED_DIR, "ndt2d_seed_fn.h")).read()
    assert "hip_runtime" not in fn and "double2" not in fn and "__global__" not in fn
    # the accessor is the only edit to the occupancy-map unit: it holds no kernel and launches none
    occ = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "occupancy_map", "ndt2d_occupancy_map.hip")).read()
    body = occ[occ.index("int ndt2d_occmap_device_map("):]
    body = body[:body.index("\n}\n")]
    assert "hipLaunchKernelGGL" not in body and "NDT2D_C_TRY" in body


def test_the_cpp_mirror_compiles_with_the_new_members(tmp_path):
    stub = os.path.join(str(tmp_path), "use.cpp")
    with open(stub, "w") as f:
        f.write('#include "particle_filter_hip.hpp"\n'
                "std::size_t use(ndt_2d_hip::ParticleFilterHip & p, ndt2d_occupancy_map * m, const signed char * g,\n"
                "                const std::uint32_t * region)\n"
                "{\n  p.initGlobal(g, 3, 3, 0.0, 0.0, 0.1);\n  p.initGlobal(g, 3, 3, 0.0, 0.0, 0.1, 100, region);\n"
                "  p.initGlobal(m);\n  p.initGlobal(m, 100, region);\n  return p.inject(0.1);\n}\n")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "ndt_2d_amd", "plugin"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
