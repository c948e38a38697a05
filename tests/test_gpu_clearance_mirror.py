"""ClearanceMapHip (ndt_2d_amd/plugin/clearance_hip.hpp) and ParticleFilterHip::initGlobal(...,
min_clearance) driven from a plain C++ program -- no Python, no torch in that process -- against the
yardsticks (tests/clearance_restatement.py, tests/seed_restatement.py) and the Python path, bit for
bit.  tests/cpp/clearance_mirror_check.cpp is compiled with g++ against include/ndt2d_hip.h and linked
with the in-tree libndt2d_hip.so."""
import os
import struct
import subprocess

import numpy as np
import pytest

import clearance_restatement as R
import seed_restatement as S
from ndt_2d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "clearance_mirror_check.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ndt_2d_amd", "plugin")]
WIDTH, HEIGHT, N, SEED, CAP = 70, 45, 3000, 20251, 3
GEO = (-1.75, 0.4, 0.05)
CLEARANCE = 0.1


def test_the_consumer_compiles_warning_free():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_cpp_clearance_and_init_global_are_the_yardsticks_bits(tmp_path):
    exe = str(tmp_path / "clearance_mirror_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC, "-o", exe,
                        "-L", libdir, "-lndt2d_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    grid = R.random_map(HEIGHT, WIDTH, 31, 0.02)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<QQQQQ", WIDTH, HEIGHT, N, SEED, CAP))
        f.write(struct.pack("<dddd", *GEO, CLEARANCE))
        f.write(grid.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    b = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        out = np.frombuffer(b, dtype=dtype, count=n, offset=at).copy()
        at += out.nbytes
        return out

    cells = WIDTH * HEIGHT
    threshold = R.min_d2(CLEARANCE, GEO[2])
    assert int(take("<u4", 1)[0]) == threshold == 4
    exact = R.d2_separable(grid)
    d2 = take("<u4", cells).reshape(HEIGHT, WIDTH)
    assert np.array_equal(d2, exact)
    capped = take("<u4", cells).reshape(HEIGHT, WIDTH)
    assert np.array_equal(capped, R.d2_separable(grid, False, CAP)) and (capped == R.FAR).any()
    inflated = take("i1", cells).reshape(HEIGHT, WIDTH)
    assert np.array_equal(inflated, R.mask(grid, exact, threshold)) and (inflated == R.INSCRIBED).any()
    # the Python path gives the same bits
    from ndt_2d_amd import ClearanceMap, ScanMatcherNDT, synth
    m = ScanMatcherNDT(0)
    m.initialize("mirror", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    cm = ClearanceMap(m)
    cm.compute(grid)
    assert np.array_equal(cm.d2(), d2)
    cm.mask(min_clearance=CLEARANCE, resolution=GEO[2])
    assert np.array_equal(cm.inflated(), inflated)
    cm.close()
    m.close()
    # initGlobal with the clearance: the restatement's poses over the filtered table
    table = R.cleared_table(grid, exact, threshold)
    assert 0 < len(table) < (grid == 0).sum()
    n = int(take("<u8", 1)[0])
    assert n == N
    seeded = take("<f8", 3 * N).reshape(N, 3)
    want = S.sample(SEED, 1, 0, N, table, WIDTH, *GEO)                 # steps 1 and 2
    assert np.array_equal(seeded.view(np.uint64), want.view(np.uint64))
    assert int(take("<u8", 1)[0]) == 2
    # the resident map of an occupancy map
    w, h = (int(v) for v in take("<u8", 2))
    geo = take("<f8", 3)
    n = int(take("<u8", 1)[0])
    assert n == 300
    resident = take("<f8", 3 * n).reshape(n, 3)
    data = take("i1", w * h).reshape(h, w)
    table = R.cleared_table(data, R.d2_separable(data), R.min_d2(CLEARANCE, geo[2]))
    assert 10 < len(table) < (data == 0).sum()
    want = S.sample(SEED, 3, 0, n, table, w, *geo)                     # steps 3 and 4
    assert np.array_equal(resident.view(np.uint64), want.view(np.uint64))
    assert at == len(b)
