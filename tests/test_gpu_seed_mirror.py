"""ParticleFilterHip::initGlobal / inject (ndt_2d_amd/plugin/particle_filter_hip.hpp) driven from a
plain C++ program -- no Python, no torch in that process -- against the restatement
(tests/seed_restatement.py), bit for bit.  tests/cpp/seed_mirror_check.cpp is compiled with g++
against include/ndt2d_hip.h and linked with the in-tree libndt2d_hip.so."""
import os
import struct
import subprocess

import numpy as np
import pytest

import seed_restatement as S
from ndt_2d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "seed_mirror_check.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ndt_2d_amd", "plugin")]
WIDTH, HEIGHT, N, SEED = 70, 45, 3000, 20241
GEO = (-1.75, 0.4, 0.05)
PROBABILITY = 0.2


def test_the_consumer_compiles_warning_free():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_cpp_init_global_and_inject_are_the_restatements_bits(tmp_path):
    exe = str(tmp_path / "seed_mirror_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC, "-o", exe,
                        "-L", libdir, "-lndt2d_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(9)
    grid = np.where(rng.random((HEIGHT, WIDTH)) < 0.5, 0, rng.choice([-1, 100], size=(HEIGHT, WIDTH))).astype(np.int8)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<QQQQ", WIDTH, HEIGHT, N, SEED))
        f.write(struct.pack("<dddd", *GEO, PROBABILITY))
        f.write(grid.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    b = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def u64():
        nonlocal at
        at += 8
        return struct.unpack_from("<Q", b, at - 8)[0]

    def f64(n):
        nonlocal at
        at += 8 * n
        return np.frombuffer(b, dtype="<f8", count=n, offset=at - 8 * n).copy()

    table = S.free_table(grid)
    assert u64() == N
    seeded = f64(3 * N).reshape(N, 3)
    want = S.sample(SEED, 1, 0, N, table, WIDTH, *GEO)                 # steps 1 and 2
    assert np.array_equal(seeded.view(np.uint64), want.view(np.uint64))
    replaced = u64()
    injected = f64(3 * N).reshape(N, 3)
    want, take = S.inject(seeded, PROBABILITY, SEED, 3, 0, table, WIDTH, *GEO)   # steps 3 and 4
    assert replaced == int(take.sum()) and 0.15 * N < replaced < 0.25 * N
    assert np.array_equal(injected.view(np.uint64), want.view(np.uint64))
    assert u64() == 4
    # the resident map of an occupancy map: the set is the restatement's over the map its read gives
    w, h = u64(), u64()
    geo = f64(3)
    n = u64()
    assert n == 300
    resident = f64(3 * n).reshape(n, 3)
    data = np.frombuffer(b, dtype=np.int8, count=w * h, offset=at).reshape(h, w)
    assert (data == 0).sum() > 10
    want = S.sample(SEED, 5, 0, n, S.free_table(data), w, *geo)      # steps 5 and 6
    assert np.array_equal(resident.view(np.uint64), want.view(np.uint64))
