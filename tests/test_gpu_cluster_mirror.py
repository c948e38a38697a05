"""ParticleFilterHip::clusters / bestCluster (ndt_2d_amd/plugin/particle_filter_hip.hpp) driven from a
plain C++ program -- no Python, no torch in that process -- against the restatement
(tests/cluster_restatement.py) of the particles and weights that program saw, to the bounds of
tests/test_gpu_clusters.py.  tests/cpp/cluster_mirror_check.cpp is compiled with g++ against
include/ndt2d_hip.h and linked with the in-tree libndt2d_hip.so."""
import collections
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_restatement as R
from cluster_cases import BOUND, compare
from ndt_2d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cluster_mirror_check.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ndt_2d_amd", "plugin")]
WIDTH, HEIGHT, N, SEED = 70, 45, 3000, 20241
GEO = (-1.75, 0.4, 0.05)

Header = collections.namedtuple("Header", "n n_left_out n_bins n_clusters rounds w_total")
Record = collections.namedtuple("Record", "label count mass weight mean_x mean_y mean_theta cxx cxy cyy var_theta")


def test_the_consumer_compiles_warning_free():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_cpp_clusters_and_best_cluster_are_the_restatements(tmp_path):
    exe = str(tmp_path / "cluster_mirror_check")
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC, "-o", exe,
                        "-L", libdir, "-lndt2d_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(9)
    grid = np.where(rng.random((HEIGHT, WIDTH)) < 0.5, 0, rng.choice([-1, 100], size=(HEIGHT, WIDTH))).astype(np.int8)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<QQQQ", WIDTH, HEIGHT, N, SEED))
        f.write(struct.pack("<dddd", *GEO, 0.0))
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

    for max_clusters, n_want in ((4, N), (8, N)):
        n = u64()
        assert n == n_want
        poses, w = f64(3 * n).reshape(n, 3), f64(n)
        header = Header(u64(), u64(), u64(), u64(), u64(), float(f64(1)[0]))
        records = []
        for _ in range(u64()):
            label, count = u64(), u64()
            records.append(Record(label, count, *f64(9).tolist()))
        want = R.cluster(poses, w, max_clusters=max_clusters)
        # (the mirror has no per-particle labels to give: the restatement's stand in for them)
        compare((header, records, want["labels"]), want, max_clusters=max_clusters)
        have_best = u64()
        mean, cov, share = f64(3), f64(9), float(f64(1)[0])
        label, count = u64(), u64()
        whole_mean = f64(3)
        assert have_best == 1 and (label, count) == (records[0].label, records[0].count)
        # bestCluster is the first record of a call of its own on the same set: the same bits
        first = records[0]
        assert mean.tolist() == [first.mean_x, first.mean_y, first.mean_theta]
        assert cov.tolist() == [first.cxx, first.cxy, 0.0, first.cxy, first.cyy, 0.0, 0.0, 0.0, first.var_theta]
        assert share == first.weight / header.w_total and abs(share - want["records"][0]["W"] / want["header"]["w_total"]) <= 4.0 * BOUND
        print("max_clusters %d: %d clusters in %d bins, best share %.4f, rounds %d" %
              (max_clusters, header.n_clusters, header.n_bins, share, header.rounds))
        if max_clusters == 4:
            # a seeded set: as many clusters as the free space has pieces (one, on a map this small and dense)
            assert header.n_bins > 100 and len(records) == min(4, header.n_clusters)
        else:
            # init(1.3, -0.4, 3.1, ...): one blob across +-pi; getMean is the whole set's, and agrees here
            assert header.n_clusters == 1 and share == 1.0 and abs(abs(mean[2]) - np.pi) < 0.1
            assert np.hypot(whole_mean[0] - mean[0], whole_mean[1] - mean[1]) < 1e-9
    assert at == len(b)
