"""Pose clusters without a GPU: the numpy restatement of the clusterer (tests/cluster_restatement.py)
against cases worked by hand; the plain-C++ header in a program of its own (plainly and under the
sanitizers), bit for bit against the restatement; what holds the unit in the build, the header and
the bindings; and the C++ mirror's new members."""
import os
import re
import subprocess

import numpy as np

import cluster_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER_DIR = os.path.join(ROOT, "ndt_2d_amd", "csrc", "cluster")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ndt_2d_amd", "plugin")]


def at(kx, ky, kt, n_theta=24, cell=0.5):
    """The middle of the bin (kx, ky, kt)."""
    return ((kx + 0.5) * cell, (ky + 0.5) * cell, -np.pi + (kt + 0.5) * 2.0 * np.pi / n_theta)


def labels_of(poses, weights=None, **kw):
    return R.cluster(np.array(poses, dtype=np.float64), weights, **kw)["labels"].tolist()


def test_keys_by_hand():
    kx, ky, kt, out = R.keys([(-0.25, 0.25, 0.0), (0.25, -0.25, 0.0), (0.0, -0.0, -np.pi), (-0.5, 0.5, np.pi),
                              (1.74, -1.76, np.nextafter(np.pi, 0.0)), (0.1, 0.1, 3.0 * np.pi)], None)
    assert kx.tolist() == [-1, 0, 0, -1, 3, 0] and ky.tolist() == [0, -1, 0, 1, -4, 0]
    assert kt.tolist()[:5] == [12, 12, 0, 0, 23] and kt[5] in (0, 23) and not out.any()
    # floor, not truncation: the bins either side of 0 are as wide as every other
    xs = (np.arange(2000) + 0.5) / 1000.0 - 1.0
    kx, _, _, _ = R.keys(np.stack([xs, xs, 0 * xs], axis=1), None)
    assert np.bincount(kx + 2).tolist()[:4] == [500, 500, 500, 500]
    # theta_bin is clamped where (t + pi) rounds up to 2 pi
    for n_theta in (1, 2, 3, 24, 360):
        assert int(R.theta_bin(np.nextafter(np.pi, 0.0), n_theta)) == n_theta - 1
        assert int(R.theta_bin(-np.pi, n_theta)) == 0
    t = R.normalise_angle(np.array([-np.pi, np.pi, 3.0 * np.pi, -3.0 * np.pi, 0.0, 4.0, -4.0, 1e9]))
    assert np.all((t >= -np.pi) & (t < np.pi)) and t[0] == -np.pi and t[1] == -np.pi and t[4] == 0.0
    assert t[5] == 4.0 - 2.0 * np.pi and t[6] == -t[5] and t[7] == np.fmod(1e9, 2.0 * np.pi)


def test_left_out_by_hand():
    poses = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (2.0 ** 29, 0, 0), (0, -2.0 ** 29, 0), (np.nextafter(2.0 ** 29, 0), 0, 0),
             (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]
    w = np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, np.nan, -1e-300, np.nextafter(1.0, 2.0), 1.0, 0.0])
    kx, _, kt, out = R.keys(poses, w)
    assert out.tolist() == [True, True, True, True, True, False, True, True, True, False, False]
    assert kx[5] == 2 ** 30 - 1 and np.all(kt[out] == -1)
    got = R.cluster(np.array(poses, dtype=np.float64), w)
    assert got["header"]["n_left_out"] == 8 and got["labels"].tolist() == [R.LEFT_OUT] * 5 + [5] + [R.LEFT_OUT] * 3 + [9, 9]
    # the particle of weight 0 counts as a member, not towards Q
    assert [(r["label"], r["count"], r["Q"]) for r in got["records"]] == [(9, 2, 2 ** 40), (5, 1, R.mass_q(0.1))]


def test_mass_by_hand():
    assert R.mass_q(0.0) == 0 and R.mass_q(2.0 ** -41) == 0 and R.mass_q(2.0 ** -40) == 1 and R.mass_q(1.0) == 2 ** 40
    assert R.mass_q(np.nextafter(2.0 ** -40, 0.0)) == 0 and R.mass_q(0.6) == 659706976665 and R.mass_q(0.75) == 3 * 2 ** 38


def test_components_by_hand():
    # x = -0.25 and +0.25: keys -1 and 0, one cluster
    assert labels_of([(-0.25, 0.1, 0.0), (0.25, 0.1, 0.0)]) == [0, 0]
    # keys that differ by (1, 1, 1): one cluster; by 2 in one coordinate: two
    assert labels_of([at(3, 4, 5), at(4, 5, 6)]) == [0, 0]
    assert labels_of([at(3, 4, 5), at(2, 3, 4)]) == [0, 0]
    assert labels_of([at(3, 4, 5), at(5, 4, 5)]) == [0, 1]
    assert labels_of([at(3, 4, 5), at(3, 6, 5)]) == [0, 1]
    assert labels_of([at(3, 4, 5), at(3, 4, 7)]) == [0, 1]
    assert labels_of([at(3, 4, 5), at(4, 5, 7)]) == [0, 1]
    # heading bins 0 and n_theta - 1: one cluster; 0 and n_theta - 2: two
    assert labels_of([at(3, 4, 0), at(3, 4, 23)]) == [0, 0]
    assert labels_of([at(3, 4, 0), at(4, 3, 23)]) == [0, 0]
    assert labels_of([at(3, 4, 0), at(3, 4, 22)]) == [0, 1]
    # n_theta = 1: every heading is bin 0; n_theta = 2: a bin and its twin are neighbours
    assert labels_of([(0.1, 0.1, -3.0), (0.1, 0.1, 3.0), (0.6, 0.6, 0.0), (1.6, 0.1, 1.0)], n_theta=1) == [0, 0, 0, 3]
    assert labels_of([(0.1, 0.1, -1.0), (0.1, 0.1, 1.0), (0.6, 0.6, 2.0), (1.6, 0.1, 1.0)], n_theta=2) == [0, 0, 0, 3]
    kx, ky, kt, _ = R.keys([(0.1, 0.1, -1.0), (0.1, 0.1, 1.0)], None, n_theta=2)
    assert kt.tolist() == [0, 1]
    # a chain joins through the middle; the label is the smallest index, wherever it sits
    assert labels_of([at(2, 0, 5), at(9, 9, 9), at(0, 0, 5), at(1, 0, 5)]) == [0, 1, 0, 0]
    assert labels_of([at(9, 9, 9), at(2, 0, 5), at(0, 0, 5), at(1, 0, 5)]) == [0, 1, 1, 1]
    # the neighbour list: 26 for n_theta >= 3, with the wrap
    near = R.neighbours((0, 0, 0), 24)
    assert len(near) == 26 and len(set(near)) == 26 and (0, 0, 0) not in near and {k[2] for k in near} == {23, 0, 1}
    assert len(set(R.neighbours((0, 0, 0), 2))) == 17 and len(set(R.neighbours((0, 0, 0), 1))) == 9


def test_rank_and_statistics_by_hand():
    # equal Q: the lower label is first, whatever the counts
    poses = [at(10, 0, 3), at(0, 0, 3), at(0, 0, 3), at(10, 0, 3), at(20, 0, 3)]
    got = R.cluster(np.array(poses), np.array([0.25, 0.25, 0.25, 0.25, 0.75]))
    assert [(r["label"], r["count"], r["Q"]) for r in got["records"]] == [(4, 1, 3 * 2 ** 38), (0, 2, 2 ** 39), (1, 2, 2 ** 39)]
    assert R.ranks_before(5, 9, 4, 1) and R.ranks_before(5, 1, 5, 9) and not R.ranks_before(5, 9, 5, 9)
    # statistics: two particles of weights 1/4 and 3/4 at x = 1 and 2, y = 3, headings +-(pi - 0.1)
    got = R.cluster(np.array([(1.0, 3.0, np.pi - 0.1), (2.0, 3.0, -(np.pi - 0.1))]), np.array([0.25, 0.75]), cell_x=4.0, cell_y=4.0, n_theta=1)
    (r,) = got["records"]
    assert r["W"] == 1.0 and r["mx"] == 1.75 and r["my"] == 3.0 and r["cxx"] == 0.25 * 0.75 ** 2 + 0.75 * 0.25 ** 2
    assert r["cxy"] == 0.0 and r["cyy"] == 0.0 and r["abs"]["x"] == 1.75 and r["abs"]["W"] == 1.0
    # the circular mean lies beyond +-pi's cut, 0.05 from it on the heavier side; the spread is taken round it
    assert abs(r["mt"] - (-np.pi + np.arctan2(0.5 * np.sin(0.1), np.cos(0.1)))) < 1e-15 and r["mt"] < -3.0
    d0, d1 = (np.pi - 0.1) - r["mt"] - 2.0 * np.pi, -(np.pi - 0.1) - r["mt"]
    assert abs(r["vt"] - (0.25 * d0 * d0 + 0.75 * d1 * d1)) < 1e-15 and r["vt"] < 0.01
    assert got["header"] == {"n": 2, "n_left_out": 0, "n_bins": 1, "n_clusters": 1, "w_total": 1.0}
    # more clusters than records; uniform weights where none are given; nothing at all
    many = R.cluster(np.array([at(3 * k, 0, 0) for k in range(20)]), None, max_clusters=4)
    assert many["header"]["n_clusters"] == 20 and [r["label"] for r in many["records"]] == [0, 1, 2, 3]
    assert many["records"][0]["Q"] == R.mass_q(1.0 / 20.0) and many["records"][0]["W"] == 1.0 / 20.0
    empty = R.cluster(np.zeros((0, 3)), None)
    assert empty["header"] == {"n": 0, "n_left_out": 0, "n_bins": 0, "n_clusters": 0, "w_total": 0.0} and empty["records"] == []


def test_plain_cpp_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/cluster_fn_check.cpp over csrc/cluster/ndt2d_cluster_fn.h: built with the host
    compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the program),
    run directly.  Its own checks: the bin edges on both sides of 0, the heading at -pi, pi, 3 pi and
    below pi, every left-out reason, q, the neighbour lists, the rank order.  Here: every printed
    sample equals the restatement's bit for bit."""
    src = os.path.join(ROOT, "tests", "cpp", "cluster_fn_check.cpp")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", CLUSTER_DIR, src]
    plain, sanitized = os.path.join(str(tmp_path), "cluster_check"), os.path.join(str(tmp_path), "cluster_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    assert outputs[0] == outputs[1]
    rows = [line.split() for line in outputs[0].splitlines()]
    n_keys = n_angles = n_lists = 0
    for r in rows:
        if r[0] == "K":
            x, y, theta, w, cell_x, cell_y = (float.fromhex(t) for t in r[1:7])
            n_theta = int(r[7])
            kx, ky, kt, out = R.keys([(x, y, theta)], np.array([w]), cell_x, cell_y, n_theta)
            q = 0 if out[0] else R.mass_q(w)
            want = [int(kx[0]), int(ky[0]), int(kt[0]), q, R.key_hash(int(kx[0]), int(ky[0]), int(kt[0]))]
            assert [int(t) for t in r[8:13]] == want, (r, want)
            n_keys += 1
        elif r[0] == "A":
            theta, t = float.fromhex(r[1]), float.fromhex(r[2])
            assert float(R.normalise_angle(theta)).hex() == t.hex(), r
            n_angles += 1
        elif r[0] == "N":
            key, n_theta = tuple(int(t) for t in r[1:4]), int(r[4])
            flat = [int(t) for t in r[5:]]
            assert [tuple(flat[3 * j:3 * j + 3]) for j in range(26)] == R.neighbours(key, n_theta), r
            n_lists += 1
    assert n_keys > 150 and n_angles == 11 and n_lists == 7


def test_the_unit_is_built_hashed_bound_and_declared():
    from ndt_2d_amd import _capi, build
    assert "cluster/ndt2d_cluster.hip" in build.SOURCES
    assert os.path.join(CLUSTER_DIR, "ndt2d_cluster_fn.h") in build.HEADERS
    assert sorted(n for n in os.listdir(CLUSTER_DIR) if n.endswith((".hip", ".h"))) == ["ndt2d_cluster.hip", "ndt2d_cluster_fn.h"]
    names = sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_cluster_"))
    assert names == sorted("ndt2d_cluster_" + n for n in (
        "create", "destroy", "last_error", "set_bins", "set_max_clusters", "launch", "fetch", "read_labels", "set_timing",
        "last_ms"))
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    assert "#define NDT2D_ABI_VERSION 4" in header and "Pose clusters" in header     # new symbols only
    assert "below 2^-40" in header                                                   # the weights that do not count
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
    # the binding's structures have the header's layout: 6 and 11 eight-byte fields (label and count share one)
    import ctypes as C
    assert C.sizeof(_capi.ClusterHeader) == 48 and C.sizeof(_capi.ClusterRecord) == 80
    assert _capi.ClusterRecord.mass.offset == 8 and _capi.ClusterRecord.var_theta.offset == 72
    unit = open(os.path.join(CLUSTER_DIR, "ndt2d_cluster.hip")).read()
    code = re.sub(r"//[^\n]*", "", unit)
    # every extern "C" body that can throw sits between the guards (last_error returns a stored string)
    assert code.count("NDT2D_C_TRY") == code.count("NDT2D_C_CATCH") == 9
    # integer atomics only: no atomic on a float or a double anywhere
    assert not re.search(r"atomicAdd\s*\(\s*(?:&\s*)?[a-z_>.-]*(?:double|float)|unsafeAtomic|atomicAdd_system|__hip_atomic_fetch_add", code)
    for call in re.findall(r"atomic(?:Add|Min|Max|CAS|Or)\s*\(([^,]+),", code):
        assert re.search(r"owner|slot_q|slot_count|root_q|root_count|ctrl|lab|st_slot|st_min|st_q|st_count", call), call
    # the arithmetic is plain C++: no HIP header and no HIP type in the header the kernels share
    fn = open(os.path.join(CLUSTER_DIR, "ndt2d_cluster_fn.h")).read()
    assert "hip_runtime" not in fn and "double2" not in fn and "__global__" not in fn and "fp contract(off)" in fn


def test_the_library_exports_the_new_symbols():
    import ctypes
    from ndt_2d_amd import _capi
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in _capi.SIGNATURES:
        if name.startswith("ndt2d_cluster_"):
            assert hasattr(lib, name), name
    assert _capi.lib().ndt2d_abi_version() == 4


def test_the_cpp_mirror_compiles_with_the_new_members(tmp_path):
    stub = os.path.join(str(tmp_path), "use.cpp")
    with open(stub, "w") as f:
        f.write('#include "particle_filter_hip.hpp"\n'
                "double use(ndt_2d_hip::ParticleFilterHip & p)\n"
                "{\n  const std::vector<ndt2d_cluster_record> & all = p.clusters();\n  p.clusters(4);\n"
                "  ndt_2d_hip::PoseClusterHip best;\n  if (!p.bestCluster(&best)) return 0.0;\n"
                "  return best.mean[0] + best.covariance[8] + best.share + static_cast<double>(all.size())\n"
                "         + static_cast<double>(p.clusterHeader().n_clusters);\n}\n")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *INCLUDES, stub],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    src = os.path.join(ROOT, "tests", "cpp", "cluster_mirror_check.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", *INCLUDES, src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
