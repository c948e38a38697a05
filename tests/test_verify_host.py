"""Host side of the match verification (csrc/verify/): the symbols, the plugin header, the build
lists, the restatement (tests/verify_restatement.py) pinned to the oracle's likelihood_point and to
the oracle's occupancy renderer, the plain-C++ ray header as a stand-alone program (once more
under the sanitizers) against the restatement, the C entry points' refusals that need no device,
the Python helpers against a stand-in matcher, and the validation of the inputs
tests/test_gpu_verify.py runs on the GPU.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import refine_restatement as R
import verify_cases as cases
import verify_restatement as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ndt2d_verify_create", "ndt2d_verify_destroy", "ndt2d_verify_last_error", "ndt2d_verify_run",
               "ndt2d_verify_set_neighbourhood", "ndt2d_verify_neighbourhood", "ndt2d_verify_set_gates", "ndt2d_verify_gates",
               "ndt2d_verify_set_rays", "ndt2d_verify_rays", "ndt2d_verify_set_timing", "ndt2d_verify_last_ms",
               "ndt2d_matcher_verify_scans", "ndt2d_matcher_verify", "ndt2d_matcher_set_verify_neighbourhood",
               "ndt2d_matcher_verify_neighbourhood", "ndt2d_matcher_set_verify_gates", "ndt2d_matcher_verify_gates",
               "ndt2d_matcher_set_verify_rays", "ndt2d_matcher_verify_rays")


def test_header_declares_and_library_exports_the_new_symbols():
    from ndt_2d_amd import _capi
    raw = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(ndt2d_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "typedef struct ndt2d_verify ndt2d_verify;" in text
    assert sorted(_capi.SIGNATURES) == sorted(declared)            # the bindings keep covering the header
    assert _capi.lib().ndt2d_abi_version() == 4                    # additions only
    values = dict(re.findall(r"#define NDT2D_(BEAM_[A-Z]+|VERIFY_[A-Z_0-9]+) (\w+)", text))
    assert values == {"BEAM_OFF": "0", "BEAM_UNSEEN": "1", "BEAM_OUTLIER": "2", "BEAM_INLIER": "3", "BEAM_PIERCED": "4",
                      "VERIFY_RECORD_U32": "8", "VERIFY_NO_CELL": "0xFFFFFFFFu"}
    assert (_capi.BEAM_OFF, _capi.BEAM_UNSEEN, _capi.BEAM_OUTLIER, _capi.BEAM_INLIER, _capi.BEAM_PIERCED) == \
        (V.OFF, V.UNSEEN, V.OUTLIER, V.INLIER, V.PIERCED) == (0, 1, 2, 3, 4)
    assert _capi.VERIFY_RECORD_U32 == V.RECORD_U32 == 8 and _capi.VERIFY_NO_CELL == V.NO_CELL == 0xFFFFFFFF
    # the contract is in the header
    for phrase in ("Match verification", "NDT2D_BEAM_UNSEEN", "2 err >= dy", "r^T I r <= gate_pierce", "dx - dy + 1",
                   "n_pierced, n_walked"):
        assert phrase in raw, phrase


def test_verify_hip_header_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "verify_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"), src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    assert "verify_hip.hpp" in open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "CMakeLists.txt")).read()
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "verify_hip.hpp")).read()
    assert "Eigen" not in text.replace("nothing of ROS or Eigen", "") and "rclcpp" not in text


def test_build_lists_and_the_shape_of_the_unit():
    from ndt_2d_amd import build
    csrc = os.path.join(ROOT, "ndt_2d_amd", "csrc")
    assert "verify/ndt2d_verify.hip" in build.SOURCES
    assert os.path.join(csrc, "verify", "ndt2d_verify_ray.h") in build.HEADERS
    assert os.path.join(csrc, "verify", "ndt2d_verify_kernel.h") in build.HEADERS
    text = open(os.path.join(csrc, "verify", "ndt2d_verify.hip")).read()
    kernel_text = open(os.path.join(csrc, "verify", "ndt2d_verify_kernel.h")).read()
    code, kernel = re.sub(r"//[^\n]*", "", text), re.sub(r"//[^\n]*", "", kernel_text)
    # the shared device functions, the batch host and the stage layout are used, not copied: the
    # host's words in the unit, the kernel's in its header, which the unit includes
    assert '#include "batch/ndt2d_batch_state.h"\n' in text and '#include "verify/ndt2d_verify_kernel.h"\n' in text
    assert '#include "verify/ndt2d_verify_ray.h"\n' in kernel_text and '#include "batch/ndt2d_installed_map.h"\n' in kernel_text
    # neither takes the search kernels' header, directly or through the search engine's: the unit compiles its own kernel only
    for header in ("ndt2d_batch_search.h", "ndt2d_batch_host.h"):
        assert header not in code and header not in kernel, header
    for used in ("BatchHost", "installed_grid(", "InstalledSource", "stage_layout(", "batch_round_trip(", "refine_jobs::refusal(",
                 "refine_jobs::plan_sent_scans(", "refine_jobs::copy_sent_scans("):
        assert used in code, used
    for used in ("cell_index<POW2>(", "record_exponent(", "verify::line_begin(", "verify::line_next(", "verify::approach(",
                 "__builtin_amdgcn_ballot_w64(", "__popcll("):
        assert used in kernel and used not in code, used
    installed = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "batch", "ndt2d_installed_map.h")).read())
    assert installed.count("struct InstalledSource") == 1 and "InstalledMap map(uint32_t) const" in installed
    assert "__global__" not in installed and "struct InstalledSource" not in open(os.path.join(csrc, "batch", "ndt2d_batch_search.h")).read()
    for absent in ("hipHostMalloc", "hipEventCreate", "hipEventRecord", "atomic", "__threadfence", "struct InstalledMap", "struct InstalledSource",
                   "while (true)", "while (1)", "for (;;)"):
        assert absent not in code and absent not in kernel, absent
    # one kernel, in the header; launched from the unit: pow2 / divide
    assert kernel.count("__global__") == 1 and code.count("__global__") == 0
    assert code.count("hipLaunchKernelGGL") == 2 and kernel.count("hipLaunchKernelGGL") == 0
    assert "template <bool POW2, uint32_t CELLS, class SOURCE>\n__global__" in kernel
    # the settings and what they refuse exist once, in the header; the setters are thin calls
    assert kernel.count("struct VerifySettings") == 1 and "a gate is negative or not finite" in kernel
    for copied in ("cells (1 or 9)", "a gate is negative", "(0 or 1)", "std::isfinite("):
        assert copied not in code, copied
    for setter in ("set_cells(\"ndt2d_verify_set_neighbourhood\"", "set_gates(\"ndt2d_verify_set_gates\"",
                   "set_rays(\"ndt2d_verify_set_rays\""):
        assert setter in code, setter
    # every extern "C" body that can throw sits between the guards (last_error returns a stored string)
    assert code.count("NDT2D_C_TRY") == code.count("NDT2D_C_CATCH") == 11
    # the ray is plain C++: no HIP header, no HIP type, no open loop
    ray = open(os.path.join(csrc, "verify", "ndt2d_verify_ray.h")).read()
    assert "hip_runtime" not in ray and "double2" not in ray and "while" not in re.sub(r"//[^\n]*", "", ray)
    # nothing at the top level of csrc/ is new (bench.source_hash() covers that directory)
    top = sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".h")))
    assert not [n for n in top if "verify" in n]


# ---- the restatement against the reference's own pins ----

def test_restated_m2_against_the_oracles_likelihood_point():
    """Neighbourhood 1: exp(-m2 / 2) of every on-grid beam is the oracle's likelihood_point to
    1e-12 (the project's score parity bound), and OFF / UNSEEN are exactly the beams where it
    returns 0.0 from an off-grid index or a cell of fewer than five points."""
    s = cases.scenario()
    grid, ndt = s["grid"], s["ref"].ndt
    worst, counted = 0.0, 0
    for pose in np.vstack([s["jobs"], [(3.4, 3.3, 1.0), (-3.9, 0.2, -2.0)]]):
        got = V.verify(grid, s["query"], pose, neighbourhood=1, rays=False)
        c, sn = R.cos_sin(pose[2])
        for i, b in enumerate(s["query"]):
            qx, qy = c * b[0] - sn * b[1] + pose[0], sn * b[0] + c * b[1] + pose[1]
            want = ndt.likelihood_point(qx, qy)
            index = ndt.getIndex(qx, qy)
            cls = int(got["classes"][i])
            if index < 0 or index >= grid.size_x * grid.size_y:
                assert cls == V.OFF and want == 0.0 and math.isinf(got["m2"][i])
            elif grid.cells[index][5] < 5:
                assert cls == V.UNSEEN and want == 0.0 and math.isinf(got["m2"][i])
            else:
                assert cls in (V.INLIER, V.OUTLIER) and int(got["cells"][i, 0]) == index
                dev = abs(math.exp(-0.5 * got["m2"][i]) - want)
                worst = max(worst, dev)
                counted += 1
                assert dev <= 1e-12, (tuple(pose), i, got["m2"][i], want)
                assert (cls == V.INLIER) == (got["m2"][i] <= 9.0)
        assert got["record"][6] == 0 and not got["pierced_mask"].any()             # rays off: nothing walked
    print("largest |exp(-m2 / 2) - likelihood_point| over %d beams: %.3e" % (counted, worst))
    assert counted > 1000        # (not vacuous: 720 of them at the true pose alone)


RENDER_BOUNDS = {"pow2": [0.5, -0.5, 0.5, -0.5], "divide": [2.25, 0.0, 0.75, 3.0]}


def _rendered_cells(d, bounds, start, end):
    """The cells orc_occupancy_render does not leave unknown for one scan of one beam."""
    L = O.lib()
    szp = C.POINTER(C.c_size_t)
    L.orc_occupancy_render.restype = None
    L.orc_occupancy_render.argtypes = [O._dp, C.c_double, C.c_double, O._dp, O._dp, szp, C.c_size_t, C.POINTER(C.c_uint32), O._dp,
                                       C.c_void_p]
    b = np.array(bounds, dtype=np.float64)
    pose = np.array([start[0], start[1], 0.0])
    point = np.array([[end[0] - start[0], end[1] - start[1]]])
    offsets = np.array([0, 1], dtype=np.uintp)
    wh = (C.c_uint32 * 2)()
    origin = np.zeros(2)
    data = np.zeros((d.size_y, d.size_x), dtype=np.int8)
    L.orc_occupancy_render(b.ctypes.data_as(O._dp), d.cell, 0.5, pose.ctypes.data_as(O._dp), point.ctypes.data_as(O._dp),
                           offsets.ctypes.data_as(szp), 1, wh, origin.ctypes.data_as(O._dp), data.ctypes.data_as(C.c_void_p))
    assert (wh[0], wh[1]) == (d.size_x, d.size_y) and tuple(origin) == tuple(d.origin)      # the bounds coincide with the NDT grid
    return set(int(v) for v in np.flatnonzero(data.ravel() != -1))


@pytest.mark.parametrize("which", ["pow2", "divide"])
def test_line_walk_against_the_oracles_renderer(which):
    """One-beam scans rendered by orc_occupancy_render with bounds and resolution that make its
    grid the NDT grid: the cells it does not leave unknown are exactly the restatement's visited
    cells -- for every (origin cell, end cell) pair of the 8 x 8 grid and every pair from six origins
    of the 7 x 13 one: all eight octants, both axes, the zero-length ray."""
    d = cases.designed(which)
    cells = [(gx, gy) for gy in range(d.size_y) for gx in range(d.size_x)]
    origins = cells if which == "pow2" else [(3, 6), (0, 0), (6, 12), (0, 12), (6, 0), (2, 9)]
    seen_steps = set()
    for o in origins:
        start = d.centre(*o)
        assert int(d.grid.index(np.array([start[0]]), np.array([start[1]]))[0]) == o[1] * d.size_x + o[0]
        for e in cells:
            want = set(y * d.size_x + x for x, y in V.line_cells(o[0], o[1], e[0], e[1]))
            got = _rendered_cells(d, RENDER_BOUNDS[which], start, d.centre(e[0], e[1], 0.25, 0.75))
            assert got == want, (o, e, sorted(got), sorted(want))
            line = V.line_cells(o[0], o[1], e[0], e[1])
            # (the renderer's form can stop one step short of the end cell, src/occupancy_grid.cpp:113-128:
            # inside the end's own 3 x 3, where nothing is tested)
            assert line[0] == o and max(abs(line[-1][0] - e[0]), abs(line[-1][1] - e[1])) <= 1
            assert len(line) <= abs(e[0] - o[0]) + abs(e[1] - o[1]) + 1
            seen_steps.add((np.sign(e[0] - o[0]), np.sign(e[1] - o[1]), abs(e[0] - o[0]) > abs(e[1] - o[1])))
    assert len(seen_steps) >= 8 + 4 + 1     # the octants, the half axes, the diagonals, the zero-length ray


# ---- the plain-C++ ray ----

def _ray_cases(d, poses, scans, job_scan):
    """The rays of a designed grid's jobs as the stand-alone program reads them, with what the
    restatement says of each."""
    lines, want = [], []
    grid = d.grid
    for pose, sc in zip(poses, job_scan):
        res = V.verify(grid, scans[sc], pose, neighbourhood=1, gate_inlier=cases.GATE_INLIER, gate_pierce=cases.GATE_PIERCE)
        c, s = R.cos_sin(pose[2])
        origin = int(grid.index(np.array([pose[0]]), np.array([pose[1]]))[0])
        for i, b in enumerate(scans[sc]):
            if not res["visited"][i]:
                continue
            qx, qy = c * b[0] - s * b[1] + pose[0], s * b[0] + c * b[1] + pose[1]
            own = int(grid.index(np.array([qx]), np.array([qy]))[0])
            lines.append("R %s %s %s %s %d %d %d %d %s" % (float(pose[0]).hex(), float(pose[1]).hex(), float(qx).hex(),
                                                           float(qy).hex(), origin % d.size_x, origin // d.size_x,
                                                           own % d.size_x, own // d.size_x, float(cases.GATE_PIERCE).hex()))
            want.append((res["visited"][i], [t[0] for t in res["tested"][i]],
                         int(res["cells"][i, 1]) if res["pierced_mask"][i] else -1, [t[1] for t in res["tested"][i]]))
    head = ["G %d %d" % (d.size_x, d.size_y)] + [" ".join(float(v).hex() for v in rec) for rec in d.cells6]
    return "\n".join(head + lines) + "\n", want


def test_plain_cpp_ray_against_the_restatement_and_under_the_sanitizers(tmp_path):
    """tests/cpp/verify_ray_check.cpp: a program of its own over csrc/verify/ndt2d_verify_ray.h,
    built with the host compiler, plainly and with -fsanitize=address,undefined (the sanitizer's
    runtime linked into the program), run directly on the designed grids' rays: visited, tested and
    pierced cells equal the restatement's, r^T I r has its bits."""
    src = os.path.join(ROOT, "tests", "cpp", "verify_ray_check.cpp")
    inc = os.path.join(ROOT, "ndt_2d_amd", "csrc", "verify")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", inc, src]
    plain, sanitized = os.path.join(str(tmp_path), "ray_check"), os.path.join(str(tmp_path), "ray_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    n_rays = n_pierced = 0
    for which in ("pow2", "divide"):
        d = cases.designed(which)
        text, want = _ray_cases(d, *d.jobs())
        path = os.path.join(str(tmp_path), which + ".txt")
        with open(path, "w") as f:
            f.write(text)
        for exe in (plain, sanitized):
            done = subprocess.run([exe, path], capture_output=True, text=True)
            assert done.returncode == 0 and not done.stderr, done.stdout[-2000:] + done.stderr
            out = done.stdout.rstrip().split("\n")
            assert out[-1] == "%d rays OK" % len(want) and "FAILED" not in done.stdout
            for ln, (visited, tested, pierced, values) in zip(out, want):
                parts = [p.split() for p in ln.split(" | ")]
                assert np.array_equal([int(v) for v in parts[0][1:]], visited), ln
                assert np.array_equal([int(v) for v in parts[1][1:]], tested), ln
                assert int(parts[2][1]) == pierced, ln
                got = [float.fromhex(v) for v in parts[3][1:]]
                assert np.array_equal(got, values, equal_nan=True), (ln, values)
        n_rays += len(want)
        n_pierced += sum(1 for w in want if w[2] >= 0)
    assert n_rays > 60 and n_pierced >= 4


# ---- the C entry points without a device ----

def test_entry_points_refuse_null_arguments_without_a_device():
    from ndt_2d_amd import _capi
    L = _capi.lib()
    out = C.c_void_p(0x1)
    assert L.ndt2d_verify_create(None, 4, C.byref(out)) == _capi.ERR_INVALID and not out.value
    assert L.ndt2d_verify_create(None, 4, None) == _capi.ERR_INVALID
    assert L.ndt2d_verify_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_verify_last_error(None) == b"null verify"
    assert L.ndt2d_verify_set_timing(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_verify_last_ms(None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_verify_set_neighbourhood(None, 9) == _capi.ERR_INVALID
    assert L.ndt2d_verify_neighbourhood(None, None) == _capi.ERR_INVALID
    assert L.ndt2d_verify_set_gates(None, 9.0, 1.0) == _capi.ERR_INVALID
    assert L.ndt2d_verify_gates(None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_verify_set_rays(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_verify_rays(None, None) == _capi.ERR_INVALID
    z = np.zeros(8)
    rec = np.zeros(8, dtype=np.uint32)
    recp = rec.ctypes.data_as(C.POINTER(C.c_uint32))
    off = np.array([0, 1], dtype=np.uintp)
    offp = off.ctypes.data_as(C.POINTER(C.c_size_t))
    assert L.ndt2d_verify_run(None, _capi.dptr(z), None, 1, _capi.dptr(z), offp, 1, recp, None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_verify_scans(None, _capi.dptr(z), None, 1, _capi.dptr(z), offp, 1, 0, recp, None, None, None, None,
                                        0) == _capi.ERR_INVALID
    assert not L.ndt2d_matcher_verify(None)
    assert L.ndt2d_matcher_set_verify_neighbourhood(None, 9) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_verify_neighbourhood(None, None) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_set_verify_gates(None, 9.0, 1.0) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_verify_gates(None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_set_verify_rays(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_verify_rays(None, None) == _capi.ERR_INVALID


# ---- the Python helpers ----

class StandInMatcher:
    """matchStarts with canned results; verifyScans records what it is asked."""

    def __init__(self, canned):
        self.canned = canned
        self.calls = []

    def matchStarts(self, starts, points):
        self.calls.append(("matchStarts", np.array(starts).copy()))
        return [dict(score=s, pose=np.array(p, dtype=np.float64), covariance=np.eye(3), best_index=b) for s, p, b in self.canned]

    def verifyScans(self, jobs, scans, job_scan=None, **kw):
        self.calls.append(("verifyScans", np.array(jobs, dtype=np.float64).copy(), len(scans), list(job_scan), kw))
        return [dict(n_beams=10, off=0, unseen=1, outlier=2, inlier=7, pierced=k, walked=10) for k in range(len(jobs))]


def test_relocalize_with_and_without_verification_and_the_explained_mask():
    from ndt_2d_amd import _capi, explained_mask, relocalize
    canned = [(-0.2, (0.01, 0.0, 0.0), 5), (-0.5, (0.0, 0.02, 0.001), 7), (0.0, (0.0, 0.0, 0.0), 2 ** 64 - 1)]
    starts = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.5], [2.0, 2.0, 1.0]])
    points = np.ones((6, 2))
    stub = StandInMatcher(canned)
    plain = relocalize(stub, points, starts)
    assert [c[0] for c in stub.calls] == ["matchStarts"] and all("verify" not in e for e in plain)
    stub2 = StandInMatcher(canned)
    checked = relocalize(stub2, points, starts, verify=dict(max_beams=0, gate_pierce=0.5))
    assert [c[0] for c in stub2.calls] == ["matchStarts", "verifyScans"]              # one extra call
    call = stub2.calls[1]
    assert call[2] == 1 and call[3] == [0, 0, 0] and call[4] == dict(max_beams=0, gate_pierce=0.5)
    assert [e["start"] for e in checked] == [e["start"] for e in plain] == [1, 0, 2]
    for k, (e, p) in enumerate(zip(checked, plain)):
        assert np.array_equal(call[1][k], e["pose"])                                  # verified at the corrected poses, in rank order
        assert e["verify"]["pierced"] == k and e["verify"]["inlier"] == 7
        for key in p:                                                                  # everything else bit for bit
            assert np.array_equal(e[key], p[key]), key
    assert relocalize(StandInMatcher([]), points, np.zeros((0, 3)), verify={}) == []
    result = dict(classes=np.array([0, 1, 2, 3, 3, 2], dtype=np.uint8), pierced_mask=np.array([0, 0, 0, 0, 1, 1], dtype=bool))
    assert list(explained_mask(result)) == [True, True, False, True, False, False]
    assert _capi.BEAM_OUTLIER == 2


# ---- fixture validation: the inputs of tests/test_gpu_verify.py, checked on the restatement ----

def _far_from_the_gates(res, gate_inlier=cases.GATE_INLIER, gate_pierce=cases.GATE_PIERCE):
    return V.near_gate(res, gate_inlier, gate_pierce) == []


@pytest.mark.parametrize("which", ["pow2", "divide"])
def test_designed_grids_hold_what_the_gpu_test_needs(which):
    d = cases.designed(which)
    assert (d.size_x, d.size_y) == ((8, 8) if which == "pow2" else (7, 13))
    assert (math.frexp(d.cell)[0] == 0.5) == (which == "pow2")           # a power of two, or not
    poses, scans, job_scan = d.jobs()
    grid = d.grid
    rx, ry = d.robot_cell
    for cells in (1, 9):
        results = [V.verify(grid, scans[sc], p, neighbourhood=cells) for p, sc in zip(poses, job_scan)]
        assert all(_far_from_the_gates(r) for r in results)
        r0 = results[0]
        # the twelve three-cell rays: a tested cell at Chebyshev distance 2 from the end, a scoring cell
        # at distance 1 that is not tested; the robot's own cell scores and is never tested
        assert grid.cells[ry * d.size_x + rx][5] >= 5
        for i, (dx, dy) in enumerate(cases.OCTANTS + cases.AXES):
            end = (rx + dx, ry + dy)
            line = [divmod(c, d.size_x)[::-1] for c in r0["visited"][i]]
            assert line[0] == (rx, ry)
            dist = [max(abs(end[0] - x), abs(end[1] - y)) for x, y in line]
            assert dist[:3] == [3, 2, 1] and len(line) <= 4
            at2, at1 = line[1], line[2]
            assert grid.cells[at1[1] * d.size_x + at1[0]][5] >= 5
            tested = [t[0] for t in r0["tested"][i]]
            assert tested == [at2[1] * d.size_x + at2[0]] and ry * d.size_x + rx not in tested
        # rays of 0, 1 and 2 cells: nothing is tested
        n12 = len(cases.OCTANTS + cases.AXES)
        for i in range(n12, n12 + len(cases.SHORT)):
            assert 1 <= len(r0["visited"][i]) <= 3 and r0["tested"][i] == []
        assert len(r0["visited"][n12]) == 1                              # the zero-length ray
        # long rays: several tested cells, some rays pierced and some walked to the end
        assert r0["pierced_mask"].any() and (~r0["pierced_mask"] & (np.array([len(t) for t in r0["tested"]]) > 0)).any()
        if which == "divide":
            assert max(len(t) for t in r0["tested"]) >= 2
            # a first cell that does not pierce, then one that does
            assert any(len(t) >= 2 and t[-1][1] <= cases.GATE_PIERCE for t in r0["tested"])
        # the degenerate cell: an outlier where a beam ends in it, never piercing
        deg = d.degenerate[1] * d.size_x + d.degenerate[0]
        ends = np.flatnonzero(r0["cells"][:, 0] == deg)
        assert cells == 9 or (len(ends) == 1 and r0["classes"][ends[0]] == V.OUTLIER)
        met = [v for t in r0["tested"] for c, v in t if c == deg]
        assert met and all(not v <= cases.GATE_PIERCE for v in met) and not (r0["cells"][:, 1] == deg).any()
        # off the grid and not finite: OFF, no ray
        assert list(r0["classes"][-7:]) == [V.OFF] * 7 and all(r0["visited"][i] == [] for i in range(len(scans[0]) - 7, len(scans[0])))
        assert r0["record"][6] == len(scans[0]) - 7
        # every class occurs
        # (with nine cells the dense middle of the grid leaves no beam unseen)
        assert all(r0["record"][k] > 0 for k in ((1, 2, 4) if cells == 1 else (1, 4))) and sum(int(r["record"][3]) for r in results) > 0
        # the column gx = 0
        col = results[2]
        assert all(c % d.size_x == 0 for v in col["visited"] for c in v) and col["record"][6] == d.size_y
        assert max(len(t) for t in col["tested"]) >= 1 and col["pierced_mask"].any()
        # the robot off the grid: nothing walked, the classes stand
        out = results[3]
        assert out["record"][6] == 0 and not out["pierced_mask"].any() and out["record"][0] == 12 and out["record"][1] < 12
        # the turned pose differs from the straight one
        assert not np.array_equal(results[1]["classes"], r0["classes"]) or not np.array_equal(results[1]["m2"], r0["m2"])
    # the corner cells with nine neighbours: clipped to four
    assert len(V.neighbours(grid, 0, 9)) == 4 and len(V.neighbours(grid, d.size_x * d.size_y - 1, 9)) == 4
    nine = V.verify(grid, scans[0], poses[0], neighbourhood=9)
    corner = [i for i, c in enumerate(np.asarray(grid.index(*(d.ray_targets()[:-7].T)))) if c in (0, d.size_x * d.size_y - 1)]
    assert len(corner) == 2 and all(nine["classes"][i] in (V.INLIER, V.OUTLIER) for i in corner)


def test_boundary_tie_and_wrap_grids():
    grid, pose, beams = cases.boundary_grid()
    below = float(np.nextafter(4.0, 0.0))
    on = V.verify(grid, beams[:1], pose, gate_inlier=4.0)
    assert on["m2"][0] == 4.0 and on["classes"][0] == V.INLIER
    assert V.verify(grid, beams[:1], pose, gate_inlier=below)["classes"][0] == V.OUTLIER
    ray = V.verify(grid, beams[1:], pose, gate_pierce=4.0)
    assert ray["tested"][0] == [(4 * 8 + 2, 4.0)] and ray["pierced_mask"][0] and ray["classes"][0] == V.UNSEEN
    assert not V.verify(grid, beams[1:], pose, gate_pierce=below)["pierced_mask"][0]
    grid, pose, beams = cases.tie_grid()
    tie = V.verify(grid, beams, pose, neighbourhood=9)
    assert tie["m2"][0] == 2.0 and int(tie["cells"][0, 0]) == 4 and tie["classes"][0] == V.INLIER
    assert V.cell_m2(grid.cells[4], 1.5, 1.5) == V.cell_m2(grid.cells[6], 1.5, 1.5) == 2.0
    assert V.verify(grid, beams, pose, neighbourhood=1)["classes"][0] == V.UNSEEN
    grid, pose, beams = cases.wrap_grid()
    wrap = V.verify(grid, beams, pose, neighbourhood=9)
    assert list(wrap["classes"]) == [V.UNSEEN, V.INLIER] and int(wrap["cells"][1, 0]) == 3 and wrap["m2"][1] == 2.0


def test_scenarios_on_cfg1_hold_their_conditions():
    """The true pose: >= 90 % inliers, <= 2 % pierced; + 1 m in x and + 0.3 rad: >= 10 % pierced
    each.  The pillar scenario: at least one pierced beam, every piercing cell within one cell of a
    pillar.  No value within 1e-8 of a gate.  The figures are printed (DESIGN.md 3.15 quotes them)."""
    s = cases.scenario()
    assert (s["grid"].size_x, s["grid"].size_y) == (41, 41) and len(s["query"]) == 720
    results = [V.verify(s["grid"], s["query"], p, neighbourhood=9) for p in s["jobs"]]
    for name, r in zip(("true pose", "+ 1 m in x", "+ 0.3 rad"), results):
        print("%-10s record %s" % (name, [int(v) for v in r["record"]]))
        assert _far_from_the_gates(r)
    n = 720.0
    assert results[0]["record"][4] >= 0.9 * n and results[0]["record"][5] <= 0.02 * n
    assert results[1]["record"][5] >= 0.1 * n and results[2]["record"][5] >= 0.1 * n
    for gate in (6.0, 9.0, 14.0):
        r = V.verify(s["grid"], s["query"], s["jobs"][0], neighbourhood=9, gate_inlier=gate, rays=False)
        print("true pose, gate_inlier %4.1f: %d inliers of 720 (%.1f %%)" % (gate, r["record"][4], r["record"][4] / 7.2))
    one = V.verify(s["grid"], s["query"], s["jobs"][0], neighbourhood=1)
    print("true pose, neighbourhood 1: record %s" % [int(v) for v in one["record"]])
    assert _far_from_the_gates(one)
    p = cases.pillar_scenario()
    r = V.verify(p["grid"], p["query"], p["jobs"][0], neighbourhood=9)
    print("pillars removed: record %s" % [int(v) for v in r["record"]])
    assert _far_from_the_gates(r) and r["record"][5] >= 1
    for cell in r["cells"][r["pierced_mask"], 1]:
        assert cases.near_a_pillar(p["grid"], cell), divmod(int(cell), 41)
