"""The host side of the pose graph's robust losses without a GPU: ndt2d_robust_rho against known
answers in 60-digit decimal arithmetic, the refusals and the null handling of the four
ndt2d_robust_* entry points, their declarations, bindings and guards, the plain-C++ loss header in a
program of its own (plainly and under the sanitizers), the plugin mirror's setLoss, and the
restatement (tests/posegraph_robust_restatement.py) against itself on the designed cases of
tests/posegraph_robust_cases.py -- which is where those cases are held to what they are for."""
import ctypes as C
import decimal
import math
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_robust_cases as RC
import posegraph_robust_restatement as RR
from ndt_2d_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = decimal.Decimal
DBL_MIN = D(2.2250738585072014e-308)

# The worst error of ndt2d_robust_rho against the decimal answers over _known() below, in ulps of
# the answer, as measured (x86-64, glibc): 1.20 for Huber, 1.43 for Cauchy.  sqrt and the divisions
# are correctly rounded, log1p is within an ulp, and each value is two or three such operations.
# The test holds to twice the measured figure.
MEASURED_WORST_ULP = 1.43
SCALES = (1.0, 1.345, 0.05, 30.0)


def _rho3(kind, scale, s):
    out = np.zeros(3)
    rc = _capi.lib().ndt2d_robust_rho(kind.encode(), float(scale), float(s), _capi.dptr(out))
    assert rc == _capi.OK, (kind, scale, s, rc)
    return out


def _decimal_rho3(kind, scale, s):
    """{rho, rho', rho''} in 60 digits from the doubles scale and s, b the double a * a as the
    contract has it."""
    a, s, b = D(scale), D(s), D(scale * scale)
    if kind == "huber":
        if s <= b:
            return s, D(1), D(0)
        q = s.sqrt()
        w = max(DBL_MIN, a / q)
        return 2 * a * q - b, w, -w / (2 * s)
    x = s / b
    u = 1 + x
    w = max(DBL_MIN, 1 / u)
    # (60 digits cannot hold 1 + 1e-300: below 1e-25 log(u) is its series, whose next term is 1e-75 of it)
    log_u = x - x * x / 2 + x * x * x / 3 if x < D("1e-25") else u.ln()
    return b * log_u, w, -(w * w) / b


def _known(kind):
    for a in SCALES:
        b = a * a
        points = [0.0, 1e-300, 1.0, 1e300]
        if kind == "huber":
            points += [b, math.nextafter(b, math.inf), math.nextafter(b, -math.inf)]
        for s in points:
            yield a, s


def _ulps(got, want):
    want_f = float(want)
    if want_f == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return float(abs(D(got) - want) / D(math.ulp(want_f)))


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_rho_against_decimal_known_answers(kind):
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for a, s in _known(kind):
            got, want = _rho3(kind, a, s), _decimal_rho3(kind, a, s)
            for j in range(3):
                err = _ulps(got[j], want[j])
                worst = max(worst, err)
                assert err <= 2.0 * MEASURED_WORST_ULP, (kind, a, s, j, got[j], float(want[j]), err)
            assert got[1] > 0.0 and got[2] <= 0.0
    print("%s: worst error %.3f ulp" % (kind, worst))


def test_huber_is_continuous_across_b():
    for a in SCALES:
        b = a * a
        below, at, above = (_rho3("huber", a, s) for s in (math.nextafter(b, -math.inf), b, math.nextafter(b, math.inf)))
        assert at[0] == b and at[1] == 1.0 and at[2] == 0.0 and below[1] == 1.0
        assert abs(above[0] - at[0]) <= 4.0 * math.ulp(b) and abs(below[0] - at[0]) <= math.ulp(b)
        assert 1.0 - 4.0 * math.ulp(1.0) <= above[1] <= 1.0                  # rho' continuous to rounding
        assert above[2] < 0.0                                               # (rho'' is not: -1 / (2 b) beyond b)


def test_trivial_is_the_identity_and_ignores_nothing_else():
    assert _rho3("trivial", 3.0, 7.5).tolist() == [7.5, 1.0, 0.0]
    assert _rho3("trivial", 3.0, 0.0).tolist() == [0.0, 1.0, 0.0]


def test_refusals_and_null_objects_without_a_gpu():
    L = _capi.lib()
    out = np.full(3, 9.0)
    for kind, scale, s in ((b"tukey", 1.0, 1.0), (b"", 1.0, 1.0), (None, 1.0, 1.0), (b"huber", 0.0, 1.0), (b"huber", -1.0, 1.0),
                           (b"cauchy", math.inf, 1.0), (b"cauchy", math.nan, 1.0), (b"trivial", 0.0, 1.0), (b"huber", 1.0, -1e-300),
                           (b"huber", 1.0, math.inf), (b"cauchy", 1.0, math.nan)):
        assert L.ndt2d_robust_rho(kind, scale, s, _capi.dptr(out)) == _capi.ERR_INVALID, (kind, scale, s)
    assert out.tolist() == [9.0, 9.0, 9.0]
    assert L.ndt2d_robust_rho(b"huber", 1.0, 1.0, None) == _capi.ERR_INVALID
    assert L.ndt2d_robust_set_loss(None, b"huber", 1.0) == _capi.ERR_INVALID
    assert L.ndt2d_robust_select(None, None, 0) == _capi.ERR_INVALID
    scale = C.c_double(5.0)
    assert L.ndt2d_robust_loss(None, C.byref(scale)) == b"" and L.ndt2d_robust_loss(None, None) == b"" and scale.value == 5.0


def test_the_entry_points_are_declared_bound_guarded_and_hashed():
    header = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    assert "#define NDT2D_ABI_VERSION 4" in header
    for line in ("int ndt2d_robust_rho(const char * kind, double scale, double s, double * rho3_out);",
                 "int ndt2d_robust_set_loss(ndt2d_posegraph * posegraph, const char * kind, double scale);",
                 "const char * ndt2d_robust_loss(ndt2d_posegraph * posegraph, double * scale_out);",
                 "int ndt2d_robust_select(ndt2d_posegraph * posegraph, const uint8_t * robust, size_t m);",
                 "g = sum rho'_c J_c^T r_c", "This g is the exact gradient of F"):
        assert line in header, line
    names = sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_robust_"))
    assert names == ["ndt2d_robust_loss", "ndt2d_robust_rho", "ndt2d_robust_select", "ndt2d_robust_set_loss"]
    assert _capi.SIGNATURES["ndt2d_robust_loss"][0] is C.c_char_p
    assert os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_loss.h") in build.HEADERS
    assert "posegraph/ndt2d_posegraph_robust.hip" in build.SOURCES
    # the losses are used by the kernels' device functions (the kernel header) and by the four entry points' unit
    kernel = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_kernel.h")).read()
    assert '#include "posegraph/ndt2d_posegraph_loss.h"' in kernel and "pg::loss_weight<kLoss>(" in kernel
    unit = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_robust.hip")).read()
    assert '#include "posegraph/ndt2d_posegraph_loss.h"' in unit and "__global__" not in unit and "hipLaunchKernelGGL" not in unit
    solver = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph.hip")).read()
    assert "ndt2d_robust_" not in re.sub(r"//[^\n]*", "", solver)              # the family lives in one unit
    bodies = re.findall(r"\n(?:int|const char \*) ndt2d_robust_\w+\([^)]*\)\n\{\n(.*?)\n\}\n", unit, flags=re.S)
    assert len(bodies) == 4
    for body in bodies:
        if body.count("\n") > 1:                                           # every multi-line body sits in the guard
            assert body.lstrip().startswith("NDT2D_C_TRY") and "NDT2D_C_CATCH(" in body.splitlines()[-1], body[:80]
    assert sum("NDT2D_C_TRY" in body for body in bodies) == 3
    loss = open(os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph", "ndt2d_posegraph_loss.h")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", loss).lower().replace("__hipcc__", "")     # plain C++, no HIP types


def test_the_loss_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/posegraph_loss_check.cpp over csrc/posegraph/ndt2d_posegraph_loss.h: built with the
    host compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the
    program), run directly.  Its own checks: rho' and rho'' against central differences, the signs,
    monotony in s.  Here: every loss was run at every scale and the printed differences are small."""
    src = os.path.join(ROOT, "tests", "cpp", "posegraph_loss_check.cpp")
    inc = os.path.join(ROOT, "ndt_2d_amd", "csrc", "posegraph")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", inc, src]
    plain, sanitized = os.path.join(str(tmp_path), "loss_check"), os.path.join(str(tmp_path), "loss_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    outputs = []
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        assert done.stdout.splitlines()[-1] == "ok"
        outputs.append(done.stdout)
    rows = [line.split() for line in outputs[0].splitlines() if line.startswith("L ")]
    assert sorted({int(r[1]) for r in rows}) == [0, 1, 2] and len(rows) == 12
    for r in rows:
        assert float(r[3]) <= 1e-6 and float(r[4]) <= 1e-6, r
    assert [line.split()[:3] for line in outputs[1].splitlines() if line.startswith("L ")] == [r[:3] for r in rows]


def test_the_plugin_mirror_with_a_loss_compiles():
    stub = os.path.join(ROOT, "tests", "stubs", "pose_graph_loss_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "stubs"), stub], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    text = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "pose_graph_hip.hpp")).read()
    for member in ("void setLoss(const std::string & kind, double scale)", "ndt2d_robust_set_loss(", "ndt2d_robust_select("):
        assert member in text, member


def test_the_python_weights_are_robust_rhos_bit_for_bit():
    from ndt_2d_amd.pose_graph import robust_weights
    rng = np.random.default_rng(5)
    for kind in RR.KINDS:
        for a in SCALES:
            b = a * a
            s = np.concatenate([[0.0, 1e-300, 1.0, 1e300, 1.7e308, b, math.nextafter(b, math.inf), math.nextafter(b, -math.inf)],
                                b * 10.0 ** rng.uniform(-8, 8, 200)])
            want = np.array([_rho3(kind, a, v)[1] for v in s])
            assert np.array_equal(robust_weights(kind, a, s.reshape(2, -1)).reshape(-1), want), (kind, a)
    with pytest.raises(ValueError):
        robust_weights("tukey", 1.0, [1.0])


# ---- the restatement against itself ----

def test_the_restated_rho_is_the_librarys():
    rng = np.random.default_rng(3)
    s = np.concatenate([[0.0, 1.0, 1e-300, 1e300], 10.0 ** rng.uniform(-6, 6, 40)])
    for kind in RR.KINDS:
        for a in SCALES:
            want = np.array([_rho3(kind, a, v) for v in s])
            got = np.stack(RR.rho(kind, a, s), axis=1)
            assert np.all(np.abs(got - want) <= 4.0 * np.spacing(np.abs(want))), (kind, a)


@pytest.mark.parametrize("loss", RC.LOSSES)
def test_the_restated_gradient_is_the_costs(loss):
    """Central differences of the restated F with h = 1e-6: their own error is 1e-12 |F'''| and the
    rounding 1e-16 F / 1e-6; 1e-6 relative to the gradient's size holds both.  On the loop at its
    start (the false closure far out in the loss, the others inside) and beside its minimiser."""
    for x_of in (lambda P: P.poses, lambda P: RC.solution("loop40", loss, "reference")["x"] + 1e-3):
        P = RC.problem("loop40", loss, "reference")
        x = np.array(x_of(P))
        g, _ = P.gradient_hessian(x, hessian=False)
        f = np.nonzero(P.free())[0]
        rng = np.random.default_rng(1)
        for k in rng.choice(f, 12, replace=False):
            hi, lo = x.reshape(-1).copy(), x.reshape(-1).copy()
            hi[k] += 1e-6
            lo[k] -= 1e-6
            d = (P.cost(hi.reshape(-1, 3)) - P.cost(lo.reshape(-1, 3))) / (hi[k] - lo[k])
            assert abs(d - g[k]) <= 1e-6 * max(1.0, float(np.max(np.abs(g)))), (k, d, g[k])


@pytest.mark.parametrize("weighting", RC.WEIGHTINGS)
@pytest.mark.parametrize("loss", RC.LOSSES)
@pytest.mark.parametrize("case", RC.CASES)
def test_the_cases_are_what_they_are_for(case, loss, weighting):
    P, ref = RC.problem(case, loss, weighting), RC.solution(case, loss, weighting)
    g, truth, false = RC.graph(case)
    gate, floor = RC.GATES[(case, loss, weighting)]
    w = P.weights(ref["x"])
    others = np.delete(w, false)
    H = P.true_hessian(ref["x"])
    eig = np.linalg.eigvalsh(H)
    other = P.solve(lam0=1e-3, up=4.0, down=0.5)
    bound = 2.0 * ref["inverse_norm"] * (ref["gradient"] + other["gradient"])
    plain = RR.Problem(weighting=weighting, **g).solve()
    err = float(np.max(np.abs(ref["x"][:, :2] - truth[:, :2])))
    err_plain = float(np.max(np.abs(plain["x"][:, :2] - truth[:, :2])))
    print("%s %s %s: floor %.2e (gate %.0e) after %d iterations; rho' false %.4f, others >= %.4f; eig(H_true) >= %.3e; the schedules differ "
          "by %.2e (bound %.2e); from the truth %.4f, trivial %.4f" % (case, loss, weighting, ref["gradient"], gate, ref["iterations"], w[false],
                                                                        others.min(), eig.min(), float(np.max(np.abs(other["x"] - ref["x"]))),
                                                                        bound, err, err_plain))
    # the gate means something, and the restatement reaches it with a factor of 10 to spare
    assert ref["gradient"] <= 0.1 * gate and gate <= 1e-6 * ref["start_gradient"] and 0.5 * floor <= ref["gradient"] <= 2.0 * floor
    assert w[false] < 0.1 and others.min() > 0.9
    assert eig.min() > 0.0 and eig.min() > 1e-8 * eig.max()
    assert other["gradient"] <= 0.1 * gate and float(np.max(np.abs(other["x"] - ref["x"]))) <= bound
    assert 3.0 * err < err_plain


@pytest.mark.parametrize("name", sorted(RC.STRIDES))
def test_the_stride_graphs_gates(name):
    """The GPU suite runs no dense solve of these two; their gates are held to the restatement here."""
    P = RC.stride_problem(name)
    gate, floor = RC.STRIDES[name][3:]
    ref = P.solve(max_iterations=80)
    w = P.weights(ref["x"])
    print("%s: floor %.2e (gate %.0e) after %d iterations, rho' in [%.4f, %.4f]" % (name, ref["gradient"], gate, ref["iterations"], w.min(), w.max()))
    assert ref["gradient"] <= 0.1 * gate and gate <= 1e-6 * ref["start_gradient"] and 0.5 * floor <= ref["gradient"] <= 2.0 * floor
    if name == "chain1025":
        assert P.n == 1025 and P.m == 1026 and w[-1] < 0.2 and np.min(w[:-1]) > 0.9
    else:
        assert w.min() < 0.9


def test_a_selection_changes_the_restated_problem():
    sel = RC.closures("loop40")
    P = RC.problem("loop40", "huber", "reference", robust=sel, key="closures")
    s, _, w, _ = P.rho(P.poses)
    assert sel.sum() == 4 and np.all(w[~sel] == 1.0) and np.all(w[sel] <= 1.0) and w[RC.graph("loop40")[2]] < 0.1
    assert np.array_equal(P.rho(P.poses)[1][~sel], s[~sel])
    assert PC.INFO_FULL.shape == (3, 3)
