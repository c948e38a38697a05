"""What the pose-graph calls refuse about their arguments, without a GPU: the header in a program of
its own (plainly and under the sanitizers), and its place in the build -- the five entry points take
every one of these texts from it and hold none themselves, and begin with the one prelude."""
import os
import re
import subprocess

from ndt_2d_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")
HEADER = os.path.join(CSRC, "posegraph", "ndt2d_posegraph_args.h")
UNITS = ["posegraph/ndt2d_posegraph.hip", "posegraph/ndt2d_posegraph_marginals.hip", "covariance/ndt2d_covariance.hip", "direct/ndt2d_direct.hip"]
# the fragments of the refusals that are written as literals
LITERALS = ['": job "', '" is not finite"', "i / 3 % n", '": the damping is negative or not finite"', '": a tolerance is negative or not finite"',
            '" names node "', '" poses, a dense matrix holds "', '": a job of "', '" bytes, the workspace is "']


def _code(path):
    return re.sub(r"//[^\n]*", "", open(path).read())


def test_the_args_header_in_a_program_of_its_own_and_under_the_sanitizers(tmp_path):
    """tests/cpp/posegraph_args_check.cpp over csrc/posegraph/ndt2d_posegraph_args.h: built with the host
    compiler, plainly and with -fsanitize=address,undefined (the runtime linked into the program), run
    directly, nothing preloaded.  Every refusal's text verbatim, the empty string for what is taken."""
    src = os.path.join(ROOT, "tests", "cpp", "posegraph_args_check.cpp")
    common = ["g++", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(CSRC, "posegraph"), "-I",
              os.path.join(CSRC, "covariance"), src]
    plain, sanitized = os.path.join(str(tmp_path), "args_check"), os.path.join(str(tmp_path), "args_check_san")
    subprocess.check_call(common + ["-O2", "-o", plain])
    subprocess.check_call(common + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-o", sanitized])
    for exe in (plain, sanitized):
        done = subprocess.run([exe], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stdout + done.stderr
        assert done.stdout.splitlines() == ["ok"], done.stdout
    text = _code(HEADER)
    assert "hip" not in text.lower().replace("__hipcc__", "") and "__global__" not in text and "#include <hip" not in text   # plain C++
    assert HEADER in build.HEADERS


def test_the_refusals_come_from_the_header_only():
    header = _code(HEADER)
    for literal in LITERALS:
        assert header.count(literal) == 1, literal
    for unit in UNITS:
        code = _code(os.path.join(CSRC, unit))
        assert '#include "posegraph/ndt2d_posegraph_args.h"' in code, unit
        for literal in LITERALS:
            if unit == "posegraph/ndt2d_posegraph.hip" and literal == '" is not finite"':
                continue   # (ndt2d_posegraph_set_graph's "pose I is not finite": the graph's own poses, another text)
            assert literal not in code, (unit, literal)
    solver = _code(os.path.join(CSRC, UNITS[0]))
    assert solver.count('" is not finite"') == 1 and "job " not in re.findall(r'[^\n]*" is not finite"[^\n]*', solver)[0]


def test_the_prelude_is_written_once():
    """pg_send_weights, pg_send_loss and pg_device_graph have one caller, pg_begin_call, which each of the
    five entry points calls; the chunk's poses are uploaded in one place."""
    state = _code(os.path.join(CSRC, "posegraph", "ndt2d_posegraph_state.h"))
    units = [_code(os.path.join(CSRC, u)) for u in UNITS]
    for name in ("pg_send_weights(", "pg_send_loss(", "pg_device_graph("):
        assert state.count(name) == 2, name                       # declared or defined, and called by pg_begin_call
        assert sum(u.count(name) for u in units) == (0 if name == "pg_device_graph(" else 1), name   # (the solver's unit defines the two)
    assert "pg_ready(" not in "".join(units[1:]) and units[0].count("pg_ready(") == 1
    assert [u.count("pg_begin_call(") for u in units] == [2, 1, 1, 1]
    assert [u.count("pg_chunk_poses(") for u in units] == [0, 1, 1, 0]
    assert not [u for u in units if "poses + k0 * n * 3" in u] and state.count("poses + k0 * n * 3") == 1
    # the objects beside the graph: one body each of create, release and the workspace's exact-size regrow
    for name in ("pg_companion_create(", "pg_companion_release(", "pg_companion_workspace("):
        assert state.count(name) == 1 and [u.count(name) for u in units] == [0, 0, 1, 1], name
    assert "hipMalloc(&s->d_workspace" not in "".join(units) and state.count("hipMalloc(&s->d_workspace, need)") == 1
