"""near_bits() of the large search's beam table (csrc/ndt2d_near_bits.h) against the per-lane
near-boundary test of lane_beams, on the host.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")


def test_near_bits_equal_the_lanes_own_test_under_the_sanitizers(tmp_path):
    """tests/cpp/near_bits_check.cpp: a program of its own, built with the host compiler and
    -fsanitize=address,undefined (the sanitizer's runtime linked into the program), run directly.
    Designed K fractions (0, 3, 4, 5, 0xfff8 .. 0xffff, steps put on the band's ends, x fields that
    carry into y) on lattices of 8, 21, 100, 101, 255, 256 and 257 steps at cfg-1's and cfg-2's scale:
    every column's and row's bit equals the OR of the lanes' test."""
    exe = os.path.join(str(tmp_path), "near_bits_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "near_bits_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    m = re.search(r"(\d+) beams, (\d+) bits checked, (\d+) set, (\d+) lanes near on x, (\d+) on y, (\d+) beams with two carries",
                  done.stdout)
    assert m, done.stdout
    beams, checked, set_bits, near_x, near_y, carries = (int(v) for v in m.groups())
    assert beams >= 2 * 7 * 200 and 0 < set_bits < checked and near_x > 0 and near_y > 0 and carries > 0


def test_one_helper_three_callers():
    """The pre-kernel and the host check take the word from the one helper; the search's lanes keep
    their own test and only skip it where the word says no lane can pass it."""
    table = open(os.path.join(CSRC, "ndt2d_match_lane.hip")).read()
    assert "near_bits(k48," in table and "near_offset_units(" in table
    lane = open(os.path.join(CSRC, "ndt2d_lane_fn.h")).read()
    assert '#include "ndt2d_near_bits.h"\n' in lane and "near_possible >> u" in lane
    check = open(os.path.join(ROOT, "tests", "cpp", "near_bits_check.cpp")).read()
    assert '#include "ndt2d_near_bits.h"\n' in check and "ndt2d::near_bits(" in check
    from ndt_2d_amd import build
    assert os.path.join(CSRC, "ndt2d_near_bits.h") in build.HEADERS
