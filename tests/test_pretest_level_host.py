"""The large search's pre-test against the wave's lowest skip level (csrc/ndt2d_pretest_level.h): the
helper's bound against the plain maximum of a box's bytes, on the host.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")


def test_level_bound_never_prunes_what_the_maximum_keeps_under_the_sanitizers(tmp_path):
    """tests/cpp/pretest_level_check.cpp: a program of its own, built with the host compiler and
    -fsanitize=address,undefined (the sanitizer's runtime linked into the program), run directly.
    Every single non-zero byte in every place of the 4 x 4 and the 8 x 8 box, 400,000 random boxes of
    either shape with every span, three million random masked OR words: against each of the 63 skip
    levels the helper's answer is never below the true maximum's, equal for a single byte; level 63
    always passes, an empty box never."""
    exe = os.path.join(str(tmp_path), "pretest_level_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pretest_level_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    m = re.search(r"(\d+) words, (\d+) single-byte boxes, (\d+) \(word, level\) pairs pass by the bound, (\d+) by the maximum, "
                  r"(\d+) kept for the OR alone", done.stdout)
    assert m, done.stdout
    words, singles, by_bound, by_maximum, conservative = (int(v) for v in m.groups())
    assert words >= 3_000_000 and singles == 255 * (16 + 64)
    # the bound keeps everything the maximum keeps, and a minority more (OR of unequal bytes)
    assert by_bound == by_maximum + conservative and 0 < conservative < by_maximum


def test_one_helper_for_the_kernels_and_the_host_check():
    """The search's chunk loop and the host check take the bound and the comparison from the one
    header; the box tests hand out the masked OR word they always formed."""
    lane = open(os.path.join(CSRC, "ndt2d_lane_fn.h")).read()
    assert '#include "ndt2d_pretest_level.h"\n' in lane
    assert "uint32_t patch_box_word(" in lane and "uint32_t strip_box_word(" in lane
    search = open(os.path.join(CSRC, "ndt2d_match_lane.hip")).read()
    assert "pretest_level_passes(pretest_level_bound(box_word), level_min)" in search
    check = open(os.path.join(ROOT, "tests", "cpp", "pretest_level_check.cpp")).read()
    assert '#include "ndt2d_pretest_level.h"\n' in check and "ndt2d::pretest_level_bound(" in check
    from ndt_2d_amd import build
    assert os.path.join(CSRC, "ndt2d_pretest_level.h") in build.HEADERS
