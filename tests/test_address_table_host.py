"""The large search's window table of record addresses (csrc/ndt2d_address_table.h): the table's
builder against the per-cell route it replaces, on the host.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ndt_2d_amd", "csrc")


def test_table_equals_the_per_cell_route_under_the_sanitizers(tmp_path):
    """tests/cpp/address_table_check.cpp: a program of its own, built with the host compiler and
    -fsanitize=address,undefined (the sanitizer's runtime linked into the program), run directly.
    Over every cell of the padded window -- windows that are the whole grid, sit at each of its
    corners, far from its origin, hold one cell, and random ones; grids of 41 x 41, 37 x 53, 53 x 37
    and smaller, with random occupancy, one cell, every cell, the first and last row and column --
    the entry is records + 48 * rank_table[bit 0 ? row * size_x + col - idx_bias : -1]; the filler
    columns and "outside" hold the sentinel's address; the near-boundary path's entry of a grid cell
    gives that cell's record and the sentinel's for a point off the grid."""
    exe = os.path.join(str(tmp_path), "address_table_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "address_table_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.rstrip().endswith("OK") and "FAILED" not in done.stdout and not done.stderr, done.stdout + done.stderr
    m = re.search(r"(\d+) windows with ranks in a byte, (\d+) windows, (\d+) window cells \((\d+) outside the grid, (\d+) at the sentinel\), "
                  r"(\d+) near cells \((\d+) beyond the window\)", done.stdout)
    assert m, done.stdout
    byte_windows, windows, cells, outside, sentinel, near, beyond = (int(v) for v in m.groups())
    # the cases do what they are for: padding outside the grid, cells that cannot score, cells that can
    assert 0 < byte_windows < windows and windows > 1000 and 0 < outside < sentinel < cells and 0 < beyond < near


def test_one_builder_for_the_kernels_and_the_host_check():
    """The search's staging loop, its exact path and the host check take the table from the one header."""
    lane = open(os.path.join(CSRC, "ndt2d_lane_fn.h")).read()
    assert '#include "ndt2d_address_table.h"\n' in lane
    assert "address_table_entry(c.table," in lane and "address_table_entry_of_cell(c.table," in lane
    search = open(os.path.join(CSRC, "ndt2d_match_lane.hip")).read()
    assert "address_table_rank(g.cell_rank," in search and "address_table_bytes(" in search
    check = open(os.path.join(ROOT, "tests", "cpp", "address_table_check.cpp")).read()
    assert '#include "ndt2d_address_table.h"\n' in check and "ndt2d::address_table_rank(" in check
    from ndt_2d_amd import build
    assert os.path.join(CSRC, "ndt2d_address_table.h") in build.HEADERS
