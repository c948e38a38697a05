"""Compile-only check of the resident map's C++ mirror (ndt_2d_amd/plugin/occupancy_map_hip.hpp)
against include/ndt2d_hip.h: the host compiler parses tests/stubs/occupancy_map_instantiation.cpp,
which uses every member.  No GPU and nothing of the reference is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_occupancy_map_hip_header_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "occupancy_map_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I",
                           os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
