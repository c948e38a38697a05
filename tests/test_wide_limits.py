"""Host side of the wide search (csrc/wide/): the symbols in the header, the bindings and the
library, the refusals that need no device, the plugin mirror's instantiation, and what holds the
unit in the build.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_DIR = os.path.join(ROOT, "ndt_2d_amd", "csrc", "wide")
NEW_SYMBOLS = tuple("ndt2d_wide_" + n for n in ("create", "destroy", "last_error", "set_tile", "tile", "match", "read_image",
                                               "set_timing", "last_ms")) + ("ndt2d_matcher_match_wide", "ndt2d_matcher_wide")


def test_header_declares_and_library_exports_the_new_symbols():
    from ndt_2d_amd import _capi
    text = open(os.path.join(ROOT, "include", "ndt2d_hip.h")).read()
    assert "#define NDT2D_ABI_VERSION 4" in text                      # new symbols only
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ndt2d_[a-z0-9_]+)\s*\(", code))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert sorted(n for n in _capi.SIGNATURES if n.startswith("ndt2d_wide_")) == sorted(NEW_SYMBOLS[:-2])
    assert _capi.lib().ndt2d_abi_version() == 4
    assert "#define NDT2D_WIDE_DEFAULT_TILE_STEPS 16" in code and "#define NDT2D_WIDE_DEFAULT_PIXELS_PER_TILE" in code


def test_entry_points_refuse_null_arguments_without_a_device():
    from ndt_2d_amd import _capi
    L = _capi.lib()
    out = C.c_void_p(0x1)
    assert L.ndt2d_wide_create(None, 64, C.byref(out)) == _capi.ERR_INVALID and not out.value
    assert L.ndt2d_wide_create(None, 64, None) == _capi.ERR_INVALID
    assert L.ndt2d_wide_destroy(None) == _capi.ERR_INVALID
    assert L.ndt2d_wide_last_error(None) == b"null wide search"
    assert L.ndt2d_wide_set_tile(None, 8, 2) == _capi.ERR_INVALID
    assert L.ndt2d_wide_tile(None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_wide_set_timing(None, 1) == _capi.ERR_INVALID
    assert L.ndt2d_wide_last_ms(None, None, None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_wide_read_image(None, None, None, 0) == _capi.ERR_INVALID
    z = np.zeros(12)
    assert L.ndt2d_wide_match(None, _capi.dptr(z), _capi.dptr(z), 1, _capi.dptr(z), 1, _capi.dptr(z), 1, 0, _capi.dptr(z),
                              None, None, None) == _capi.ERR_INVALID
    assert L.ndt2d_matcher_match_wide(None, _capi.dptr(z), _capi.dptr(z), 1, 1.0, 0.05, 0.2, 0.01, 0, None, _capi.dptr(z),
                                      None, None, None) == _capi.ERR_INVALID
    assert not L.ndt2d_matcher_wide(None)


def test_the_plugin_mirror_compiles():
    src = os.path.join(ROOT, "tests", "stubs", "wide_search_instantiation.cpp")
    done = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stubs"), src],
                          capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr
    cmake = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "CMakeLists.txt")).read()
    assert "wide_search_hip.hpp" in cmake


def test_the_unit_is_built_hashed_and_keeps_its_rules():
    from ndt_2d_amd import build
    assert "wide/ndt2d_wide.hip" in build.SOURCES
    assert os.path.join(WIDE_DIR, "ndt2d_wide_fn.h") in build.HEADERS
    assert sorted(n for n in os.listdir(WIDE_DIR) if n.endswith((".hip", ".h"))) == ["ndt2d_wide.hip", "ndt2d_wide_fn.h"]
    unit = open(os.path.join(WIDE_DIR, "ndt2d_wide.hip")).read()
    code = re.sub(r"//[^\n]*", "", unit)
    # every extern "C" body that can throw sits between the guards
    assert code.count("NDT2D_C_TRY") == code.count("NDT2D_C_CATCH") == 7
    # fixed trees: no read-modify-write atomics anywhere in the unit
    assert not re.search(r"atomic(Add|Min|Max|CAS|Or|And|Exch|Inc)|__hip_atomic_fetch", code)
    # the exact kernel scores through the batched searches' walk and merges with their rule
    assert '#include "batch/ndt2d_walk_fn.h"' in unit and "lane_walk<C, POW2>(" in code and "merge_best(" in code
    assert "sum_chunks(" in code and "record_exponent" not in code
    # the stop rule and the refusals the header promises
    assert "0x1.0p-35" in code and "strictly ascending" in code and "2^26 pixels" in code and "8 x 8 cells" in code
    # the arithmetic is plain C++: no HIP header and no HIP type in the header the kernels share
    fn = open(os.path.join(WIDE_DIR, "ndt2d_wide_fn.h")).read()
    assert "hip_runtime" not in fn and "double2" not in fn and "__global__" not in fn
    # the grid is read through the view, and nothing is installed
    assert "installed_grid(" in code and "ndt2d_set_grid" not in code
