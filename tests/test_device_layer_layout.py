"""The device layer of the C ABI is csrc/device/: the context in one header, one translation unit per
concern, nothing included as a .hip, no kernel (which is what entitles it to sit outside the hash
of the kernel sources, bench.py source_hash), and buffers that release themselves."""
import os
import re

from ndt_2d_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ndt_2d_amd", "csrc")
DEVICE = os.path.join(CSRC, "device")
HEADER = os.path.join(DEVICE, "ndt2d_context.h")


def _read(path):
    with open(path) as f:
        return f.read()


def _code(path):
    """The file's text without its comments."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", _read(path), flags=re.S))


def _sources():
    for where, _, names in os.walk(CSRC):
        for name in sorted(names):
            if name.endswith((".hip", ".h", ".cpp")):
                yield os.path.join(where, name)


def _units():
    units = sorted(os.path.join(DEVICE, f) for f in os.listdir(DEVICE) if f.endswith(".hip"))
    assert len(units) >= 5, units
    return units


def test_the_old_files_are_gone_and_no_device_unit_is_included():
    assert not os.path.exists(os.path.join(CSRC, "ndt2d_device.hip"))
    assert not os.path.exists(os.path.join(CSRC, "starts", "ndt2d_device_view.hip"))
    units = {os.path.basename(u) for u in _units()}
    assert units
    # no file under csrc/ includes a .hip, of the device layer or of any other unit, and none is
    # listed as a header: what units share is in headers
    for path in _sources():
        for inc in re.findall(r'#\s*include\s*["<]([^">]+)[">]', _read(path)):
            assert not inc.endswith(".hip"), (path, inc)
    assert not [h for h in build.HEADERS if h.endswith(".hip")]


def test_the_context_is_defined_once_in_the_header_and_seen_by_the_device_units_only():
    where = [p for p in _sources() if re.search(r"\bstruct ndt2d_context\b", _read(p))]
    assert where == [HEADER], where
    assert len(re.findall(r"\bstruct ndt2d_context\b", _read(HEADER))) == 1
    includers = [p for p in _sources() if "ndt2d_context.h" in re.findall(r'#\s*include\s*"(?:[^"]*/)?([^"/]+)"', _read(p))]
    assert sorted(includers) == _units(), includers


def test_the_device_layer_holds_no_kernel():
    for path in _units() + [HEADER]:
        code = _code(path)
        for word in ("__global__", "__device__", "hipLaunchKernelGGL", "<<<"):
            assert word not in code, (path, word)


def test_build_lists_follow_the_directory():
    for unit in _units():
        assert "device/" + os.path.basename(unit) in build.SOURCES, unit
    assert HEADER in build.HEADERS
    assert not [h for h in build.HEADERS if h.startswith(DEVICE + os.sep) and h.endswith(".hip")]
    assert not [h for h in build.HEADERS if os.path.basename(h) in ("ndt2d_device.hip", "ndt2d_device_view.hip")]
    for unit in _units():
        text = _read(unit)
        if "NDT2D_TEST_MAYBE_FAIL(" in text or "NDT2D_TEST_HOOKS" in text:
            assert "device/" + os.path.basename(unit) in build.HOOKED_SOURCES, unit
    hooked = [s for s in build.HOOKED_SOURCES if s.startswith("device/")]
    assert len(hooked) >= 3 and all(s in build.SOURCES for s in hooked), hooked   # search, poses, the hook's setter


def test_buffers_release_themselves():
    header = _code(HEADER)
    for name in ("DeviceBuffer", "PinnedStage"):
        body = header[header.index("struct " + name):]
        body = body[:body.index("\n};")]
        assert "~" + name + "()" in body, name
        assert re.search(name + r"\(const " + name + r" &\) = delete;", body), name
    members = set()
    for decl in re.findall(r"^\s*(?:DeviceBuffer|PinnedStage) ([\w, ]+);", header, flags=re.M):
        members.update(m.strip() for m in decl.split(","))
    assert len(members) >= 37 and {"cells_global", "stage_grid", "tmp_noise"} <= members, sorted(members)
    unit = _code(os.path.join(DEVICE, "ndt2d_context.hip"))
    destroy = unit[unit.index("int ndt2d_destroy("):]
    destroy = destroy[:destroy.index("\n}\n")]
    assert "delete h;" in destroy and "hipStreamDestroy(h->own_stream)" in destroy
    for m in sorted(members):
        assert not re.search(r"h->" + m + r"\b", destroy), m
