"""Syntax-checks the pluginlib shim against the reference's own interface headers
(include/ndt_2d/scan_matcher.hpp etc.).  Eigen3 / rclcpp / pluginlib are absent in
this image, so tests/stubs/ holds minimal stand-ins for THOSE (test-only).  The compiler
runs in build() (oracle/Makefile, _ref/syntax_*.txt), where the reference's headers are
present; its result travels with oracle/_ref/ and is read here."""
import hashlib
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("src", ["ndt_2d_amd/plugin/scan_matcher_ndt_hip.cpp",
                                 "tests/stubs/shim_instantiation.cpp"])
def test_shim_compiles_against_reference_interface(src):
    name = os.path.splitext(os.path.basename(src))[0]
    result = os.path.join(ROOT, "oracle", "_ref", "syntax_%s.txt" % name)
    if not os.path.exists(result):
        pytest.skip("oracle/_ref/syntax_%s.txt not built (build() needs the reference's headers)" % name)
    lines = open(result).read().splitlines()
    with open(os.path.join(ROOT, src), "rb") as f:
        want = hashlib.sha256(f.read()).hexdigest()
    assert lines[0].split()[0] == want, "%s changed since build() checked it: run build() again" % src
    assert lines[-1] == "exit 0", "\n".join(lines[1:])
    assert len(lines) == 2, "\n".join(lines[1:-1])


def test_plugins_xml_registers_against_the_reference_base_class():
    xml = open(os.path.join(ROOT, "ndt_2d_amd", "plugin", "plugins.xml")).read()
    assert 'base_class_type="ndt_2d::ScanMatcher"' in xml
    assert 'type="ndt_2d_hip::ScanMatcherNDTHip"' in xml
