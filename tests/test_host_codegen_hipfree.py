"""The kernel-description layer (exprgrad_amd/csrc/host: kd.cpp, codegen.cpp, match.cpp, epilogue.cpp and the row-fusion units
rowfuse_*.cpp) with the switch table and the error text is free of HIP: every unit compiles with plain g++ under -Wall -Werror
with only include/ and csrc/ on the include path (no ROCm directory), and neither the units nor any project header they
include names a <hip/...> header."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exprgrad_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
UNITS = ["host/kd.cpp", "host/codegen.cpp", "host/match.cpp", "host/epilogue.cpp", "switches.cpp", "error.cpp"] + \
    sorted(os.path.relpath(p, CSRC) for p in glob.glob(os.path.join(CSRC, "host", "rowfuse_*.cpp")))


def project_includes(path, seen):
    """path and, transitively, every header of the project it includes with quotes"""
    path = os.path.normpath(path)
    if path in seen:
        return
    seen.add(path)
    for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        for base in (os.path.dirname(path), CSRC, INCLUDE):
            if os.path.exists(os.path.join(base, name)):
                project_includes(os.path.join(base, name), seen)
                break
        else:
            raise AssertionError("%s includes %s, which is not in the project" % (path, name))


def test_the_row_fusion_units_are_all_listed():
    rowfuse = [u for u in UNITS if "rowfuse_" in u]
    assert len(rowfuse) >= 5 and not os.path.exists(os.path.join(CSRC, "host", "rowfuse.cpp")), rowfuse
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert set(UNITS) <= set(srcs), sorted(set(UNITS) - set(srcs))


@pytest.mark.parametrize("unit", UNITS)
def test_unit_compiles_without_hip(tmp_path, unit):
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I", INCLUDE, "-I", CSRC, os.path.join(CSRC, unit), "-o",
                          str(tmp_path / "unit.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]


def test_no_unit_reaches_a_hip_header():
    seen = set()
    for unit in UNITS:
        project_includes(os.path.join(CSRC, unit), seen)
    assert any(p.endswith("rowfuse.hpp") for p in seen) and any(p.endswith("exprgrad_hip.h") for p in seen)
    bad = [p for p in sorted(seen) if re.search(r"#\s*include\s*<hip/", open(p).read())]
    assert not bad, bad
    assert not [p for p in seen if p.endswith("eg_internal.hpp")]
