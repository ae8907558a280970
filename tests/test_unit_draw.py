"""The interval of the particle sources' generator (old-vpic_amd/csrc/unit_draw.h), without a GPU: tests/unit_draw_check.cpp,
built with the host compiler, walks all 2^24 values of r >> 8 and the ends of the 32-bit range and asserts 0 < unit_open < 1
-- a draw of exactly 1 would give a refluxed or emitted particle a normal momentum of exactly zero -- and the header's mix32
is held to the numpy restatement of the mixer include/vpic_hip.h states (tests/collide_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

CASES = ["every_value_is_strictly_inside", "ends_of_the_range_and_the_low_bits"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("unit_draw")), "unit_draw_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "unit_draw_check.cpp"), "-o", exe])
    return exe


def test_header_is_plain_cpp_and_the_sources_include_it():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "unit_draw.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src and "__global__" not in src
    assert '#include "unit_draw.h"' in open(os.path.join(ROOT, "old-vpic_amd", "csrc", "particles.hip")).read()


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_unit_open(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr


def test_mix32_is_the_stated_mixer(driver):
    from collide_ref import mix32
    x = [0, 1, 255, 256, 12345, 0x9e3779b9, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff]
    out = subprocess.run([driver, "--mix32"] + [str(v) for v in x], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [int(mix32(np.uint64(v))) for v in x]
