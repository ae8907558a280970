"""Where vpic_hip_collide collides a species -- in place or after a sort -- and which kernel instance it launches
(plan_collide in old-vpic_amd/csrc/policy.h), without a GPU: tests/collide_policy_check.cpp, built with the host
compiler, drives one named case per rule."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["exact_voxel_ranges_collide_in_place", "exact_tile_ranges_collide_in_place", "sorts_first_unsorted", "sorts_first_tile_only",
         "sorts_first_tail", "sorts_first_holes", "sorts_first_failed_check", "sorts_first_pending_fused_sort",
         "instance_by_fullest_cell", "over_the_cap_is_an_error"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("collide_policy")), "collide_policy_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "collide_policy_check.cpp"), "-o", exe])
    return exe


def test_policy_header_is_still_plain_cpp():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src and "__device__" not in src and "__global__" not in src
    assert "plan_collide" in src and "collide_ranges_exact" in src


def test_the_cap_and_the_wave_size_are_the_headers():
    """VPIC_HIP_COLLIDE_MAX_CELL of the header, COLLIDE_MAX_CELL of the package and of the numpy reference are one number;
    the wavefront instance ends at 64 particles of a species per cell"""
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    hdr = open(os.path.join(ROOT, "include", "vpic_hip.h")).read()
    cap = int(re.search(r"#define VPIC_HIP_COLLIDE_MAX_CELL (\d+)", hdr).group(1))
    V = importlib.import_module("old-vpic_amd")
    assert cap >= 1024 and V.COLLIDE_MAX_CELL == cap == V.layout.COLLIDE_MAX_CELL == importlib.import_module("collide_ref").MAX_CELL
    pol = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    assert re.search(r"COLLIDE_WAVE_CELL = 64;", pol)


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_collide_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
