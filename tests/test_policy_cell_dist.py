"""The host decisions of the cell distributions (plan_cell_groups and plan_distribution_sums without values in
old-vpic_amd/csrc/policy.h), without a GPU: tests/cell_dist_policy_check.cpp, built with the host compiler, drives one named
case per rule -- no idle workgroup on a grid of a few cells, the cap on large grids, the LDS budget of a histogram alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["no_idle_workgroup", "capped", "no_values"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("cell_dist_policy")), "cell_dist_policy_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cell_dist_policy_check.cpp"), "-o", exe])
    return exe


def test_the_launch_uses_the_decisions():
    hip = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "cell_dist.hip")).read()
    assert "plan_cell_groups(c.cells, 64 * CELL_WAVES)" in hip and "constexpr int CELL_WAVES = 4;" in hip
    assert "plan_distribution_sums((long long)bins, n_val, VPIC_HIP_DIST_LDS_BINS)" in hip


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_cell_dist_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
