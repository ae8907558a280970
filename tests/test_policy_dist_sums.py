"""Which path the per-bin sums of a histogram take (plan_distribution_sums in old-vpic_amd/csrc/policy.h), without a GPU:
tests/dist_sums_policy_check.cpp, built with the host compiler, drives one named case per rule -- the whole histogram in
LDS up to the boundary word count and global adds one bin beyond it, for one to four values."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["boundary_per_value_count", "boundary_word_count", "lds_never_above_budget", "largest_histogram"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("dist_sums_policy")), "dist_sums_policy_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dist_sums_policy_check.cpp"), "-o", exe])
    return exe


def test_the_decision_stands_beside_plan_distribution():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
    assert src.index("inline DistPlan plan_distribution(") < src.index("inline DistSumsPlan plan_distribution_sums(")
    # the budget the kernel is launched with is the header's
    text = open(os.path.join(ROOT, "include", "vpic_hip.h")).read()
    assert "#define VPIC_HIP_DIST_LDS_BINS 8192\n" in text
    hip = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "distribution.hip")).read()
    assert "plan_distribution_sums((long long)bins, n_val, VPIC_HIP_DIST_LDS_BINS)" in hip


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_dist_sums_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
