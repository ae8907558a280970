"""The engine's host decisions (old-vpic_amd/csrc/policy.h: sort, push, the launch shapes of the species diagnostics) without a GPU: tests/policy_check.cpp, built with the
host compiler, drives one named case per rule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["row_window", "passes_per_wavefront", "tile_imbalance", "stage", "histogram", "sort_inside_fallback",
         "tail_regrouping", "instance", "tile_order", "flavour", "sort_plan", "sort_inside_or_before", "sort_due_rule",
         "early_sort", "chunks", "spectrum_window", "distribution_path", "distribution_tiles"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "policy_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "policy_check.cpp"), "-o", exe])
    return exe


def test_policy_header_is_plain_cpp():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
