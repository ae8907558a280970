"""Where advance_p finds a particle once positions and cells are 16-byte records (old-vpic_amd/csrc/record_offsets.h),
without a GPU: tests/record_offsets_check.cpp, built with the host compiler, drives the offset arithmetic at its limits --
the last tile of a 2^30-particle launch, the reference's order at 2^31 - 8192 particles, the lanes behind np."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["tile_at_the_top_of_a_launch", "reference_order_at_the_largest_species", "padding_lanes_behind_np",
         "reach_of_a_base", "sort_destination_anywhere"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("record_offsets")), "record_offsets_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "record_offsets_check.cpp"), "-o", exe])
    return exe


def test_offsets_header_is_plain_cpp_and_the_kernel_uses_it():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "record_offsets.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src and "__global__" not in src
    push = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "push.hip")).read()
    assert '#include "record_offsets.h"' in push
    for name in ("record_offset(", "word_offset(", "push_segment_particles(", "RECORD_SHIFT"):
        assert name in push, name


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_record_offsets(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
