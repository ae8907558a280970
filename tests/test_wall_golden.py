"""tests/golden/wall_probe.npz is what the reference makes of tests/decks/wall_probe.cxx today: where the reference tree is
present, tools/gen_wall_golden.py's run is repeated and must give the committed fixture byte for byte.  Elsewhere the test is
skipped, and the fixture's own consistency is still held (CPU)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wall_probe.npz")


def tool():
    spec = importlib.util.spec_from_file_location("gen_wall_golden", os.path.join(ROOT, "tools", "gen_wall_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_fixture_is_the_reference_run(tmp_path):
    if not os.path.isdir("/root/reference/src") or not os.path.exists("/opt/conda/include/mpi.h"):
        pytest.skip("reference tree or MPI headers not present")
    G = tool()
    data = G.fixture_bytes(G.run_reference(str(tmp_path)))
    with open(FIXTURE, "rb") as f:
        assert f.read() == data


def test_the_fixture_adds_up():
    """nabs plus the link lines is the particles lost, per species; n_out grows by the lines; the header is n_out as the
    first write found it; every x in the file is the +x wall's"""
    g = np.load(FIXTURE)
    steps, lines = g["steps"], [l.decode().split() for l in g["lines"]]
    assert steps.shape == (13, 6) and list(steps[:, 0]) == list(range(13))
    assert bytes(g["header"]) == b"%% %17.0f\n" % 5
    assert steps[-1, 3] - steps[0, 3] == len(lines) > 300
    light, heavy = steps[0, 4] - steps[-1, 4], steps[0, 5] - steps[-1, 5]             # nabs[] follows id[]: heavy, light
    by_id = [sum(1 for l in lines if int(l[0]) == k) for k in (0, 1)]
    assert steps[-1, 2] + by_id[0] == light and steps[-1, 1] + by_id[1] == heavy
    assert min(steps[-1, 1], steps[-1, 2], by_id[0], by_id[1]) >= 100
    assert all(l[1] == "8.000000e+00" for l in lines)
    assert np.all(np.diff(steps[:, 1:4], axis=0) >= 0)
