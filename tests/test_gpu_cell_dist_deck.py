"""Cell distributions on the C++ deck host: tests/decks/cell_dist_probe.cxx (written for this test, deck API only) sets a
magnetic and an electric field that vary in space, loads a species whose particles each have a weight of their own, runs
four steps, and at the last one writes the electrons' moments (dump_hydro), asks the host for a map over x and z given in
PHYSICAL units of the cells inside a y range (physical) and a |cB| range, with four sums beside the counts -- J.E, the
charge density from the hydro array, Ex times X in local cells, one, the first at a quantum that refuses part of the
cells (vpic_simulation::cell_distribution) -- and then writes
the field array (dump_fields).  The test restates the map from the deck's own two dumps with
test_cell_dist_ref.cell_distribution_ref, the descriptor converted to cells by hand, and compares every byte.

(The box's cells measure 2 x 1 x 0.5 from (-8, 0, 0), so the conversions between physical units and cells are exact.)"""
import glob
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_cell_dist_ref import cell_distribution_ref  # noqa: E402

pytestmark = pytest.mark.gpu
L = importlib.import_module("old-vpic_amd.layout")


def read_dump(pattern, dtype, nv):
    """the array at the end of a V0 dump file (header, array header, then nv records)"""
    (path,) = glob.glob(pattern)
    size = os.path.getsize(path)
    return np.fromfile(path, dtype, offset=size - nv * np.dtype(dtype).itemsize)


def test_map_equals_the_restatement_of_the_deck_s_own_dumps(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "cell_dist_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "cell_dist_probe")])
    r = subprocess.run([str(tmp_path / "cell_dist_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"cell_dist_probe: cells (\d+), kept (\d+), counted (\d+), through global memory (\d+)", r.stdout)
    assert m, r.stdout[-4000:]
    print(m.group(0))
    dims = (16, 8, 8)
    nv = L.nv(*dims)
    f = read_dump(str(tmp_path / "cell_dist_fields.*"), L.field_t, nv)
    h = read_dump(str(tmp_path / "cell_dist_hydro.*"), L.hydro_t, nv)
    assert len(f) == nv and len(h) == nv
    # the deck's descriptor in cells: x from -8 in bins of 4 with cells of 2, z from 0 in bins of 0.5 with cells of 0.5, 1 <= y < 7 with cells of 1
    desc = dict(axes=[("x", 0.0, 2.0, 8), ("z", 0.0, 1.0, 8)], select=[("y", 1.0, 7.0), ("b_c", 0.5, 10.0)])
    values = [(("jdote_c",), 1e-12), (("hydro.rho",), 1e-10), (("ex_c", "x"), 1e-9), (("one",), 1.0)]
    counts, isums, refused, (seen, kept, counted) = cell_distribution_ref(f, h, dims, desc, values)
    bins, n_val = 64, 4
    helper = (tmp_path / "cell_dist_helper.bin").read_bytes()
    assert len(helper) == 8 * bins + 8 * n_val * bins + 8 * 8
    got_counts = np.frombuffer(helper, np.uint64, bins).reshape(8, 8)
    got_isums = np.frombuffer(helper, np.int64, n_val * bins, 8 * bins).reshape(n_val, 8, 8)
    stats = np.frombuffer(helper, np.int64, 8, 8 * bins + 8 * n_val * bins)
    print(f"map: {counted} of {seen} cells counted, {kept} kept, {np.count_nonzero(counts)} of {bins} bins non-empty, refused {list(refused)}, "
          f"largest |sum| {[int(np.abs(s).max()) for s in isums]}; differing counts {int((got_counts != counts).sum())}, sums {int((got_isums != isums).sum())}")
    # the probe is worth something: the ranges leave cells out and keep others, every bin is populated, the first value
    # refuses some cells and takes others and the rest refuse none, the charge density is negative everywhere, and
    # the bins differ
    assert seen == 16 * 8 * 8 and 0.1 * seen < kept < 0.75 * seen and counted == kept and np.all(counts > 0)
    assert 0 < refused[0] < counted and list(refused[1:]) == [0, 0, 0]
    assert len(np.unique(isums[0])) > bins // 2 and np.all(isums[1] < 0) and len(np.unique(isums[1])) > bins // 2
    assert np.count_nonzero(isums[2]) > bins // 2 and np.array_equal(isums[3].astype(np.uint64), counts)
    assert np.array_equal(got_counts, counts)
    assert np.array_equal(got_isums, isums)
    assert list(stats) == [seen, kept, counted, 0] + list(refused)
    assert tuple(int(x) for x in m.groups()) == (seen, kept, counted, 0)
