"""vpic_simulation::load_species_profile on the C++ deck host: tests/decks/load_probe.cxx (written for this test, deck API
only) loads a force-free-sheet electron species and a two-weight ion species from per-cell tables on one rank and an
8 x 8 x 16 grid, dumps both before the first step and after the fourth.  Held: counts per cell, q, positions, voxels and
tags == tests/load_ref.py; the momenta, taken back into the drift's rest frame, have the moments of the tables within 6
standard errors; no particle went from a host mirror to the device; the run completes with finite energies."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import load_ref as R  # noqa: E402

F = np.float32
DIMS, STEPS, SEED = (8, 8, 16), 4, 20261020


def dumped(path, n):
    L = importlib.import_module("old-vpic_amd.layout")
    p = np.fromfile(path, L.particle_t, offset=os.path.getsize(path) - n * L.particle_t.itemsize)     # the records end the file
    assert len(p) == n
    return p[np.argsort(p["tag"], kind="stable")]


def deck_tables():
    """the deck's tables, as it forms them"""
    k = np.arange(16)
    z = -8.0 + (k + 0.5) * 1.0
    col = lambda a, t: np.asarray(a, t).reshape(16, 1, 1)
    return dict(count=col(2 + k % 5, np.int32), sheet=col(np.where((k >= 6) & (k < 10), 5, 0), np.int32),
                udx=col(0.3 / np.cosh(z / 2.0), F), udy=col(0.3 * np.tanh(z / 2.0), F))


def rest_frame(p, ud):
    """the momenta boosted back by the cell's drift: w = u + ((gd - 1) (u . D) / D2 - gamma_u) D"""
    u = np.stack([p["ux"], p["uy"], p["uz"]], axis=1).astype(np.float64)
    D2 = (ud * ud).sum(axis=1)
    gd, gu = np.sqrt(1 + D2), np.sqrt(1 + (u * u).sum(axis=1))
    return u + (((gd - 1) * (u * ud).sum(axis=1) / D2 - gu))[:, None] * ud


def moments_hold(w, sigma, what):
    n = len(w)
    for k in range(w.shape[1]):
        x = w[:, k] / sigma
        print("%s component %d: mean %.4f (bound %.4f), variance - 1 %.4f (bound %.4f)" % (what, k, x.mean(), 6 / np.sqrt(n), (x * x).mean() - 1, 6 * np.sqrt(2.0 / n)))
        assert abs(x.mean()) <= 6 / np.sqrt(n) and abs((x * x).mean() - 1) <= 6 * np.sqrt(2.0 / n)


def test_a_deck_loads_its_species_on_the_device(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "load_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "load_probe")])
    r = subprocess.run([str(tmp_path / "load_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("load_probe")))
    t = deck_tables()
    e_ref = R.load(DIMS, t["count"], F(-1.0 / 64), (t["udx"], t["udy"], None), (F(0.05),) * 3, seed=SEED, stream=0, tag0=1)[0]
    bg_ref = R.load(DIMS, 4, F(1.0 / 64), None, (F(0.02),) * 3, seed=SEED, stream=1, tag0=1)[0]
    sh_ref = R.load(DIMS, t["sheet"], F(1.0 / 128), None, (F(0.05),) * 3, seed=SEED, stream=2, tag0=1000001)[0]
    i_ref = np.concatenate([bg_ref, sh_ref])
    n_e, n_i = len(e_ref), len(i_ref)
    assert n_e == 64 * int(t["count"].sum()) and n_i == 64 * (4 * 16 + 20)

    lines = re.findall(r"load_probe: step (\d+), electrons (\d+), ions (\d+), mirror uploads (\d+), energies (\S+) (\S+)", r.stdout)
    assert [int(l[0]) for l in lines] == [0, STEPS]
    for l in lines:
        assert (int(l[1]), int(l[2])) == (n_e, n_i) and int(l[3]) == 0          # no particle came from a host mirror
        assert all(np.isfinite(float(v)) and float(v) > 0 for v in l[4:])
    assert [int(v) for v in re.findall(r"dumped, mirror uploads (\d+)", r.stdout)] == [0, 0]

    e0, i0 = dumped(tmp_path / "electron.0.0", n_e), dumped(tmp_path / "ion.0.0", n_i)
    exact = ("dx", "dy", "dz", "i", "q", "tag", "tag2")
    for got, ref in ((e0, e_ref), (i0, i_ref)):
        for c in exact:                                                          # (sorted by tag: the call's order; counts per cell with them)
            assert np.array_equal(got[c].view("u%d" % got[c].dtype.itemsize), ref[c].view("u%d" % ref[c].dtype.itemsize)), c
    # the momenta: statistically.  Electrons back in their cell's rest frame, ions as they are (no drift)
    cz = e0["i"] // (10 * 10) - 1
    ud = np.stack([t["udx"].ravel()[cz], t["udy"].ravel()[cz], np.zeros(n_e)], axis=1).astype(np.float64)
    moments_hold(rest_frame(e0, ud), 0.05, "electrons")
    as_loaded = lambda p: np.stack([p["ux"], p["uy"], p["uz"]], axis=1).astype(np.float64)      # noqa: E731
    moments_hold(as_loaded(i0[:len(bg_ref)]), 0.02, "background ions")
    moments_hold(as_loaded(i0[len(bg_ref):]), 0.05, "sheet ions")
    # after four steps: every particle is still there and has moved
    e1, i1 = dumped(tmp_path / ("electron.%d.0" % STEPS), n_e), dumped(tmp_path / ("ion.%d.0" % STEPS), n_i)
    for a, b in ((e0, e1), (i0, i1)):
        assert np.array_equal(a["tag"], b["tag"]) and np.array_equal(a["q"], b["q"])
        assert all(np.all(np.isfinite(b[c])) for c in ("dx", "dy", "dz", "ux", "uy", "uz"))
    assert (e0["dx"] != e1["dx"]).mean() > 0.99
