"""vpic_simulation::cool on the C++ deck host: tests/decks/cool_probe.cxx (written for this test, deck API only) holds a
pair-plasma species at vth = 0.6 c in a uniform cB = (0.5, 0.5, 0.5), q/m = 0 so that only the cooling changes a momentum,
and cools it in begin_particle_collisions every step for four steps, with a dry call beside every applying one.  Held: no
particle mirror comes to the host across the calls or between them; sum |q| (gamma - 1), from dump_particles at step 0
and 4, fell by the sum of the returned energies within half a quantum per particle and call plus the double rounding of
the sums; the dry calls changed nothing (each returns what the applying call behind it returns, and two in a row return
the same); the mean gamma fell far above rounding; the planted particles with u exactly along B are bit-identical."""
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

from test_gpu_collide_deck import particles  # noqa: E402

STEPS, N_PLANTED = 4, 8
N = 8 * 8 * 8 * 48 + N_PLANTED
QUANTUM = 2.0 ** -58
NUM = r"([-+0-9.eE]+)"


def q_gamma_minus_one(p):
    u = np.stack([p["ux"], p["uy"], p["uz"]], 1).astype(np.float64)
    uu = (u * u).sum(1)
    return np.abs(p["q"]).astype(np.float64) * (uu / (np.sqrt(1.0 + uu) + 1.0))


def test_a_deck_cools_on_the_device(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "cool_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "cool_probe")])
    r = subprocess.run([str(tmp_path / "cool_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("cool_probe")))
    calls = re.findall(r"cool_probe: cooling of step (\d+), dry " + NUM + ", applied " + NUM + r", mirror downloads before (\d+), after (\d+)", r.stdout)
    assert [int(c[0]) for c in calls] == list(range(STEPS))
    assert all(c[3] == c[4] for c in calls)                          # no mirror came to the host for the cooling ...
    assert len({c[3] for c in calls}) == 1                           # ... nor between the calls
    dry, wet = [float(c[1]) for c in calls], [float(c[2]) for c in calls]
    again = re.findall(r"cool_probe: two dry calls behind the last, " + NUM + " and " + NUM, r.stdout)
    assert len(again) == 1
    # the dry calls changed nothing: each saw what the applying call behind it saw, and two in a row see the same
    assert dry == wet and all(e > 0 for e in wet)
    assert float(again[0][0]) == float(again[0][1]) and 0 < float(again[0][0]) < wet[-1]
    p0, p1 = particles(tmp_path / "electron.0.0", N), particles(tmp_path / ("electron.%d.0" % STEPS), N)
    assert np.array_equal(p0["tag"], p1["tag"]) and np.array_equal(p0["q"], p1["q"]) and np.all(np.abs(p0["q"]) == 2.0 ** -30)
    k0, k1 = q_gamma_minus_one(p0), q_gamma_minus_one(p1)
    fell, returned = k0.sum() - k1.sum(), sum(wet)
    # half a quantum per particle and call; each of the 2 n terms is formed in at most 8 roundings and the pairwise sums
    # add log2(n), each call's tally carries 4 more per particle relative to what it took
    slack = STEPS * N * QUANTUM / 2 + (8 + np.log2(N)) * 2.0 ** -53 * (k0.sum() + k1.sum()) + STEPS * 4 * 2.0 ** -53 * returned
    print("sum |q| (gamma - 1) fell by", fell, "returned", returned, "difference", fell - returned, "slack", slack)
    assert abs(fell - returned) <= slack
    g0 = 1.0 + k0 / np.abs(p0["q"])
    g1 = 1.0 + k1 / np.abs(p1["q"])
    print("mean gamma", g0.mean(), "->", g1.mean())
    assert 1.3 < g0.mean() < 2.5 and g1.mean() < g0.mean() - 0.01       # (float rounding of u: 1e-7)
    planted = p0["tag"] > 10 ** 6
    assert planted.sum() == N_PLANTED
    for c in ("ux", "uy", "uz"):
        assert p0[c][planted].tobytes() == p1[c][planted].tobytes()
        assert (p0[c][~planted].view(np.uint32) != p1[c][~planted].view(np.uint32)).mean() > 0.99
    assert np.all(p0["ux"][planted] == p0["uy"][planted]) and np.all(p0["ux"][planted] == p0["uz"][planted])
    assert sorted(np.abs(p0["ux"][planted]).tolist()) == [0.25, 0.25, 0.5, 0.5, 1.0, 1.0, 2.0, 2.0]
