"""vpic_simulation::collide on the C++ deck host: tests/decks/collide_probe.cxx (written for this test, deck API only)
collides its electrons among themselves and with its ions in begin_particle_collisions, every step for four steps, and
dumps both species before and after.  The species have q/m = 0, so the fields never act on them: only the collisions
change a momentum.  Held: no particle mirror comes to the host across the collisions; the total momentum m_e sum u_e +
m_i sum u_i per component stays within the bound of tests/test_gpu_collide.py::test_conservation, once per call (equal
weights; K = 4 WORST_P of tests/test_collide_ref.py's docstring); and the electrons' temperature anisotropy T_z / T_x,
loaded at 4, has moved towards 1 -- a direction only: nobody has a measured rate."""
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

from test_collide_ref import WORST_P  # noqa: E402

STEPS, N = 4, 8 * 8 * 8 * 48


def particles(path, n):
    import importlib
    L = importlib.import_module("old-vpic_amd.layout")
    p = np.fromfile(path, L.particle_t, offset=os.path.getsize(path) - n * L.particle_t.itemsize)     # the records end the file
    assert len(p) == n
    return p[np.argsort(p["tag"], kind="stable")]


def anisotropy(p):
    u = np.stack([p["ux"], p["uy"], p["uz"]], 1).astype(np.float64)
    t = u.var(0)
    return t[2] / t[0]


def test_a_deck_collides_on_the_device(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "collide_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "collide_probe")])
    r = subprocess.run([str(tmp_path / "collide_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    calls = re.findall(r"collide_probe: collisions of step (\d+), mirror downloads before (\d+), after (\d+)", r.stdout)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("collide_probe")))
    assert [int(s) for s, _, _ in calls] == list(range(STEPS))
    assert all(before == after for _, before, after in calls)       # no mirror came to the host for the collisions ...
    assert len({before for _, before, _ in calls}) == 1              # ... nor between them
    e0, i0 = particles(tmp_path / "electron.0.0", N), particles(tmp_path / "ion.0.0", N)
    e1, i1 = particles(tmp_path / ("electron.%d.0" % STEPS), N), particles(tmp_path / ("ion.%d.0" % STEPS), N)
    for a, b in ((e0, e1), (i0, i1)):
        assert np.array_equal(a["tag"], b["tag"]) and np.array_equal(a["q"], b["q"])
    mom = lambda e, i: np.array([1.0 * e[c].astype(np.float64).sum() + 100.0 * i[c].astype(np.float64).sum() for c in ("ux", "uy", "uz")])   # noqa: E731
    top = max(np.sqrt(sum(e0[c].astype(np.float64) ** 2 for c in ("ux", "uy", "uz")).max()),
              100.0 * np.sqrt(sum(i0[c].astype(np.float64) ** 2 for c in ("ux", "uy", "uz")).max()))
    # two calls per step: N electrons in the first, N + N particles in the second
    bound = STEPS * 4 * WORST_P * (N + 2 * N) * 2.0 ** -24 * top
    dp = mom(e1, i1) - mom(e0, i0)
    print("d(total momentum)", dp, "bound", bound, "of", mom(e0, i0))
    assert np.abs(dp).max() <= bound
    changed = (e1["ux"].view(np.uint32) != e0["ux"].view(np.uint32)).mean()
    rms = np.sqrt(((e1["ux"].astype(np.float64) - e0["ux"]) ** 2).mean())
    print("electrons changed", changed, "rms change of ux", rms, "anisotropy", anisotropy(e0), "->", anisotropy(e1))
    assert changed > 0.99 and rms > 1e-3                             # far above rounding (vth = 0.02)
    assert np.array_equal(i0["ux"], i1["ux"]) is False
    a0, a1 = anisotropy(e0), anisotropy(e1)
    assert 3.5 < a0 < 4.5 and abs(a1 - 1) < abs(a0 - 1) and a1 < 0.97 * a0
