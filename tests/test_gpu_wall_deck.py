"""absorb_tally and link_boundary on the C++ deck host: tests/decks/wall_probe.cxx (written for this test, deck API only)
against what the REFERENCE made of the same deck (tests/golden/wall_probe.npz, tools/gen_wall_golden.py).  The species
have q/m = 0 and are loaded with uniform_rand only, which the host reproduces bit for bit, so both absorb the same
particles in the same steps.  Held:

  nabs[] and n_out of every step               == the fixture's
  the link file                                the header byte for byte; its lines, sorted, == the fixture's sorted lines;
                                               every x is the +x wall's coordinate
  nabs plus the lines                          the particles lost, per species (from the dumps of the first and the last step)
  particle mirrors                             none came to the host between the first and the last step
  vpic_simulation::wall_tally                  its counts are nabs and the lines; its charge is count * q within half a quantum
                                               per particle (the quantum: the largest |q| loaded, times 2^-30)
  a second run in the same directory           stops with the reference's "already exists" message"""
import importlib
import importlib.util
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

N, STEPS = 3000, 12


def tool():
    spec = importlib.util.spec_from_file_location("gen_wall_golden", os.path.join(ROOT, "tools", "gen_wall_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def particles(path, n):
    L = importlib.import_module("old-vpic_amd.layout")
    p = np.fromfile(path, L.particle_t, offset=os.path.getsize(path) - n * L.particle_t.itemsize)     # the records end the file
    assert len(p) == n and (n == 0 or (p["tag"].min() >= 1 and p["tag"].max() <= N and len(np.unique(p["tag"])) == n)), path
    return p


def test_a_deck_tallies_and_links_like_the_reference(tmp_path):
    G = tool()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wall_probe.npz"))
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "wall_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "DECK_DEFS=-DWALL_PROBE_HIP_HOST", "OUT=" + str(tmp_path / "wall_probe")])
    exe = str(tmp_path / "wall_probe.hip.exe")
    r = subprocess.run([exe, "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=dict(os.environ, VPIC_HIP_HOST_TIMING="1"))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("wall_probe")))
    steps = G.parse_steps(r.stdout)
    assert steps.shape == gold["steps"].shape
    assert np.array_equal(steps, gold["steps"]), (steps.tolist(), gold["steps"].tolist())
    header, lines = G.parse_link(tmp_path / "link.0")
    assert header == bytes(gold["header"])
    assert len(lines) == len(gold["lines"]) and np.array_equal(lines, gold["lines"]), \
        [(a, b) for a, b in zip(lines, gold["lines"]) if a != b][:3]
    assert all(l.split()[1] == b"8.000000e+00" for l in lines)
    # the particles lost, per species (nabs[] follows id[]: heavy, light; species ids: light 0, heavy 1)
    for name, sid, nabs, left in (("light", 0, steps[-1, 2], steps[-1, 4]), ("heavy", 1, steps[-1, 1], steps[-1, 5])):
        p0, p1 = particles(tmp_path / ("%s.0.0" % name), N), particles(tmp_path / ("%s.%d.0" % (name, STEPS)), int(left))
        linked = sum(1 for l in lines if int(l.split()[0]) == sid)
        assert len(p0) == N and len(p0) - len(p1) == nabs + linked, (name, len(p0), len(p1), int(nabs), linked)
        assert np.all(np.isin(p1["tag"], p0["tag"]))
    # no particle mirror came to the host between the first and the last step
    d = [int(v) for v in re.findall(r"wall_probe: step \d+ mirror downloads (\d+)", r.stdout)]
    assert len(d) == STEPS + 1 and len(set(d[1:])) == 1, d
    # the accessor: counts are nabs and the lines of the species; the charge is count * q within half a quantum per particle
    acc = re.findall(r"wall_probe: step (\d+) light -x (\d+) (\S+) (\S+) \+x (\d+) (\S+) (\S+)", r.stdout)
    assert len(acc) == STEPS + 1
    last = acc[-1]
    linked_light = sum(1 for l in lines if int(l.split()[0]) == 0)
    assert int(last[1]) == steps[-1, 2] and int(last[4]) == linked_light
    q, quantum = float(np.float32(-0.002)), float(np.float32(0.0075)) * 2.0 ** -30
    for count, charge, energy in ((int(last[1]), float(last[2]), float(last[3])), (int(last[4]), float(last[5]), float(last[6]))):
        assert abs(charge - count * q) <= 0.5 * quantum * count + 1e-9 * abs(count * q), (count, charge)     # (the second term: ten printed digits)
        assert energy < 0                                                                                   # q < 0, ke > 0
    assert "wall sums refused 0" in r.stderr, r.stderr[-2000:]
    # a second run in the same directory: the link file is in the way
    r2 = subprocess.run([exe, "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r2.returncode != 0
    assert "File link.0 already exists (probably from a earlier run or recovery) ... Please move it or change link filename" in r2.stderr, r2.stderr[-2000:]


def test_a_restarted_deck_goes_on_tallying_and_linking(tmp_path):
    """dump_restart at step 6, then `deck.exe restart restart_wall` with the first run's link file moved away: the handlers,
    nabs[] and n_out come back from the restart file -- steps 7..12 print the fixture's nabs[] and n_out, the new link
    file's header is n_out of step 6, and its lines are the fixture's lines the first six steps did not write"""
    G = tool()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "wall_probe.npz"))
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "wall_probe.cxx")
    at = 6
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "DECK_DEFS=-DWALL_PROBE_HIP_HOST -DWALL_PROBE_RESTART_AT=%d" % at,
                           "OUT=" + str(tmp_path / "wall_probe_r")])
    exe = str(tmp_path / "wall_probe_r.hip.exe")
    r = subprocess.run([exe, "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert np.array_equal(G.parse_steps(r.stdout), gold["steps"]) and (tmp_path / "restart_wall.0").exists()
    _, whole = G.parse_link(tmp_path / "link.0")
    assert np.array_equal(whole, gold["lines"])
    os.rename(tmp_path / "link.0", tmp_path / "link_of_the_first_run.0")
    r = subprocess.run([exe, "restart", "restart_wall"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    steps = G.parse_steps(r.stdout)
    print(steps.tolist())
    assert list(steps[:, 0][-(STEPS - at):]) == list(range(at + 1, STEPS + 1)), steps[:, 0].tolist()
    for row in steps:
        assert np.array_equal(row, gold["steps"][row[0]]), (row.tolist(), gold["steps"][row[0]].tolist())
    header, lines = G.parse_link(tmp_path / "link.0")
    assert header == b"%% %17.0f\n" % gold["steps"][at, 3]
    assert len(lines) == gold["steps"][-1, 3] - gold["steps"][at, 3]
    want = sorted(gold["lines"].tolist())
    for l in lines.tolist():                                            # a sub-multiset of the fixture's lines
        assert l in want, l
        want.remove(l)
    # the accessor's totals came along: the counts of the last step are those of the uninterrupted run
    acc = re.findall(r"wall_probe: step (\d+) light -x (\d+) \S+ \S+ \+x (\d+) ", r.stdout)[-1]
    assert int(acc[0]) == STEPS and int(acc[1]) == gold["steps"][-1, 2] and int(acc[2]) == sum(1 for l in gold["lines"] if int(l.split()[0]) == 0)
