"""vpic_hip_step -- the call bench.py times -- held to the oracle step by step on every sort decision it makes by itself
(GPU box only).  Every case runs through step_ref.SteppedRun: before every step the oracle is restarted from the engine's
own state, so particles are compared bit for bit, the accumulator against the exact sums (every word in deterministic
mode, ACC_TOL of the largest sum in float mode) and fields and interpolator without any tolerance (tests/step_ref.py states
the three criteria; tests/test_step_ref.py checks the harness on the CPU).  Every case also asserts that the path it is
named for ran, from what the engine reports: species_stats, species_order and the count of launches that sorted as they
pushed.  No API reports which advance_p instance a launch was, nor whether an appended tail was regrouped before its push:
REACHES below DECLARES the instances a case is built to reach (from policy.h's rules and the asserted facts), it does not
observe them, and the two VPIC_HIP_TAIL_SORT_MIN settings of test_arrivals are held to the same facts.

The clumped case: a tile must hold more than 65536 particles for the engine to leave the tile order (policy.h:
plan_push), a thousand per cell, and the ORACLE's own float sums of so many equal terms are already at 0.6 - 0.9 of ACC_TOL
from the exact ones (tests/test_step_ref.py wants at most half on every float deck).  Deterministic mode runs the
equal-charge deck, every word exact; float mode runs the deck with the charge spread (step_ref._clumped_spread says what
that costs criterion 2)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import step_ref as S  # noqa: E402
from step_ref import D, L, pyorc  # noqa: E402
from species_states import package  # noqa: E402

gpu = pytest.mark.gpu                   # (every test but the coverage test, which is plain logic and runs anywhere)
SCALE = pyorc.fixed_scale(S.Q0)
MODES = ("float", "deterministic")
KNOBS = ("VPIC_HIP_SORT_IN_PUSH", "VPIC_HIP_WINDOW", "VPIC_HIP_TILE_COARSE", "VPIC_HIP_STAGE", "VPIC_HIP_EARLY_SORT",
         "VPIC_HIP_TAIL_SORT_MIN", "VPIC_HIP_NO_TAIL_SORT", "VPIC_HIP_FOLLOW", "VPIC_HIP_ITERS", "VPIC_HIP_OLD_SORT")


@pytest.fixture(scope="module")
def V():
    return package()


class Run:
    """An engine with a deck of the matrix uploaded (in the deck's random array order, nothing sorted) and its SteppedRun"""

    def __init__(self, V, monkeypatch, deck, mode, env=None, room=0):
        for k in KNOBS:                                            # the knobs are read when the engine is created
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, str(v))
        self.dims, self.walls, args, kw, self.og, species = S.deck(deck)
        self.mode = mode
        e = self.e = V.Engine(V.make_grid(*args, **kw))
        e.set_vacuum()
        e.set_accumulation(mode, S.Q0)
        e.set_sort_order("engine")
        e.profile_enable(True)
        self.sps = []
        for sp in species:
            n = len(sp["p"])
            k = e.new_species(sp["q_m"], n + room + 64, n + room + 64)
            e.set_particles(k, sp["p"])
            self.sps.append(k)
        e.load_interpolator()
        meta = [dict(sp=k, q_m=sp["q_m"], tagged=sp["tagged"]) for k, sp in zip(self.sps, species)]
        self.run = S.SteppedRun(e, self.og, pyorc.vacuum_coefficients(), meta, SCALE if mode == "deterministic" else None)
        self.facts = []

    def advance(self, k, interval):
        self.facts.append(self.run.advance(k, interval))
        return self.facts[-1]

    def steps(self, n, interval, first=0):
        for k in range(first, first + n):
            self.advance(k, interval)

    def sorts(self):
        return [[st["sorts"] for st in f["species_stats"]] for f in self.facts]

    def orders(self):
        return [self.e.species_order(sp) for sp in self.sps]

    def sorting_launches(self):
        return self.e.profile_read_sorting()[1]

    def stats(self, key):
        return [self.e.species_stats(sp)[key] for sp in self.sps]

    def close(self):
        self.e.close()


def scheduled(r, interval):
    """every species was sorted on every interval-th step; whatever else it was sorted for, the engine booked as a sort ahead
    of the interval (a hot species misses its tiles' windows within a step or two: policy.h, early_sort)"""
    for k, f in enumerate(r.facts):
        for st in f["species_stats"]:
            assert st["sorts"] - st["early_sorts"] == k // interval + 1, (k, st)
    return True


def sorted_by_voxel(r):
    """the species is in the reference's order: a push leaves no partition behind (order "none" after a step, never "tile"),
    and a sort asked for now, with the choice left to the engine, is by voxel"""
    assert r.orders() == ["none"] * len(r.sps)
    for sp in r.sps:
        r.e.sort_p(sp)
    assert r.orders() == ["voxel"] * len(r.sps)
    return True


def crossing(r):
    """something happened in every step: particles changed cell"""
    assert all(sum(f["crossed"]) > 0 for f in r.facts)


# ---- which advance_p instances (policy.h: PushInstance) each case is built to reach, per accumulation mode: a DECLARATION
# (see the module's docstring), kept complete by the coverage test below ------------------------------------------------------
REACHES = {
    "fused": {"float": {"tile", "tile_hist", "tile_sort"}, "deterministic": {"det_tile"}},
    "before": {"float": {"tile", "tile_hist"}},
    "measured": {"float": {"tile", "tile_hist", "tile_sort"}},
    "tagged": {"float": {"tile", "tile_hist"}, "deterministic": {"det_tile"}},
    "every_step": {"float": {"tile"}},
    "never": {"float": {"row_narrow"}},
    "early": {"float": {"tile"}, "deterministic": {"det_tile"}},
    "adaptive": {"float": {"tile"}, "deterministic": {"det_tile"}},
    "coarse": {"float": {"tile_only"}, "deterministic": {"det_tile_only"}},
    "rows": {"float": {"row_narrow", "row_wide"}},
    "thin": {"float": {"row_narrow", "row_wide"}, "deterministic": {"det_row"}},   # (wide from the second push on: 0.4 cross)
    "walls": {"float": {"tile", "tile_hist"}, "deterministic": {"det_tile"}},
    "reflect": {"float": {"tile", "tile_hist"}, "deterministic": {"det_tile"}},
    "chargeless": {"float": {"chargeless", "tile"}, "deterministic": {"chargeless", "det_tile"}},
    "clumped": {"float": {"tile", "row_narrow"}, "deterministic": {"det_tile", "det_row"}},
    "arrivals": {"float": {"tile", "tile_hist", "tile_sort"}, "deterministic": {"det_tile"}},
    "back_to_tiles": {"deterministic": {"det_tile"}},
}
WALL_DECKS = ["walls_ragged_ax", "walls_ragged_az", "walls_long_ax", "walls_long_az"]
# the decks of the cases, by test
DECK_OF = {"fused": "beams", "before": "beams", "measured": "beams", "tagged": "hot_tagged", "every_step": "beams", "never": "beams",
           "early": "hot_tagged", "adaptive": "hot", "coarse": "hot", "rows": "hot", "thin": "thin", "walls": WALL_DECKS,
           "reflect": "hot_reflect", "chargeless": "chargeless", "clumped": {"float": "clumped_spread", "deterministic": "clumped"}, "arrivals": "beams", "back_to_tiles": "hot_tagged",
           # (float compares counts, not tags: the untagged deck, whose sorts can happen inside the push)
           "no_read_between_steps": {"float": "beams", "deterministic": "beams_tagged"}}


def test_the_cases_cover_every_instance_every_grid_both_modes_every_wall_layout():
    src = open(os.path.join(S.ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    names = {n.strip() for n in re.search(r"enum class PushInstance \{([^}]*)\}", src).group(1).split(",")}
    assert len(names) == 10 and "tile_sort" in names             # (the phased pushes launch these same instances in two parts)
    reached = set().union(*[v for c in REACHES.values() for v in c.values()])
    assert reached == names, names ^ reached
    assert {m for c in REACHES.values() for m in c} == set(MODES)
    used = {d for v in DECK_OF.values() for d in ([v] if isinstance(v, str) else v.values() if isinstance(v, dict) else v)}
    assert used == set(S.DECKS)                                   # (every deck the CPU tests vouch for is run, and no other)
    assert {S.DECKS[d][0] for d in used} == {S.MAIN, S.RAGGED, S.THIN, S.LONG, (16, 16, 16)}
    assert {S.DECKS[d][0] for d in WALL_DECKS} == {S.RAGGED, S.LONG}
    assert {S.DECKS[d][1] for d in WALL_DECKS} == {"absorb_x_reflect_z", "reflect_y_absorb_z"}
    assert {S.DECKS[d][1] for d in used} == set(D.WALLS)
    tests = {n[len("test_"):] for n in globals() if n.startswith("test_")}
    assert set(REACHES) <= tests and set(DECK_OF) <= tests and set(REACHES) <= set(DECK_OF), set(REACHES) ^ set(DECK_OF)


# ---- fixed intervals: the sort inside the push, before it, either ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES)
def test_fused(V, monkeypatch, mode):
    """interval 4: step 3 counts for the sort, step 4 sorts inside its push -- in float mode; never in deterministic mode"""
    r = Run(V, monkeypatch, DECK_OF["fused"], mode, {"VPIC_HIP_SORT_IN_PUSH": 1})
    r.steps(9, 4)
    crossing(r)
    assert r.sorts()[-1] == [3, 3] and r.orders() == ["tile", "tile"]
    if mode == "float":
        assert r.sorting_launches() >= 2
    else:
        assert r.sorting_launches() == 0
    r.close()


@gpu
def test_before(V, monkeypatch):
    r = Run(V, monkeypatch, DECK_OF["before"], "float", {"VPIC_HIP_SORT_IN_PUSH": 0})
    r.steps(9, 4)
    crossing(r)
    assert [s[0] for s in r.sorts()] == [k // 4 + 1 for k in range(9)] and r.sorts()[-1] == [3, 3]
    assert r.sorting_launches() == 0 and r.orders() == ["tile", "tile"]
    r.close()


@gpu
def test_measured(V, monkeypatch):
    """the knob unset: inside the push or before it by the engine's own measurement, 18 sort cycles -- right whichever way"""
    r = Run(V, monkeypatch, DECK_OF["measured"], "float")
    r.steps(37, 2)
    crossing(r)
    assert r.sorts()[-1] == [19, 19] and r.orders() == ["tile", "tile"]
    assert r.sorting_launches() >= 1                              # (inside the push at first: policy.h, sort_inside_push)
    r.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_tagged(V, monkeypatch, mode):
    """tags ride outside the push: the ordinary sort, no launch that sorts"""
    r = Run(V, monkeypatch, DECK_OF["tagged"], mode, {"VPIC_HIP_SORT_IN_PUSH": 1})
    r.steps(8, 3)
    crossing(r)
    assert scheduled(r, 3) and r.sorting_launches() == 0 and r.orders() == ["tile"]
    r.close()


@gpu
def test_every_step(V, monkeypatch):
    r = Run(V, monkeypatch, DECK_OF["every_step"], "float")
    r.steps(8, 1)
    assert [s[0] for s in r.sorts()] == list(range(1, 9)) and r.orders() == ["tile", "tile"]
    r.close()


@gpu
def test_never(V, monkeypatch):
    """interval 0 on an unsorted upload: the row instance on an array in no order"""
    r = Run(V, monkeypatch, DECK_OF["never"], "float")
    r.steps(8, 0)
    crossing(r)
    assert r.sorts()[-1] == [0, 0] and r.orders() == ["none", "none"] and r.sorting_launches() == 0
    r.close()


# ---- sorts the engine decides on -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES)
def test_early(V, monkeypatch, mode):
    """interval 40 outlasts the tiles' windows of a hot species (a 16 x 12 x 8 grid has 24 tiles: more than 32 x 24 runs of
    equal cells miss them in the first push after a sort): the engine sorts ahead of the interval (policy.h: early_sort),
    and the steps after that sort still pass; VPIC_HIP_EARLY_SORT=0 keeps it from doing so.  The deterministic instances
    publish no count of missed runs (missed_runs stays 0), so no deck makes the early sort fire there: the same run
    passes with the one scheduled sort."""
    r = Run(V, monkeypatch, DECK_OF["early"], mode)
    r.steps(12, 40)
    crossing(r)
    early = [f["species_stats"][0]["early_sorts"] for f in r.facts]
    if mode == "float":
        assert early[-1] >= 1 and early[-3] >= 1, early          # ... with steps after it
        assert all(f["species_stats"][0]["missed_runs"] > 32 * 24 for f in r.facts[:3])
    else:
        assert early[-1] == 0 and r.stats("missed_runs") == [0]
    assert scheduled(r, 40) and r.orders() == ["tile"]
    r.close()
    if mode == "float":
        r = Run(V, monkeypatch, DECK_OF["early"], mode, {"VPIC_HIP_EARLY_SORT": 0})
        r.steps(12, 40)
        assert r.stats("early_sorts") == [0] and r.sorts()[-1] == [1] and r.orders() == ["tile"]
        r.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_adaptive(V, monkeypatch, mode):
    r = Run(V, monkeypatch, DECK_OF["adaptive"], mode)
    r.steps(24, -20)
    crossing(r)
    assert r.sorts()[-1][0] >= 2 and r.orders() == ["tile"]
    r.close()


@gpu
@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_coarse(V, monkeypatch, mode, stage):
    r = Run(V, monkeypatch, DECK_OF["coarse"], mode, {"VPIC_HIP_TILE_COARSE": 1, "VPIC_HIP_STAGE": stage})
    r.steps(8, 3)
    crossing(r)
    assert r.stats("by_tile_only") == [1] and r.orders() == ["tile"] and scheduled(r, 3)
    r.close()


@gpu
@pytest.mark.parametrize("window", ["narrow", "wide"])
def test_rows(V, monkeypatch, window):
    r = Run(V, monkeypatch, DECK_OF["rows"], "float", {"VPIC_HIP_WINDOW": window})
    r.steps(8, 3)
    crossing(r)
    assert r.sorts()[-1] == [3] and r.sorting_launches() == 0 and sorted_by_voxel(r)
    r.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_thin(V, monkeypatch, mode):
    """12 x 1 x 12: thinner than a tile, the reference's order and the row instances with no knob set"""
    r = Run(V, monkeypatch, DECK_OF["thin"], mode)
    r.steps(8, 3)
    crossing(r)
    assert r.sorts()[-1] == [3] and r.sorting_launches() == 0 and sorted_by_voxel(r)
    r.close()


@gpu
@pytest.mark.parametrize("deck", WALL_DECKS)
@pytest.mark.parametrize("mode", MODES)
def test_walls(V, monkeypatch, mode, deck):
    """absorbing walls take particles step after step (the count falls as the oracle's does), the pushes after a back-fill
    still pass, and the sort after it restores the tile order"""
    r = Run(V, monkeypatch, deck, mode, {"VPIC_HIP_SORT_IN_PUSH": 1})
    n0 = r.e.np(r.sps[0])
    r.steps(9, 4)
    took = [sum(f["absorbed"]) for f in r.facts]
    assert sum(t > 0 for t in took) >= 3, took
    assert r.e.np(r.sps[0]) == n0 - sum(took)
    assert scheduled(r, 4) and r.orders() == ["tile"]           # (step 8 sorted)
    r.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_reflect(V, monkeypatch, mode):
    """reflecting walls on all six faces of the ragged grid: no particle leaves, every step passes"""
    r = Run(V, monkeypatch, DECK_OF["reflect"], mode, {"VPIC_HIP_SORT_IN_PUSH": 1})
    r.steps(9, 4)
    crossing(r)
    assert all(sum(f["absorbed"]) == 0 for f in r.facts) and scheduled(r, 4) and r.orders() == ["tile"]
    r.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_chargeless(V, monkeypatch, mode):
    """a charged species and its charge-0 copy: the copy's particles bit for bit the charged one's, the accumulator that of
    the charged one alone (the oracle's copy deposits zeros)"""
    r = Run(V, monkeypatch, DECK_OF["chargeless"], mode)
    r.steps(8, 3)
    crossing(r)
    assert scheduled(r, 3) and r.orders() == ["tile", "tile"] and r.stats("by_tile_only") == [0, 1]
    a, b = [D.by_tag(r.e.get_particles(sp)) for sp in r.sps]
    assert np.all(b["q"] == 0) and np.all(a["q"] != 0)
    for c in ("dx", "dy", "dz", "i", "ux", "uy", "uz"):
        assert np.array_equal(a[c].view(np.uint32), b[c].view(np.uint32)), c
    r.close()


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_clumped(V, monkeypatch, mode):
    """every particle in one tile: the push after the tile sort notices, falls back to the row instance, the next sort is
    by voxel, and every step passes (the deck of either mode: see the module's docstring)"""
    r = Run(V, monkeypatch, DECK_OF["clumped"][mode], mode)
    r.steps(5, 2)
    crossing(r)
    assert r.stats("too_clumped_for_tiles") == [1] and r.sorts()[-1] == [3] and sorted_by_voxel(r)
    r.close()


@gpu
@pytest.mark.parametrize("n_new,tail_sort_min", [(37, 10), (37, 100), (2000, 100), (2000, 1 << 20)])
@pytest.mark.parametrize("mode", MODES)
def test_arrivals(V, monkeypatch, mode, n_new, tail_sort_min):
    """particles appended between steps, with VPIC_HIP_TAIL_SORT_MIN at or below the tail's length (the engine regroups the
    tail by tile before its push) and above it (pushed as it is).  Which of the two happened is reported by no API and is
    NOT asserted: both settings are held to the same facts -- every step passes, and no sort happens inside the push while
    the array is longer than what was sorted: the sort of step 4 is the ordinary one, that of step 8 is inside the push
    again (float mode)"""
    r = Run(V, monkeypatch, DECK_OF["arrivals"], mode, {"VPIC_HIP_SORT_IN_PUSH": 1, "VPIC_HIP_TAIL_SORT_MIN": tail_sort_min}, room=2 * n_new)
    r.steps(2, 4)
    r.e.append_particles(r.sps[0], S.arrivals(r.dims, n_new, 60))
    r.steps(1, 4, first=2)
    r.e.append_particles(r.sps[1], S.arrivals(r.dims, n_new, 61))
    r.steps(2, 4, first=3)
    assert r.facts[-1]["np"] == [20 * 16 * 12 * 8 + n_new] * 2
    assert r.sorts()[-1] == [2, 2] and r.sorting_launches() == 0
    r.steps(4, 4, first=5)
    assert r.sorts()[-1] == [3, 3] and r.orders() == ["tile", "tile"]
    assert r.sorting_launches() == (2 if mode == "float" else 0)
    r.close()


@gpu
def test_back_to_tiles(V, monkeypatch):
    """deterministic mode: a tile-ordered species that a caller sorted by voxel between steps (the reference's order, as a
    hydro dump asks for) is put back into tile order before its push"""
    r = Run(V, monkeypatch, DECK_OF["back_to_tiles"], "deterministic")
    r.steps(3, 4)
    assert r.orders() == ["tile"] and r.sorts()[-1] == [1]
    r.e.set_sort_order("reference")
    r.e.sort_p(r.sps[0])
    r.e.set_sort_order("engine")
    assert r.orders() == ["voxel"]
    r.steps(1, 4, first=3)
    assert r.orders() == ["tile"] and r.sorts()[-1] == [3]      # (the caller's sort and the engine's own)
    r.steps(2, 4, first=4)
    r.close()


# ---- the host running ahead of the device ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES)
def test_no_read_between_steps(V, monkeypatch, mode):
    """12 steps at interval 4 with no read of any kind between them: the host waits only for the end of the step before the
    last one it enqueued.  Deterministic: fields and particles those of 12 free-running oracle steps bit for bit.  Float:
    the particle count, the fields within the bounds test_trajectory_20_steps holds a float run to, and -- on the untagged
    deck -- sorts that happened inside the push while the host ran ahead (sort_and_push decides "as last time" while the
    last measurement has not come back).  In both modes the accumulator step 11 left, put through the oracle's clear_jf,
    unload_accumulator and synchronize_jf, is the engine's own jfx, jfy, jfz with ==.  Then one more step, enqueued behind
    them, through SteppedRun: all three criteria, with the oracle started from the state the 12 steps left.  (Against the
    FREE-RUNNING oracle's exact sums of step 11 the float accumulator was off by 2.04e-6 and by 1.76e-6 of the largest sum
    in two runs: two float runs have drifted apart by then, the figure measures that drift and not the sums, and it is
    not asserted.)"""
    r = Run(V, monkeypatch, DECK_OF["no_read_between_steps"][mode], mode)
    dims, walls, args, kw, og, species = S.deck(DECK_OF["no_read_between_steps"][mode])
    for k in range(12):
        r.e.step(k, 4)
    f, fi, a = np.zeros(og.nv, L.field_t), np.zeros(og.nv, L.interpolator_t), np.zeros(og.nv + 1, L.accumulator_t)
    m = pyorc.vacuum_coefficients()
    ref = [dict(p=np.concatenate([sp["p"], np.zeros(1, L.particle_t)]), np=len(sp["p"]), q_m=sp["q_m"],
                pm=np.zeros(len(sp["p"]) + 1, L.particle_mover_t)) for sp in species]
    for k in range(12):
        pyorc.step(f, fi, a, m, ref, og, det_scale=SCALE if mode == "deterministic" else None)
    got = r.e.get_fields()
    jf = got.copy()                                               # step 11's accumulator -> jf, by the oracle
    acc = np.zeros(og.nv + 1, L.accumulator_t)
    acc[:og.nv] = r.e.get_accumulator()
    assert max(np.abs(acc[c]).max() for c in ("jx", "jy", "jz")) > 0
    pyorc.clear_jf(jf, og)
    pyorc.unload_accumulator(jf, acc, og)
    pyorc.synchronize_jf_local(jf, og)
    for c in ("jfx", "jfy", "jfz"):
        assert np.array_equal(got[c], jf[c]), "%s differs in %d voxels from the unloaded accumulator" % (c, (got[c] != jf[c]).sum())
    assert np.abs(f["ex"]).max() > 0 and np.abs(f["cbz"]).max() > 0
    assert [r.e.np(sp) for sp in r.sps] == [s["np"] for s in ref]
    assert r.orders() == ["tile", "tile"] and r.stats("sorts") == [3, 3]
    if mode == "deterministic":
        for c in S.FIELD_WORDS:
            assert np.array_equal(got[c], f[c]), "%s differs in %d voxels" % (c, (got[c] != f[c]).sum())
        for sp, s in zip(r.sps, ref):
            g, w = D.by_tag(r.e.get_particles(sp)), D.by_tag(s["p"][:s["np"]])
            assert np.array_equal(S.words(g), S.words(w)) and np.array_equal(g["tag"], w["tag"])
    else:
        assert r.sorting_launches() >= 2
        for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
            assert np.abs(got[c] - f[c]).max() <= 2e-4 * max(np.abs(f[c]).max(), np.abs(f["ex"]).max()), c
    r.steps(1, 4, first=12)
    assert r.stats("sorts") == [4, 4]
    r.close()
