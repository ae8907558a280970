"""The harness of tests/step_ref.py checked on the CPU before tests/test_gpu_step.py relies on it.

  - A correct stand-in for the engine -- pyorc.step with float sums, every species' array reordered between steps by a
    random permutation or by pyorc.sort_p -- passes 6 steps of every deck of the matrix: the harness accepts any array
    order and the oracle's own rounding.
  - Eight planted faults fail, each at the criterion it belongs to and with the step in the message.
  - ACC_TOL is a condition on the decks, not a measurement: on the first step of every deck the oracle's own float
    accumulator, pushed in array order and in a seeded random permutation, stays within ACC_TOL / 2 of the exact sums.
    Largest ratio seen: 0.24 of ACC_TOL (4.82e-7, deck "beams", array order, first step); the test prints them all.  The
    equal-charge clumped deck is no float deck: more than 65536 particles in one tile (what makes the engine leave the
    tile order) are a thousand per cell, and the oracle's own float sums of so many terms are 1.2e-6 to 1.8e-6 from the
    exact ones (six seeds, 66000 and 80000 particles, cold, hot, drifting).  It runs in deterministic mode, here too,
    where the accumulator is compared exactly; its float deck is "clumped_spread" (step_ref._clumped_spread says what the
    spread of charge costs), 0.22 of ACC_TOL on its first step."""
import contextlib

import numpy as np
import pytest

import step_ref as S
from step_ref import L, pyorc

FAULT_STEP = 3


class StandIn:
    """What SteppedRun needs of an Engine, over pyorc.step.  fault: (name, step) plants one fault into the state the
    step leaves behind."""

    def __init__(self, og, species, fault=None, seed=9, det_scale=None):
        self.og, self.fault, self.rng, self.det_scale = og, fault, np.random.default_rng(seed), det_scale
        self.m = pyorc.vacuum_coefficients()
        self.f, self.fi = np.zeros(og.nv, L.field_t), np.zeros(og.nv, L.interpolator_t)
        self.a = np.zeros(og.nv + 1, L.accumulator_t)
        self.species = []
        for sp in species:
            n = len(sp["p"])
            p = np.zeros(n + 1, L.particle_t)
            p[:n] = sp["p"]
            self.species.append(dict(p=p, np=n, q_m=sp["q_m"], pm=np.zeros(n + 1, L.particle_mover_t),
                                     partition=np.zeros(og.nv + 1, np.int32)))

    def get_fields(self):
        return self.f.copy()

    def get_interpolator(self):
        return self.fi.copy()

    def get_accumulator(self):
        return self.a[:self.og.nv].copy()

    def get_particles(self, sp):
        s = self.species[sp]
        return s["p"][:s["np"]].copy()

    def species_stats(self, sp):
        return {}

    def step(self, k, interval):
        for s in self.species:                                    # another array order before every step
            if k % 3 == 1:
                pyorc.sort_p(s["p"], s["np"], s["partition"], self.og)
            else:
                s["p"][:s["np"]] = s["p"][:s["np"]][self.rng.permutation(s["np"])]
        name, at = self.fault if self.fault and self.fault[1] == k else (None, None)
        before = [s["p"][:s["np"]].copy() for s in self.species]
        fi_before, a_before = self.fi.copy(), self.a.copy()
        with self._no_clear() if name == "accumulator_not_cleared" else contextlib.nullcontext():
            pyorc.step(self.f, self.fi, self.a, self.m, self.species, self.og, det_scale=self.det_scale)
        if name is None:
            return
        p = self.species[0]["p"]
        n = self.species[0]["np"]
        if name == "ux_one_ulp":
            p["ux"][n // 2] = np.nextafter(p["ux"][n // 2], np.float32(np.inf))
        elif name == "one_missing_one_twice":
            assert not np.array_equal(S.words(p[5:6]), S.words(p[6:7]))
            p[5] = p[6]
        elif name == "left_in_old_cell":
            assert n == len(before[0])                            # (nothing absorbed: slot j is still the same particle)
            step_x = p["i"][:n].astype(np.int64) - before[0]["i"]
            j = int(np.flatnonzero(np.abs(step_x) == 1)[0])       # crossed one x face, no wrap
            p["dx"][j] = p["dx"][j] + np.float32(2 * step_x[j])  # the offset as it was before the move to the next cell
            p["i"][j] = before[0]["i"][j]
        elif name == "accumulator_word_off":
            top = max(np.abs(self.a[c]).max() for c in ("jx", "jy", "jz"))
            v = int(np.argmax(np.abs(self.a["jy"][:, 2])))
            self.a["jy"][v, 2] += np.float32(4e-6 * top)
        elif name == "accumulator_not_cleared":
            assert np.abs(a_before["jx"]).max() > 0
        elif name == "ex_one_ulp":
            v = int(np.flatnonzero(self._interior())[7])
            self.f["ex"][v] = np.nextafter(self.f["ex"][v], np.float32(np.inf))
        elif name == "ghost_jfx":
            v = int(np.flatnonzero(~self._interior())[-3])
            self.f["jfx"][v] += np.float32(1e-3)
        elif name == "interpolator_stale":
            assert not np.array_equal(self.fi["ex"], fi_before["ex"])
            self.fi[:] = fi_before
        else:
            raise KeyError(name)

    def _interior(self):
        g = self.og
        z, y, x = np.meshgrid(np.arange(g.nz + 2), np.arange(g.ny + 2), np.arange(g.nx + 2), indexing="ij")
        return ((x >= 1) & (x <= g.nx) & (y >= 1) & (y <= g.ny) & (z >= 1) & (z <= g.nz)).ravel()

    @contextlib.contextmanager
    def _no_clear(self):
        keep = pyorc.clear_accumulators
        pyorc.clear_accumulators = lambda *args, **kw: None
        try:
            yield
        finally:
            pyorc.clear_accumulators = keep


def run(name, fault=None):
    dims, walls, args, kw, og, species = S.deck(name)
    det_scale = None if name in S.FLOAT_DECKS else pyorc.fixed_scale(S.Q0)     # (the stand-in with exact sums, as the engine)
    e = StandIn(og, species, fault, det_scale=det_scale)
    meta = [dict(sp=k, q_m=sp["q_m"], tagged=sp["tagged"]) for k, sp in enumerate(species)]
    return S.SteppedRun(e, og, e.m, meta, det_scale)


@pytest.mark.parametrize("name", list(S.DECKS))
def test_a_correct_stand_in_passes_every_deck(orc, name):
    r = run(name)
    facts = [r.advance(k, 0) for k in range(6)]
    assert all(sum(f["crossed"]) > 0 for f in facts)
    assert all(f["acc_ratio"] <= S.ACC_TOL for f in facts) and (name in S.FLOAT_DECKS or all(f["acc_ratio"] == 0 for f in facts))
    if "walls" in name:
        assert sum(sum(f["absorbed"]) > 0 for f in facts) >= 3
    else:
        assert all(sum(f["absorbed"]) == 0 for f in facts)


FAULTS = [("ux_one_ulp", 1), ("one_missing_one_twice", 1), ("left_in_old_cell", 1), ("accumulator_word_off", 2),
          ("accumulator_not_cleared", 2), ("ex_one_ulp", 3), ("ghost_jfx", 3), ("interpolator_stale", 3)]


@pytest.mark.parametrize("deck", ["hot_tagged", "beams"])
@pytest.mark.parametrize("fault,criterion", FAULTS)
def test_a_planted_fault_fails_at_its_criterion(orc, fault, criterion, deck):
    """... on a tagged deck and on a tag-less one (criterion 1 compares them in different ways)"""
    r = run(deck, (fault, FAULT_STEP))
    for k in range(FAULT_STEP):
        r.advance(k, 0)
    with pytest.raises(S.StepMismatch) as err:
        r.advance(FAULT_STEP, 0)
    assert err.value.criterion == criterion and err.value.step == FAULT_STEP, str(err.value)
    assert ("step %d, criterion %d" % (FAULT_STEP, criterion)) in str(err.value)
    print(err.value)


HEADROOM = {}


@pytest.mark.parametrize("name", S.FLOAT_DECKS)
def test_the_float_bound_leaves_the_engine_half_of_it(orc, name):
    """the oracle's own float accumulator on the deck's first step (zero fields) and on its second (the first with
    fields), in array order and permuted: within ACC_TOL / 2 of the exact sums"""
    dims, walls, args, kw, og, species = S.deck(name)
    e = StandIn(og, species)
    scale = pyorc.fixed_scale(max(float(np.abs(s["p"]["q"]).max()) for s in species))
    rng = np.random.default_rng(77)
    for order in ("array", "permuted", "array, step 1", "permuted, step 1"):
        if order == "array, step 1":
            e.step(0, 0)
        fi = e.get_interpolator()
        a = np.zeros(og.nv + 1, L.accumulator_t)
        with pyorc.fixed_accumulator(og, scale) as (a64, _):
            for k in range(len(species)):
                p = e.get_particles(k)
                if order.startswith("permuted"):
                    p = p[rng.permutation(len(p))]
                pyorc.advance_p(p, len(p), species[k]["q_m"], np.zeros(len(p) + 1, L.particle_mover_t), a, fi, og)
        ratio = S.acc_ratio(a, a64, scale)
        HEADROOM[(name, order)] = ratio
        print("headroom %-16s %-8s %.3g (%.2f of ACC_TOL)" % (name, order, ratio, ratio / S.ACC_TOL))
        assert ratio <= S.ACC_TOL / 2, (name, order, ratio)
