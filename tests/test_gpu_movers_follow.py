"""Pending movers and the calls that could reorder the array under them.

A mover names its particle by array index.  THE INVARIANT (include/vpic_hip.h at vpic_hip_sort_p): after any call of the
library, either every pending mover of a species names the same particle (by tag) with the same displacement words as
before the call, or the call failed with an error that says why and left the species, its bookkeeping and its movers byte
for byte as they were.

Two fixtures, one fresh engine per call.  "shuffled": an 8x8x8 grid with absorbing x walls, 4096 tagged particles uploaded
in random voxel order (not in tile order), 64 movers planted with set_movers on chosen live indices.  "holes": the
"tile_tail_holes" state of species_states.py (tile order, appended particles, dead slots) with 64 movers planted the same
way, so dead slots and movers exist together.  Every planted mover names a live, in-range particle.

The calls: sort_p in either sort order; exchange_begin under deterministic accumulation -- the second one of a step, in a
recovery round, which must succeed and must not reorder the species -- and under float accumulation as the control;
get_particles of a species with dead slots (it would have to compact); accumulate_hydro_p and accumulate_rho_p in both
accumulation modes; reserve; the calls that only read or only touch momenta (center_p, energy_p, select, distribution,
energy_spectrum, cool dry), which must leave the array order alone as well; collide and load_profile, which must refuse."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import small_calls_ref as R  # noqa: E402
import species_states  # noqa: E402
from species_states import N_DOOMED, N_TAIL, package  # noqa: E402
from test_gpu_cool import bookkeeping, snapshot  # noqa: E402

pytestmark = pytest.mark.gpu
GRID = (8, 8, 8)
N, N_MOVERS = 4096, 64


def plant(V, e, sp, seed):
    """N_MOVERS movers on live array indices chosen at random, every displacement word different; returns them sorted by index"""
    p, idx = snapshot(e, sp)
    rng = np.random.default_rng(seed)
    pm = np.zeros(N_MOVERS, V.layout.particle_mover_t)
    pm["i"] = np.sort(rng.choice(idx, N_MOVERS, replace=False))
    for k, c in enumerate(("dispx", "dispy", "dispz")):
        pm[c] = (0.001 * (1 + np.arange(N_MOVERS)) + 0.1 * k).astype(np.float32)
    e.set_movers(sp, pm)
    assert e.nm(sp) == N_MOVERS
    return pm


def shuffled(V):
    L = V.layout
    nx, ny, nz = GRID
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.2),
                             pbc=[L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0]))
    e.set_vacuum()
    e.load_interpolator()
    sp = e.new_species(-1.0, 2 * N, 4 * N_MOVERS)
    p = R.particles(90, N, GRID)
    p["q"] = np.where(p["q"] == 0, np.float32(0.01), p["q"])
    e.set_particles(sp, p)
    assert e.species_order(sp) == "none"
    plant(V, e, sp, 91)
    return e, sp


def holes(V):
    p = R.particles(92, N, GRID, spread=0.5)
    tail = R.particles(93, N_TAIL, GRID, spread=0.5, tag0=2 * 10 ** 7)
    e, sp = species_states.build_state(V, "tile_tail_holes", p, GRID, tail, dt=0.2, doomed_dx=0.99)
    assert e.nm(sp) == 0 and e.species_order(sp) == "tile" and e.species_stats(sp)["dead_slots"] == N_DOOMED
    plant(V, e, sp, 94)
    return e, sp


def named(e, sp):
    """what the pending movers name: (tags of their particles, ascending; the displacement words in that order, as bytes)"""
    p, idx = snapshot(e, sp)
    pm = e.get_movers(sp)
    rows = np.searchsorted(idx, pm["i"])
    assert (rows < len(idx)).all() and np.array_equal(idx[rows], pm["i"]), "a mover names a dead or out-of-range slot"
    tags = p["tag"][rows]
    order = np.argsort(tags, kind="stable")
    disp = np.stack([pm["dispx"], pm["dispy"], pm["dispz"]], axis=1)[order]
    return tags[order].tolist(), disp.tobytes()


def everything(e, sp):
    p, idx = snapshot(e, sp)
    return p.tobytes(), idx.tobytes(), bookkeeping(e, sp), e.get_movers(sp).tobytes(), e.nm(sp)


def array_order(e, sp):
    p, idx = snapshot(e, sp)
    return p["tag"].tobytes(), idx.tobytes()


# name: (what it does, may it fail?, must it leave the array order alone when it succeeds?)
def _sort(order):
    def call(V, e, sp):
        e.set_sort_order(order)
        e.sort_p(sp)
    return call


def _exchange_begin(mode):
    def call(V, e, sp):
        e.set_sort_order("engine")
        e.set_accumulation(mode, 0.1)
        e.exchange_begin()
    return call


def _hydro(mode):
    def call(V, e, sp):
        e.set_accumulation(mode, 0.1)
        e.clear_hydro()
        e.accumulate_hydro_p(sp)
    return call


def _rho(mode):
    def call(V, e, sp):
        e.set_accumulation(mode, 0.1)
        e.clear_rhof()
        e.accumulate_rho_p(sp)
    return call


def _reserve(V, e, sp):
    _, max_np, max_nm = e.capacity(sp)
    e.reserve(sp, max_np + 1000, max_nm + 100)
    assert e.capacity(sp)[1:] == (max_np + 1000, max_nm + 100)


SUCCEED, MAY_REFUSE, MUST_REFUSE = "succeeds", "may refuse", "refuses"
CALLS = {
    "sort_p_reference": (_sort("reference"), MAY_REFUSE, False),
    "sort_p_engine": (_sort("engine"), MAY_REFUSE, False),
    "exchange_begin_deterministic": (_exchange_begin("deterministic"), SUCCEED, True),
    "exchange_begin_float": (_exchange_begin("float"), SUCCEED, True),
    "get_particles": (lambda V, e, sp: e.get_particles(sp), MAY_REFUSE, False),
    "accumulate_hydro_p_float": (_hydro("float"), SUCCEED, True),
    "accumulate_hydro_p_deterministic": (_hydro("deterministic"), SUCCEED, True),
    "accumulate_rho_p_float": (_rho("float"), SUCCEED, True),
    "accumulate_rho_p_deterministic": (_rho("deterministic"), SUCCEED, True),
    "reserve": (_reserve, SUCCEED, True),
    "center_p": (lambda V, e, sp: e.center_p(sp), SUCCEED, True),
    "energy_p": (lambda V, e, sp: e.energy_p(sp), SUCCEED, True),
    "select": (lambda V, e, sp: e.select(sp, select=[("ke", 0.0, 1.0)], index=True), SUCCEED, True),
    "distribution": (lambda V, e, sp: e.distribution(sp, [("ux", -1.0, 0.125, 16)]), SUCCEED, True),
    "energy_spectrum": (lambda V, e, sp: e.energy_spectrum(sp, n_log=16, log_lo=-6.0, d_log=0.5), SUCCEED, True),
    "cool_dry": (lambda V, e, sp: e.cool(sp, 1e-2, 1e-3, 2.0 ** -33, dry=True), SUCCEED, True),
    "collide": (lambda V, e, sp: e.collide(sp, m_a=1.0, wq_a=100.0, cvar=1e-4, dt=0.3, seed=5, call=1), MUST_REFUSE, False),
    "load_profile": (lambda V, e, sp: e.load_profile(sp, 1, -0.01, seed=1), MUST_REFUSE, False),
}


def check(fixture, name):
    V = package()
    call, outcome, keeps_order = CALLS[name]
    e, sp = fixture(V)
    before, state, order = named(e, sp), everything(e, sp), array_order(e, sp)
    assert len(set(before[0])) == N_MOVERS
    try:
        call(V, e, sp)
        failed = None
    except V.VpicHipError as err:
        failed = str(err)
    print(fixture.__name__, name, "refused: " + failed if failed else "succeeded")
    if failed is None:
        assert outcome != MUST_REFUSE, name
        assert e.nm(sp) == N_MOVERS, name
        assert named(e, sp) == before, name                       # every mover: the same particle, the same displacement words
        if keeps_order:
            assert array_order(e, sp) == order, name
    else:
        assert outcome != SUCCEED, (name, failed)
        assert "mover" in failed, failed                          # the error says why
        assert everything(e, sp) == state, name                   # and nothing was touched
    e.close()


@pytest.mark.parametrize("name", list(CALLS))
def test_shuffled_species(name):
    check(shuffled, name)


@pytest.mark.parametrize("name", ["sort_p_engine", "exchange_begin_deterministic", "get_particles", "accumulate_hydro_p_deterministic",
                                  "accumulate_rho_p_float", "reserve", "center_p", "energy_p", "select", "collide"])
def test_species_with_dead_slots(name):
    check(holes, name)
    if name == "get_particles":                                   # (the case is what it says: the species would have to be compacted)
        assert N_DOOMED > 0


def test_without_movers_the_same_calls_reorder():
    """the control: with no mover pending, sort_p sorts, the deterministic exchange_begin puts the species into tile order and
    get_particles compacts -- the refusals above are about the movers and nothing else"""
    V = package()
    e, sp = shuffled(V)
    e.set_movers(sp, np.zeros(0, V.layout.particle_mover_t))
    assert e.nm(sp) == 0
    e.sort_p(sp)
    assert e.species_order(sp) == "voxel"
    e.set_sort_order("engine")
    e.set_accumulation("deterministic", 0.1)
    e.exchange_begin()
    assert e.species_order(sp) == "tile"
    e.close()
    e, sp = holes(V)
    e.set_movers(sp, np.zeros(0, V.layout.particle_mover_t))
    p = e.get_particles(sp)
    assert len(p) == N + N_TAIL and e.species_stats(sp)["dead_slots"] == 0
    e.close()
