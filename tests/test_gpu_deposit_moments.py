"""The float push instances sum deposit MOMENTS and form the terms where a value leaves for the global accumulator
(push_device.h: streak12_moments, term_of, moments_to_terms; push.hip: the flush and deposit_run).  One case per
path that applies the map, on an 8 x 8 x 8 grid -- two tiles per axis, so every tile window's halo wraps around the box -- at
16 particles per cell: after every one of a few pushes the accumulator is the oracle's within ACC_TOL of its largest entry
and every particle is the oracle's bit for bit (the deposits feed no particle state).  Each case prints its worst accumulator
error as a share of the bound; profiles/deposit_moments_error.txt keeps those of this build and of its parent, which summed
the terms themselves, and the last test holds the worst of them to twice the parent's.  GPU box only."""
import importlib

import numpy as np
import pytest

from conftest import bits_equal
from sort_ref import _records
from test_gpu_tiles import ACC_TOL, random_interpolator

pytestmark = pytest.mark.gpu

N, PPC = 8, 16
DT = np.float32(0.5)
SHARES = {}                         # case -> worst accumulator error over its pushes, as a share of ACC_TOL x largest entry
# The same figure from the parent build (terms summed, no map), this file run against it: profiles/deposit_moments_error.txt
PARENT_WORST_SHARE = 0.147
FAST_ULP = 8                        # FAST arithmetic: momenta within 8 ulp of the scalar pipeline's (tests/test_gpu_kernels.py)


@pytest.fixture(scope="module")
def V():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


@pytest.fixture(scope="module")
def deck(V, orc, L):
    """grids (periodic, reflecting z) and one interpolator, shared by every case"""
    rng = np.random.default_rng(101)
    refl = dict(pbc=[0, 0, L.REFLECT_PARTICLES, 0, 0, L.REFLECT_PARTICLES])
    d = dict(g=V.make_grid(N, N, N, float(N), float(N), float(N), DT), og=orc.make_grid(N, N, N, float(N), float(N), float(N), DT),
             g_refl=V.make_grid(N, N, N, float(N), float(N), float(N), DT, **refl), og_refl=orc.make_grid(N, N, N, float(N), float(N), float(N), DT, **refl))
    d["fi"] = random_interpolator(orc, L, d["og"], rng, amp=0.02)
    return d


def particles(L, seed, vth, drift=0.0, q=-1.0 / PPC):
    """PPC particles in every cell, thermal spread vth per component, drift along x; charges vary by +-50 %"""
    rng = np.random.default_rng(seed)
    n = N * N * N * PPC
    p = np.zeros(n, L.particle_t)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-1, 1, n).astype(np.float32)
    cell = np.repeat(np.arange(N * N * N), PPC)
    p["i"] = L.voxel(cell % N + 1, cell // N % N + 1, cell // (N * N) + 1, N, N, N)
    for c in ("ux", "uy", "uz"):
        p[c] = (rng.standard_normal(n) * vth).astype(np.float32)
    p["ux"] += np.float32(drift)
    p["q"] = (q * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    p["tag"] = np.arange(n) + 1
    return p


def share_of_bound(acc, ref_a):
    a = np.stack([acc["jx"], acc["jy"], acc["jz"]]).astype(np.float64)
    r = np.stack([ref_a["jx"], ref_a["jy"], ref_a["jz"]]).astype(np.float64)
    top = np.abs(r).max()
    assert top > 0
    return np.abs(a - r).max() / (ACC_TOL * top)


def by_tag(a):
    return a[np.argsort(a["tag"], kind="stable")]


def pushes(name, e, sp, orc, L, og, fi, steps, launch=None, same=None):
    """`steps` pushes of the engine's species, each against the oracle's push of the array as the engine held it before: the
    accumulator within ACC_TOL after every push, the particles the oracle's.  launch(step): the engine's push of that step
    (default: advance_p); same(got, ref): the particle comparison (default: bit for bit in place)."""
    worst = 0.0
    for step in range(steps):
        ref = e.get_particles(sp)
        ref_a = np.zeros(og.nv, L.accumulator_t)
        pm = np.zeros(len(ref), L.particle_mover_t)
        assert orc.advance_p(ref, len(ref), -1.0, pm, ref_a, fi, og) == 0
        e.clear_accumulators()
        assert (launch(step) if launch else e.advance_p(sp)) == 0
        got = e.get_particles(sp)
        assert (same or bits_equal)(got, ref), (name, step)
        s = share_of_bound(e.get_accumulator(), ref_a)
        print("%s, push %d: worst accumulator error %.3f of the bound" % (name, step + 1, s))
        worst = max(worst, s)
    SHARES[name] = max(SHARES.get(name, 0.0), worst)
    assert worst <= 1.0, name
    return worst


def tile_engine(V, monkeypatch, g, fi, p, coarse=False, extra_capacity=64):
    monkeypatch.setenv("VPIC_HIP_WINDOW", "tile")
    monkeypatch.setenv("VPIC_HIP_TILE_COARSE", "1" if coarse else "0")
    e = V.Engine(g)
    e.set_interpolator(fi)
    sp = e.new_species(-1.0, len(p) + extra_capacity, 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    return e, sp


def test_plain_tile_launch(V, orc, L, deck, monkeypatch):
    """Window<2>: runs of equal cells scanned, the window flushed through the map; a warm beam, a tenth of it crossing per step"""
    e, sp = tile_engine(V, monkeypatch, deck["g"], deck["fi"], particles(L, 1, 0.05, drift=0.2))
    pushes("tile", e, sp, orc, L, deck["og"], deck["fi"], 4)
    e.close()


def test_hist_and_sort_launches(V, orc, L, deck, monkeypatch):
    """Sort interval 2 over four steps: a plain push, one that counts for the sort (HIST), one that sorts as it pushes (SORT), one
    that counts again -- and the sorting launch that closes the second interval.  The SORT launch writes the species in its new
    order: the same particle records, whatever their places."""
    monkeypatch.setenv("VPIC_HIP_SORT_IN_PUSH", "1")
    p = particles(L, 2, 0.05, drift=0.2)
    p["tag"] = 0                                            # (tags ride outside the push: a tagged species sorts the ordinary way)
    e = V.Engine(deck["g"])
    e.set_sort_order("engine")
    e.set_interpolator(deck["fi"])
    sp = e.new_species(-1.0, 2 * len(p), 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    e.profile_enable(True)

    def launch(step):
        if step in (1, 3):
            V.lib().vpic_hip_species_sort_hint(e._h, sp)    # this push counts for the sort that follows
        return e.sort_advance_p(sp) if step in (2, 4) else e.advance_p(sp)

    pushes("hist+sort", e, sp, orc, L, deck["og"], deck["fi"], 5, launch, lambda got, ref: np.array_equal(_records(got), _records(ref)))
    assert e.profile_read_sorting()[1] == 2                 # both sorts happened inside their push (which needs the counts of the push before)
    e.close()


def test_species_sorted_by_tile_only(V, orc, L, deck, monkeypatch):
    """Window<3>, the unordered instance: every lane adds its own moments; hot, half the particles cross per step"""
    e, sp = tile_engine(V, monkeypatch, deck["g"], deck["fi"], particles(L, 3, 0.6), coarse=True)
    pushes("tile only", e, sp, orc, L, deck["og"], deck["fi"], 4)
    e.close()


@pytest.mark.parametrize("coarse", [False, True], ids=["by cell", "by tile only"])
@pytest.mark.parametrize("misses", ["few", "many"])
def test_runs_that_miss_the_window(V, orc, L, deck, monkeypatch, misses, coarse):
    """VPIC_HIP_FOLLOW=0: the windows stay on their tiles while a beam at 0.45 cells per step leaves them -- three cells off
    after seven steps, when the deposits of its leading half miss the window.  few: one particle in sixty is in the beam, the
    others rest: a pass has a miss or two, which are expanded, wait in the wavefront's list and leave through flush_misses.  many: every particle
    is in the beam, with a transverse spread that mixes the cells along the array: more than MISS_CAP = 5 runs of a pass miss,
    and their totals go to global memory on the spot, expanded in registers."""
    monkeypatch.setenv("VPIC_HIP_FOLLOW", "0")
    p = particles(L, 4, 0.3 if misses == "many" else 0.01, drift=2.0 if misses == "many" else 0.0)
    if misses == "few":
        p["ux"][::60] += np.float32(2.0)
    e, sp = tile_engine(V, monkeypatch, deck["g"], deck["fi"], p, coarse=coarse)
    name = "misses, %s, %s" % (misses, "by tile only" if coarse else "by cell")
    pushes(name, e, sp, orc, L, deck["og"], deck["fi"], 8)
    e.sync()
    missed, passes = e.species_stats(sp)["missed_runs"], len(p) // 64
    print("%s: %d runs of the last push missed their window (%d passes)" % (name, missed, passes))
    assert (0 < missed <= 5 * passes) if misses == "few" else (missed > 5 * passes)
    e.close()


def test_appended_particles_pushed_without_a_window(V, orc, L, deck, monkeypatch):
    """A handful of particles appended after the sort is pushed by workgroups of its own without a window (NO_WINDOW): every
    run total goes to global memory."""
    p = particles(L, 5, 0.3)
    extra = particles(L, 6, 0.3)[::97][:60]
    extra["tag"] += len(p)
    e, sp = tile_engine(V, monkeypatch, deck["g"], deck["fi"], p, extra_capacity=256)
    e.append_particles(sp, extra[:3])
    e.append_particles(sp, extra[3:])
    pushes("appended", e, sp, orc, L, deck["og"], deck["fi"], 4, same=lambda got, ref: bits_equal(by_tag(got), by_tag(ref)))
    e.close()


def test_a_cell_that_receives_only_charge_0_lanes(V, orc, L, deck, monkeypatch):
    """The particles of the cells with x = 3, 4, 5 carry no charge and hardly move: the cells with x = 4 receive zeros only.
    All their moments are zero, the terms formed from them are zero, and the flush skips them: those accumulators stay as they
    were cleared, as the oracle's do."""
    p = particles(L, 7, 0.01)
    x = (p["i"] % (N + 2))
    p["q"][(x >= 3) & (x <= 5)] = 0
    e, sp = tile_engine(V, monkeypatch, deck["g"], deck["fi"], p)
    pushes("charge 0", e, sp, orc, L, deck["og"], deck["fi"], 4)
    acc = e.get_accumulator()
    quiet = np.arange(deck["og"].nv) % (N + 2) == 4
    for c in ("jx", "jy", "jz"):
        assert np.all(acc[c][quiet].view(np.uint32) == 0), c
        assert np.any(acc[c][~quiet] != 0), c
    e.close()


def test_reflecting_z_walls(V, orc, L, deck, monkeypatch):
    """hot particles between reflecting z walls: segments that end on a wall and turn back, in the crossers' path"""
    e, sp = tile_engine(V, monkeypatch, deck["g_refl"], deck["fi"], particles(L, 8, 0.6))
    pushes("reflecting z", e, sp, orc, L, deck["og_refl"], deck["fi"], 4)
    e.close()


@pytest.mark.parametrize("window", ["narrow", "wide"])
def test_reference_order_row_windows(V, orc, L, deck, monkeypatch, window):
    """The reference's order by voxel: the float row window (Window<0>) and the double one (Window<1>) hold moments too, and
    their flush applies the map."""
    monkeypatch.setenv("VPIC_HIP_WINDOW", window)
    e = V.Engine(deck["g"])
    e.set_interpolator(deck["fi"])
    p = particles(L, 9, 0.3)
    sp = e.new_species(-1.0, len(p) + 64, 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == "voxel"
    pushes("row window, " + window, e, sp, orc, L, deck["og"], deck["fi"], 4)
    e.close()


def test_fast_arithmetic(V, orc, L, deck, monkeypatch):
    """FAST arithmetic (contracted multiply-adds, 1-ulp rsq / rcp): its particles are the scalar pipeline's to a few ulp, not bit
    for bit, so each push is compared with the oracle's push of the array as the engine held it: momenta within FAST_ULP, and the
    accumulator within the same ACC_TOL."""
    def same(got, ref):
        scale = np.maximum.reduce([np.abs(ref[c]) for c in ("ux", "uy", "uz")])
        return all(np.all(np.abs(got[c].astype(np.float64) - ref[c]) <= FAST_ULP * np.spacing(scale)) for c in ("ux", "uy", "uz"))

    p = particles(L, 10, 0.05, drift=0.2)
    monkeypatch.setenv("VPIC_HIP_WINDOW", "tile")
    monkeypatch.setenv("VPIC_HIP_TILE_COARSE", "0")
    e = V.Engine(deck["g"])
    e.set_push_mode("fast")
    e.set_interpolator(deck["fi"])
    sp = e.new_species(-1.0, len(p) + 64, 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    pushes("fast", e, sp, orc, L, deck["og"], deck["fi"], 4, same=same)
    e.close()


def test_worst_error_against_the_parent_s():
    """The record: every case's worst error as a share of the bound, and the worst of them against twice the parent's."""
    assert SHARES, "the cases above fill the record"
    for name, s in sorted(SHARES.items()):
        print("deposit moments: %-36s worst error %.3f of the bound" % (name, s))
    worst = max(SHARES.values())
    print("deposit moments: worst of all cases %.3f of the bound (parent: %.3f)" % (worst, PARENT_WORST_SHARE))
    assert worst <= 2 * PARENT_WORST_SHARE
