"""vpic_hip_species_cool on the GPU against THE RULE in numpy (tests/cool_ref.py): EXACT equality -- every word of the
new momenta as uint32, the species' sum, every per-voxel sum and the four statistics as integers -- on grids 5x3x4 and
9x6x5 (the second larger than a tile in every axis and a multiple of none), in every order a species' array can be in
(species_states.build_state: "unsorted", "voxel", "tile", "tile_only" in a fresh child process, "tile_tail_holes" with
appended particles and dead slots), through all the kernel's instances: applying, dry, and either with the per-voxel
sums.  Both sides round every operation once, so there is no tolerance to choose.

What the species holds is read with Engine.select (every live particle with its array index, dead slots counted, nothing
about the species changed: a download would drop the dead slots), before and after; everything but the momenta must be
byte for byte what it was, with the order, the partitions and the statistics of the species."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cool_ref as R  # noqa: E402
import species_states  # noqa: E402
from species_states import N_DOOMED, N_TAIL, STATES, package  # noqa: E402
from test_cool_ref import (GRIDS, HAND_ICS, HAND_QUANTUM, HAND_SYNC, IC, N_GPU, QUANTUM, SYNC, cool_interpolator,  # noqa: E402
                           cool_particles, guard_voxels, hand_interpolator, handmade_cool, n_voxels, plant_guards)
from test_distribution_ref import HAND_GRID  # noqa: E402
from test_gpu_load import environment  # noqa: E402
from test_spectrum_ref import voxel  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK, SPAN = 256, 1024 * 256          # csrc/cool.hip: COOL_THREADS, and COOL_MAX_BLOCKS * COOL_THREADS (the grid-stride span)
OTHER = [n for n in ("dx", "dy", "dz", "i", "q", "tag", "tag2")]


def engine_for(V, grid, dt=0.3):
    nx, ny, nz = grid
    return V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt)))


def build(V, state, grid, seed):
    """(engine, species) with N_GPU generated particles in the array state asked for; the fields are zero while the state
    is built, so the one push of "tile_tail_holes" moves positions only"""
    holes = state == "tile_tail_holes"
    p = cool_particles(seed, N_GPU, grid, spread=0.95 if holes else 1.0)
    tail = None
    if holes:
        tail = cool_particles(seed + 1, N_TAIL, grid, spread=0.95)
        tail["tag"] = np.arange(N_TAIL) + 2 * 10 ** 7
    # |v| < 1 and cells of size 1: 0.95 + 2 * 0.02 < 1, nobody but the doomed leaves a cell; they do: 0.99 + 2 * 0.95 * 0.02 > 1
    return species_states.build_state(V, state, p, grid, tail, dt=0.02 if holes else 0.4, doomed_dx=0.99)


def snapshot(e, sp):
    """(every live particle in array order, its array index) -- the species is not touched"""
    r = e.select(sp, index=True)
    assert r.count == e.np(sp) == len(r.particles)
    return r.particles, r.index


def bookkeeping(e, sp):
    order = e.species_order(sp)
    part = e.get_partition(sp).tobytes() if order == "voxel" else e.get_tile_partition(sp).tobytes() if order == "tile" else b""
    return e.species_stats(sp), order, e.np(sp), e.capacity(sp), part


def momenta(p):
    return np.stack([p["ux"], p["uy"], p["uz"]], axis=1).astype(np.float32).view(np.uint32)


def same_but_momenta(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in OTHER)


def check_result(r, ref, cells, what):
    assert r.isum == ref.isum, what
    assert r.energy == ref.isum * QUANTUM, what
    assert r.stats == ref.stats, (what, r.stats, ref.stats)
    if cells:
        assert r.cell_isums.dtype == np.int64 and np.array_equal(r.cell_isums, ref.cell_isums), what
    else:
        assert r.cell_isums is None, what


def check_state(state, g):
    V = package()
    grid = GRIDS[g]
    e, sp = build(V, state, grid, 20 + g)
    fi = cool_interpolator(30 + g, grid)
    e.set_interpolator(fi)
    holes = state == "tile_tail_holes"
    p0, idx0 = snapshot(e, sp)
    book = bookkeeping(e, sp)
    assert len(p0) == N_GPU + (N_TAIL if holes else 0) and book[0]["dead_slots"] == (N_DOOMED if holes else 0)
    ref = R.cool_ref(p0, fi, SYNC, IC, QUANTUM)
    assert ref.stats["seen"] == len(p0) and ref.stats["changed"] > 0.9 * len(p0) and (ref.addend < 0).any() and (ref.addend > 0).any()
    # dry, with and without the per-voxel sums: the tallies, and not a byte of the species
    for cells in (True, False):
        r = e.cool(sp, SYNC, IC, QUANTUM, dry=True, cells=cells)
        check_result(r, ref, cells, (state, "dry", cells))
        p1, idx1 = snapshot(e, sp)
        assert p1.tobytes() == p0.tobytes() and np.array_equal(idx1, idx0) and bookkeeping(e, sp) == book
    # applying
    r = e.cool(sp, SYNC, IC, QUANTUM)
    check_result(r, ref, False, (state, "apply"))
    p1, idx1 = snapshot(e, sp)
    assert np.array_equal(momenta(p1), ref.u.view(np.uint32)), state
    assert same_but_momenta(p1, p0) and np.array_equal(idx1, idx0) and bookkeeping(e, sp) == book
    # applying with the per-voxel sums, on what the first call left: the rule applied twice
    ref2 = R.cool_ref(R.apply_ref(p0, ref), fi, SYNC, IC, QUANTUM)
    r = e.cool(sp, SYNC, IC, QUANTUM, cells=True)
    check_result(r, ref2, True, (state, "apply, cells"))
    p2, idx2 = snapshot(e, sp)
    assert np.array_equal(momenta(p2), ref2.u.view(np.uint32)), state
    assert same_but_momenta(p2, p0) and np.array_equal(idx2, idx0) and bookkeeping(e, sp) == book
    print(f"{state} {grid}: {r.stats}, isum {ref.isum} then {ref2.isum}")
    e.close()


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("state", STATES)
def test_every_word_equals_the_rule(state, g):
    # a grid thinner than a tile on some axis (5x3x4) takes the tile order only when told to; the knobs are read when the
    # engine is created, and "tile_only" needs a fresh process for its own
    with environment(**(dict(VPIC_HIP_WINDOW="tile") if state.startswith("tile") else {})):
        if state == "tile_only":
            species_states.run_child(__file__, [state, g], timeout=300)
        else:
            check_state(state, g)


def test_dry_equals_the_applying_call_on_a_twin():
    V = package()
    grid = GRIDS[1]
    fi = cool_interpolator(31, grid)
    (a, sa), (b, sb) = build(V, "tile", grid, 21), build(V, "tile", grid, 21)
    a.set_interpolator(fi)
    b.set_interpolator(fi)
    before = a.get_particles(sa)
    dry = a.cool(sa, SYNC, IC, QUANTUM, dry=True, cells=True)
    wet = b.cool(sb, SYNC, IC, QUANTUM, cells=True)
    assert a.get_particles(sa).tobytes() == before.tobytes()               # downloads: bit-identical before and after
    ref = R.cool_ref(before[np.argsort(before["tag"])], fi, SYNC, IC, QUANTUM)
    cooled = b.get_particles(sb)
    assert np.array_equal(momenta(cooled[np.argsort(cooled["tag"])]), ref.u.view(np.uint32))
    assert wet.isum == ref.isum and wet.stats == ref.stats and np.array_equal(wet.cell_isums, ref.cell_isums)
    assert dry.isum == wet.isum and dry.stats == wet.stats and np.array_equal(dry.cell_isums, wet.cell_isums)
    assert dry.stats["changed"] >= 0.99 * N_GPU
    a.close()
    b.close()


def test_order_does_not_matter():
    V = package()
    grid = GRIDS[1]
    fi = cool_interpolator(31, grid)
    p = cool_particles(21, N_GPU, grid)
    shuffled = p[np.random.default_rng(9).permutation(len(p))]
    got = []
    for arr in (p, shuffled):
        e = engine_for(V, grid)
        e.set_interpolator(fi)
        sp = e.new_species(-1.0, len(arr), 8)
        e.set_particles(sp, arr)
        r = e.cool(sp, SYNC, IC, QUANTUM, cells=True)
        back = e.get_particles(sp)
        got.append((r, back[np.argsort(back["tag"])]))
        e.close()
    (ra, pa), (rb, pb) = got
    assert ra.isum == rb.isum and np.array_equal(ra.cell_isums, rb.cell_isums) and ra.stats == rb.stats
    assert pa.tobytes() == pb.tobytes()                                    # per tag: the same new momenta


def test_launch_shapes():
    """np = 0, 1, around a wavefront, around a workgroup, and around the span of one grid-stride pass"""
    V = package()
    grid = GRIDS[0]
    fi = cool_interpolator(30, grid)
    e = engine_for(V, grid)
    e.set_interpolator(fi)
    everything = cool_particles(40, SPAN + 1, grid)
    full = R.cool_ref(everything, fi, SYNC, IC, QUANTUM)                    # (computed once: a prefix's result is the prefix of it)
    sp = e.new_species(-1.0, SPAN + 1, 8)
    for n in (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, SPAN - 1, SPAN, SPAN + 1):
        p = everything[:n]
        if n:
            e.set_particles(sp, p)                              # (the species starts empty)
        cells = np.zeros(n_voxels(grid), np.int64)
        np.add.at(cells, p["i"], full.addend[:n])
        for dry in (True, False):
            r = e.cool(sp, SYNC, IC, QUANTUM, dry=dry, cells=True)
            assert r.isum == int(full.addend[:n].sum()), (n, dry)
            assert np.array_equal(r.cell_isums, cells), (n, dry)
            assert r.stats == dict(seen=n, changed=int(full.changed[:n].sum()), refused=0, left_alone=0), (n, dry)
        assert e.np(sp) == n
        back = e.get_particles(sp)
        assert np.array_equal(momenta(back), full.u[:n].view(np.uint32)), n
        assert same_but_momenta(back, p), n
    e.close()


def upload_any_voxel(V, e, sp, p):
    f = V.lib().vpic_hip_debug_set_particles_any_voxel          # (a test hook that no header declares: the arguments say their types)
    p = np.ascontiguousarray(p, V.layout.particle_t)
    if f(e._h, C.c_int(sp), p.ctypes.data_as(C.c_void_p), C.c_int64(len(p))):
        raise V.VpicHipError(V.lib().vpic_hip_last_error().decode())


@pytest.mark.parametrize("g", [0, 1])
def test_guards_planted(g):
    """a NaN word in one voxel's record, an inf word in another's: their particles are left alone and counted, everybody
    else is cooled; a tiny quantum refuses the tally and still writes the momenta; particles in ghost voxels use those
    voxels' records"""
    V = package()
    grid = GRIDS[g]
    nx, ny, nz = grid
    fi = plant_guards(cool_interpolator(30 + g, grid), grid)
    p = cool_particles(20 + g, N_GPU, grid)
    rng = np.random.default_rng(3)
    ghosts = cool_particles(50 + g, 200, grid)
    ghosts["i"] = voxel(rng.choice([0, nx + 1], 200), rng.integers(0, ny + 2, 200), rng.integers(0, nz + 2, 200), grid)
    ghosts["tag"] += 10 ** 6
    p = np.concatenate([p, ghosts])
    v_nan, v_inf = guard_voxels(grid)
    for quantum in (QUANTUM, 1e-300):
        ref = R.cool_ref(p, fi, SYNC, IC, quantum)
        in_guard = (p["i"] == v_nan) | (p["i"] == v_inf)
        assert ref.alone.tolist() == in_guard.tolist() and 0 < in_guard.sum() < 0.2 * len(p)
        assert (ref.stats["refused"] == 0) if quantum == QUANTUM else (ref.stats["refused"] >= 0.95 * (len(p) - in_guard.sum()))
        e = engine_for(V, grid)
        e.set_interpolator(fi)
        sp = e.new_species(-1.0, len(p), 8)
        upload_any_voxel(V, e, sp, p)
        dry = e.cool(sp, SYNC, IC, quantum, dry=True, cells=True)
        check_result_q(dry, ref, quantum)
        assert e.get_particles(sp).tobytes() == p.tobytes()
        r = e.cool(sp, SYNC, IC, quantum, cells=True)
        check_result_q(r, ref, quantum)
        back = e.get_particles(sp)
        assert np.array_equal(momenta(back), ref.u.view(np.uint32)) and same_but_momenta(back, p)
        assert momenta(back)[in_guard].tobytes() == momenta(p)[in_guard].tobytes()
        print(grid, quantum, r.stats)
        e.close()


def check_result_q(r, ref, quantum):
    assert r.isum == ref.isum and r.energy == ref.isum * quantum and r.stats == ref.stats, (r.stats, ref.stats)
    assert np.array_equal(r.cell_isums, ref.cell_isums)


def test_handmade_particles_take_every_branch_on_the_device():
    """the hand-made particles of test_cool_ref.py with their interpolator, alone and behind generated ones: plain, left
    alone through a NaN and through an inf, a ghost voxel, and chi clamped -- with ic = 0 the clamp decides three float
    words of that particle (test_cool_ref.test_the_clamp_decides_a_float_word), with ic = 0.01 it is refused for the
    tally and still written.  An upload takes no dead slot and no i >= nv (asserted): the dead slots of
    "tile_tail_holes" stand for the first, and no entry point of the library can put the second on the device."""
    V = package()
    hand = handmade_cool()
    fi = hand_interpolator()
    nv = n_voxels(HAND_GRID)
    uploadable = (hand["i"] >= 0) & (hand["i"] < nv)
    assert uploadable.tolist() == [True, True, True, False, True, True, False]
    filler = cool_particles(60, 150, HAND_GRID)
    filler["tag"] += 100
    for p in (hand[uploadable], np.concatenate([filler, hand[uploadable], filler[:70]])):
        for ic in HAND_ICS:
            for quantum in (HAND_QUANTUM, 1e-300):
                ref = R.cool_ref(p, fi, HAND_SYNC, ic, quantum)
                clamped = np.flatnonzero(p["tag"] == 6)[0]
                assert ref.stats["left_alone"] >= 2 and not ref.alone[clamped]
                assert ref.refused[clamped] == (ic != 0.0)
                e = engine_for(V, HAND_GRID)
                e.set_interpolator(fi)
                sp = e.new_species(-1.0, len(p), 8)
                for bad in (3, 6):
                    with pytest.raises(V.VpicHipError):
                        upload_any_voxel(V, e, sp, hand[bad:bad + 1])
                upload_any_voxel(V, e, sp, p)
                check_result_q(e.cool(sp, HAND_SYNC, ic, quantum, dry=True, cells=True), ref, quantum)
                r = e.cool(sp, HAND_SYNC, ic, quantum, dry=True)
                assert r.isum == ref.isum and r.stats == ref.stats and r.cell_isums is None
                assert e.get_particles(sp).tobytes() == p.tobytes()
                check_result_q(e.cool(sp, HAND_SYNC, ic, quantum, cells=True), ref, quantum)
                back = e.get_particles(sp)
                assert np.array_equal(momenta(back), ref.u.view(np.uint32)) and same_but_momenta(back, p), (ic, quantum)
                upload_any_voxel(V, e, sp, p)
                r = e.cool(sp, HAND_SYNC, ic, quantum)                    # ... and the applying instance without the per-voxel sums
                assert r.isum == ref.isum and r.stats == ref.stats
                assert np.array_equal(momenta(e.get_particles(sp)), ref.u.view(np.uint32)), (ic, quantum)
                print(len(p), ic, quantum, ref.stats, ref.isum)
                e.close()


def test_bookkeeping_survives_collide():
    """sort_p, cool, then collide within the species: the exact ranges of the sort still hold (sorted_first == 0)"""
    V = package()
    grid = GRIDS[1]
    for order in ("voxel", "tile"):
        e = engine_for(V, grid)
        e.set_interpolator(cool_interpolator(31, grid))
        sp = e.new_species(-1.0, N_GPU, 8)
        e.set_particles(sp, cool_particles(21, N_GPU, grid))
        if order == "tile":
            e.set_sort_order("engine")
        e.sort_p(sp)
        assert e.species_order(sp) == order
        assert e.cool(sp, SYNC, IC, QUANTUM).stats["changed"] >= 0.99 * N_GPU
        e.collide(sp, m_a=1.0, wq_a=100.0, cvar=1e-4, dt=0.3, seed=5, call=1, relativistic=True)
        st = e.collide_stats()
        assert st["sorted_first"] == 0 and st["pairs"] > 0, st
        e.close()


def records(p):
    """the 48-byte records of p as a sorted list: a multiset"""
    return sorted(p[k].tobytes() for k in range(len(p)))


@pytest.mark.parametrize("order", ["voxel", "tile"])
def test_bookkeeping_survives_the_push(order):
    """sort_p, cool, advance_p against a twin that received the reference's cooled particles by set_particles and then ran
    sort_p, advance_p: equal as a multiset of 48-byte records (a sort pending inside the push included: order "tile")"""
    V = package()
    grid = GRIDS[1]
    fi = cool_interpolator(31, grid)
    p = cool_particles(21, N_GPU, grid)
    ref = R.cool_ref(p, fi, SYNC, IC, QUANTUM)
    out = []
    for twin in (False, True):
        e = engine_for(V, grid, dt=0.3)
        e.set_vacuum()
        e.set_interpolator(fi)
        sp = e.new_species(-1.0, N_GPU + 4096, 8192)
        e.set_particles(sp, R.apply_ref(p, ref) if twin else p)
        if order == "tile":
            e.set_sort_order("engine")
        e.sort_p(sp)
        if not twin:
            r = e.cool(sp, SYNC, IC, QUANTUM)
            assert r.isum == ref.isum and r.stats == ref.stats
        e.clear_accumulators()
        e.advance_p(sp)
        assert e.np(sp) == N_GPU and e.nm(sp) == 0
        out.append(e.get_particles(sp))
        e.close()
    assert records(out[0]) == records(out[1])
    assert records(out[0]) != records(p)


def test_argument_errors():
    """every bad argument is refused: non-zero, the argument named, and the species, the last statistics and the caller's
    arrays untouched"""
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    grid = GRIDS[0]
    e = engine_for(V, grid)
    e.set_interpolator(cool_interpolator(30, grid))
    p = cool_particles(20, 500, grid)
    sp = e.new_species(-1.0, len(p), 8)
    e.set_particles(sp, p)
    good = e.cool(sp, SYNC, IC, QUANTUM, dry=True, cells=True)
    assert good.stats["seen"] == 500 and good.isum != 0
    nv = n_voxels(grid)
    energy = C.c_int64(-77)
    cells = np.full(nv, -5, np.int64)

    def call(species=sp, desc=True, out=True, patch=None):
        d = eng.CoolDesc(SYNC, IC, QUANTUM, 0, 0)
        if patch:
            patch(d)
        return l.vpic_hip_species_cool(e._h, species, C.byref(d) if desc else None, C.byref(energy) if out else None,
                                       cells.ctypes.data_as(C.c_void_p))

    def fails(rc, word):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert word in msg, msg
        assert energy.value == -77 and np.all(cells == -5)
        assert e.cool_stats() == good.stats
        assert e.get_particles(sp).tobytes() == p.tobytes()

    fails(call(species=sp + 1), "sp")
    fails(call(species=-1), "sp")
    fails(call(desc=False), "NULL c")
    fails(call(out=False), "energy")
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        fails(call(patch=lambda d: setattr(d, "sync", bad)), "sync")
        fails(call(patch=lambda d: setattr(d, "ic", bad)), "ic")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        fails(call(patch=lambda d: setattr(d, "quantum", bad)), "quantum")
    fails(call(patch=lambda d: setattr(d, "flags", 2)), "flag")
    fails(call(patch=lambda d: setattr(d, "flags", 1 | 4)), "flag")
    fails(l.vpic_hip_species_cool_stats(e._h, None), "output")
    with pytest.raises(V.VpicHipError):
        e.cool(sp, -1.0)
    with pytest.raises(V.VpicHipError):
        e.cool(sp + 3, SYNC)
    # sync == 0 is allowed, and the engine still answers
    assert call(patch=lambda d: setattr(d, "sync", 0.0)) == 0 and energy.value != -77
    e.close()


if __name__ == "__main__":
    check_state(sys.argv[1], int(sys.argv[2]))
    print("child OK")
