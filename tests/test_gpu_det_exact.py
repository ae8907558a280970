"""The deterministic push against an exact reference, word for word (GPU box only).

In deterministic accumulation (include/vpic_hip.h: vpic_hip_set_accumulation) every one of the 12 deposits of every streak
is rounded to a 64-bit fixed-point number and summed as an integer, and acc_finalize rounds each sum once into the float
accumulator -- so nothing depends on array order, wavefront scheduling, windows or atomics, and an order-free CPU
computation predicts every word.  That computation is the oracle's push with its fixed-point switch on (tests/det_exact.py,
oracle/vpic_oracle.h: orc_set_fixed_accumulator; pinned on the CPU by tests/test_det_ref.py).  Every comparison in this file
is exact: accumulators as uint32 words, ghosts included; particles and movers by tag, bit for bit; fields after full steps.

Instances (policy.h: PushInstance): det_tile (tile order by cell), det_tile_only (VPIC_HIP_TILE_COARSE=1, fresh child),
det_row (the reference's order: asked for, or kept on grids thinner than a tile), and the windowless fixed-point deposits
of injection.  Emission (vpic_hip_emit) and the reflux walls are held exactly elsewhere: the device takes the square root
of the emitter's charge law in float, the oracle in double, so the oracle is no exact reference for it -- the numpy
restatement of the arithmetic include/vpic_hip.h states is (tests/source_ref.py, tests/test_gpu_emit.py), and
tests/test_gpu_reflux.py holds every round of boundary_p with Maxwellian reflux handlers to the oracle."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from conftest import bits_equal  # noqa: E402
import det_exact as D  # noqa: E402
from det_exact import L, pyorc  # noqa: E402
from species_states import package, run_child  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = pyorc.fixed_scale(D.Q0)
N_TAIL, N_DOOMED = 1500, 200
TAIL_SORT_MIN = {"tail_below": 100, "tail_above": 1 << 20}          # below / above the tail's length
THIN = ((5, 3, 2), (16, 1, 6))                                      # thinner than a tile on some axis: the reference's order
N_PARTICLES = {(4, 4, 4): 3000, (10, 9, 7): 8000, (5, 3, 2): 2000, (16, 1, 6): 3000, (65, 5, 4): 16000}
STATES = ("tile", "tile_only", "voxel", "thin", "unsorted", "tail_below", "tail_above")
INSTANCE = {"tile": "det_tile", "unsorted": "det_tile", "tail_below": "det_tile", "tail_above": "det_tile",
            "tile_only": "det_tile_only", "voxel": "det_row", "thin": "det_row"}
CROSSING = {"cold": (D.COLD, None), "hot0": (D.HOT, 0), "hot1": (D.HOT, 1)}        # momentum spread, VPIC_HIP_STAGE

# (grid, particle walls, array state, crossing)
CASES = [
    ((10, 9, 7), "periodic", "tile", "hot0"),
    ((10, 9, 7), "reflect", "tile", "hot1"),
    ((10, 9, 7), "absorb_x_reflect_z", "tile", "cold"),
    ((10, 9, 7), "reflect_y_absorb_z", "tile", "hot1"),
    ((10, 9, 7), "periodic", "tile_only", "hot0"),
    ((10, 9, 7), "reflect", "tile_only", "hot1"),
    ((10, 9, 7), "absorb_x_reflect_z", "tile_only", "cold"),
    ((10, 9, 7), "reflect_y_absorb_z", "tile_only", "hot1"),
    ((5, 3, 2), "periodic", "thin", "hot0"),
    ((5, 3, 2), "reflect", "thin", "cold"),
    ((5, 3, 2), "absorb_x_reflect_z", "thin", "hot1"),
    ((5, 3, 2), "reflect_y_absorb_z", "thin", "hot0"),
    ((10, 9, 7), "periodic", "voxel", "hot0"),
    ((10, 9, 7), "reflect_y_absorb_z", "voxel", "cold"),
    ((10, 9, 7), "reflect", "unsorted", "hot0"),
    ((10, 9, 7), "periodic", "unsorted", "cold"),
    ((10, 9, 7), "absorb_x_reflect_z", "tail_below", "hot0"),
    ((10, 9, 7), "reflect_y_absorb_z", "tail_above", "cold"),
    ((10, 9, 7), "reflect_y_absorb_z", "tail_below", "cold"),
    ((10, 9, 7), "absorb_x_reflect_z", "tail_above", "hot1"),
    ((4, 4, 4), "periodic", "tile", "hot0"),
    ((4, 4, 4), "reflect", "tile", "cold"),
    ((4, 4, 4), "absorb_x_reflect_z", "voxel", "hot1"),
    ((16, 1, 6), "periodic", "thin", "hot0"),
    ((16, 1, 6), "absorb_x_reflect_z", "thin", "cold"),
    ((65, 5, 4), "periodic", "tile", "cold"),
    ((65, 5, 4), "reflect", "tile", "hot0"),
    ((65, 5, 4), "reflect_y_absorb_z", "voxel", "hot1"),
]


def case_id(c):
    return "%dx%dx%d-%s-%s-%s" % (c[0] + c[1:])


@pytest.fixture(scope="module")
def V():
    return package()


def live_particles(e, sp):
    """(particles, their slots in the species' array): movers name slots, and a download of a species with dead slots
    would compact it first"""
    if e.species_stats(sp)["dead_slots"]:
        r = e.select(sp, index=True)
        assert r.count == e.np(sp) == len(r.particles)
        return r.particles, r.index
    p = e.get_particles(sp)
    return p, np.arange(len(p))


def movers_by_tag(e, sp, p, slots):
    pm = e.get_movers(sp)
    order = np.argsort(slots)
    at = np.searchsorted(slots[order], pm["i"])
    assert np.array_equal(slots[order][at], pm["i"]), "a mover names a slot that holds no live particle"
    tags = p["tag"][order][at]
    o = np.argsort(tags, kind="stable")
    return tags[o], pm[o]


def same_disp(a, b):
    """the movers' remaining displacements bit for bit (their `i` names a slot of the array, whose order is the engine's)"""
    return all(bits_equal(a[c], b[c]) for c in ("dispx", "dispy", "dispz"))


def check(e, sps, refs, dims, scale, what=""):
    """The engine's accumulator against the exact sums of the last of refs (a chain of det_exact.Pushed into the same
    sums), all 12 words of every voxel as uint32 (so a zero sum must be +0.0); per species, particles by tag and movers
    by their particle's tag, bit for bit."""
    ref = refs[-1]
    bad = D.describe_bad_words(e.get_accumulator(), ref.a64, ref.streaks, scale, dims)
    assert bad is None, what + "\n" + bad
    for sp, r in zip(sps, refs):
        p, slots = live_particles(e, sp)
        assert len(p) == len(r.p), what
        assert bits_equal(D.by_tag(p), D.by_tag(r.p)), what + ": particles differ from the oracle's"
        assert e.nm(sp) == r.nm, what + ": %d movers, the oracle has %d" % (e.nm(sp), r.nm)
        if r.nm:
            tags, pm = movers_by_tag(e, sp, p, slots)
            rtags, rpm = r.movers_by_tag()
            assert np.array_equal(tags, rtags) and same_disp(pm, rpm), what + ": movers differ from the oracle's"


def engine(V, dims, walls, q_ref=D.Q0, order="engine"):
    """(engine in deterministic mode with the random interpolator loaded, oracle grid, that interpolator)"""
    args, kw, og = D.grids(dims, walls)
    e = V.Engine(V.make_grid(*args, **kw))
    e.set_vacuum()
    e.set_accumulation("deterministic", q_ref)
    e.set_sort_order(order)
    fi = D.interpolator(og)
    e.set_interpolator(fi)
    return e, og, fi


def wall_cells(dims, walls):
    """voxels of the cells next to one absorbing wall of the layout, its axis and side"""
    nx, ny, nz = dims
    face = [f for f in (3, 5, 0, 2) if D.WALLS[walls][f] == D.ABSORB][0]
    axis, hi = face % 3, face >= 3
    r = [np.arange(1, n + 1) for n in dims]
    r[axis] = np.array([dims[axis] if hi else 1])
    x, y, z = np.meshgrid(*r, indexing="ij")
    return L.voxel(x, y, z, nx, ny, nz).reshape(-1), axis, hi


def run_case(V, case, setenv):
    """One push of one case: the engine in the array state asked for, then clear_accumulators, advance_p, and check."""
    dims, walls, state, crossing = case
    u_scale, stage = CROSSING[crossing]
    if stage is not None:
        setenv("VPIC_HIP_STAGE", str(stage))
    if state in TAIL_SORT_MIN:
        setenv("VPIC_HIP_TAIL_SORT_MIN", str(TAIL_SORT_MIN[state]))
    n = N_PARTICLES[dims]
    e, og, fi = engine(V, dims, walls, order="reference" if state == "voxel" else "engine")
    p = D.particles(1, n, dims, u_scale)
    sp = e.new_species(D.Q_M, n + N_TAIL + N_DOOMED + 64, n + N_TAIL + N_DOOMED + 64)
    what = case_id(case)
    if state in TAIL_SORT_MIN:
        # tile order, an appended tail, and dead slots: one step of the resident exchange removes the particles that
        # reach an absorbing wall (N_DOOMED are placed for it); the NEXT push is the one compared
        cells, axis, hi = wall_cells(dims, walls)
        d = D.particles(2, N_DOOMED, dims, 0.0, first_tag=10 ** 7, cells=cells)
        d[("dx", "dy", "dz")[axis]] = 0.9 if hi else -0.9
        d[("ux", "uy", "uz")[axis]] = 3.0 if hi else -3.0
        e.set_particles(sp, np.concatenate([p, d]))
        e.sort_p(sp)
        assert e.species_order(sp) == "tile"
        e.append_particles(sp, D.particles(3, N_TAIL, dims, u_scale, first_tag=10 ** 6))
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(sp)
        e.exchange_pack([0] * 6, [0] * 6, 8192)
        e.exchange_finish([])
        assert e.exchange_flags == 0
        assert e.species_stats(sp)["dead_slots"] >= N_DOOMED and e.nm(sp) == 0
        p, _ = live_particles(e, sp)
        assert len(p) == n + N_TAIL + N_DOOMED - e.species_stats(sp)["dead_slots"]
        e.set_interpolator(D.interpolator(og, seed=8))          # (other fields for the push that is compared)
        fi = D.interpolator(og, seed=8)
    else:
        e.set_particles(sp, p)
        if state != "unsorted":
            e.sort_p(sp)
        if state != "unsorted":                                  # (an unsorted species is sorted by the push itself, below)
            assert e.species_order(sp) == ("voxel" if INSTANCE[state] == "det_row" else "tile"), what
    if state in ("tile", "tile_only") + tuple(TAIL_SORT_MIN):
        assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0), what
    ref = D.Pushed(og, p, fi, SCALE)
    e.clear_accumulators()
    e.advance_p(sp)
    # the instance that was meant to run did: det_row leaves no tile order behind, the others keep (or make) it
    if INSTANCE[state] == "det_row":
        assert e.species_order(sp) != "tile", what
    else:
        assert e.species_order(sp) == "tile", what
        assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0), what
        assert state in TAIL_SORT_MIN or e.species_stats(sp)["sorts"] == 1, what
    # the case is what its name says: cold hardly crosses, hot crosses for more than a third (and, on a periodic grid of
    # three axes, some particle crosses three faces in one step)
    moved = (ref.p["i"] != p["i"])
    if u_scale == D.HOT:
        assert moved.mean() + ref.nm / len(p) > 1 / 3, what
        if walls == "periodic" and min(dims) > 1:
            nx, ny = dims[0] + 2, dims[1] + 2
            c0 = np.stack([p["i"] % nx, p["i"] // nx % ny, p["i"] // (nx * ny)])
            c1 = np.stack([ref.p["i"] % nx, ref.p["i"] // nx % ny, ref.p["i"] // (nx * ny)])
            assert ((c0 != c1).sum(axis=0) == 3).any(), what
    else:
        assert 0 < moved.mean() < 0.1, what
    if "absorb" in walls:
        assert ref.nm > 0, what
    assert ref.streaks.sum() > len(p) and np.abs(ref.a64).max() < 2 ** 62
    check(e, [sp], [ref], dims, SCALE, what)
    e.close()


def test_the_cases_cover_every_value_of_every_axis_and_every_instance_every_wall_layout():
    assert {c[0] for c in CASES} == set(N_PARTICLES) == {(4, 4, 4), (10, 9, 7), (5, 3, 2), (16, 1, 6), (65, 5, 4)}
    assert {c[1] for c in CASES} == set(D.WALLS) and len(D.WALLS) == 4
    assert {c[2] for c in CASES} == set(STATES)
    assert {c[3] for c in CASES} == set(CROSSING)
    assert len(set(CASES)) == len(CASES)
    for dims, walls, state, _ in CASES:
        assert (state == "thin") == (dims in THIN)                 # a thin grid keeps the reference's order whatever is asked
        assert state not in TAIL_SORT_MIN or "absorb" in walls     # dead slots need a wall that removes particles
    for instance in ("det_tile", "det_tile_only", "det_row"):
        on = (5, 3, 2) if instance == "det_row" else (10, 9, 7)
        assert {c[1] for c in CASES if INSTANCE[c[2]] == instance and c[0] == on} == set(D.WALLS), instance
    # hot species by tile only with the positions of a pass staged and not (VPIC_HIP_STAGE)
    assert {c[3] for c in CASES if c[2] == "tile_only"} >= {"hot0", "hot1"}
    assert TAIL_SORT_MIN["tail_below"] < N_TAIL < TAIL_SORT_MIN["tail_above"]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_push_every_word(V, case, monkeypatch):
    if case[2] == "tile_only":
        run_child(__file__, ["tile_only", CASES.index(case)], 120)
    else:
        run_case(V, case, monkeypatch.setenv)


# ---- further single cases ------------------------------------------------------------------------------------------------
def one_push(V, dims, walls, p, order, q_ref=D.Q0, scale=SCALE, what="", q_m=D.Q_M, by_tile_only=None):
    e, og, fi = engine(V, dims, walls, q_ref=q_ref, order=order)
    sp = e.new_species(q_m, max(len(p), 1) + 64, max(len(p), 1) + 64)
    e.set_particles(sp, p)
    if len(p):
        e.sort_p(sp)
        assert e.species_order(sp) == ("tile" if order == "engine" else "voxel")
    if by_tile_only is not None:
        assert e.species_stats(sp)["by_tile_only"] == by_tile_only
    ref = D.Pushed(og, p, fi, scale, q_m)
    e.clear_accumulators()
    e.advance_p(sp)
    check(e, [sp], [ref], dims, scale, what)
    e.close()
    return ref


@pytest.mark.parametrize("order", ["engine", "reference"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_a_handful_of_particles(V, n, order):
    """an empty species (every word +0.0), one particle, and a wavefront less one, exactly one, plus one"""
    ref = one_push(V, (10, 9, 7), "reflect", D.particles(4, n, (10, 9, 7), D.HOT), order, what="%d particles" % n)
    assert ref.streaks.sum() >= n and (n == 0) == (not ref.a64.any())


@pytest.mark.parametrize("order", ["engine", "reference"])
def test_one_full_cell_beside_empty_ones(V, order):
    """300 cold particles in one cell: a run of equal cells longer than a wavefront (the integer run sums of det_tile)"""
    cell = [L.voxel(6, 5, 4, 10, 9, 7)]
    ref = one_push(V, (10, 9, 7), "periodic", D.particles(5, 300, (10, 9, 7), D.COLD, cells=cell), order)
    assert ref.streaks[cell[0]] >= 290 and (ref.streaks > 0).sum() < 8


def test_stale_tiles(V):
    """Two pushes without a sort in between, cleared before the second: hot particles have left their tiles, some of them
    the tiles' windows, and deposit through global memory.  The second push is the one compared."""
    dims = (10, 9, 7)
    e, og, fi = engine(V, dims, "reflect")
    p = D.particles(6, 8000, dims, D.HOT)
    sp = e.new_species(D.Q_M, len(p) + 64, 64)
    e.set_particles(sp, p)
    e.sort_p(sp)
    first = D.Pushed(og, p, fi, SCALE)
    ref = D.Pushed(og, first.p, fi, SCALE)
    for _ in range(2):
        e.clear_accumulators()
        e.advance_p(sp)
    assert e.species_stats(sp)["sorts"] == 1 and e.species_order(sp) == "tile"
    check(e, [sp], [ref], dims, SCALE)
    e.close()


@pytest.mark.parametrize("order", ["engine", "reference"])
def test_two_species_of_opposite_charge_into_one_accumulator(V, order):
    """no clear in between: the words hold the sum of both species' integers, which nearly cancel"""
    dims = (10, 9, 7)
    e, og, fi = engine(V, dims, "absorb_x_reflect_z", order=order)
    pa = D.particles(7, 6000, dims, D.HOT, q0=-D.Q0)
    pb = D.particles(7, 6000, dims, D.HOT, q0=D.Q0, first_tag=10 ** 6)          # the same places and momenta
    sa, sb = e.new_species(-1.0, 6064, 6064), e.new_species(0.5, 6064, 6064)
    for sp, p in ((sa, pa), (sb, pb)):
        e.set_particles(sp, p)
        e.sort_p(sp)
    ra = D.Pushed(og, pa, fi, SCALE, -1.0)
    rb = D.Pushed(og, pb, fi, SCALE, 0.5, a64=ra.a64, streaks=ra.streaks)
    e.clear_accumulators()
    e.advance_p(sa)
    e.advance_p(sb)
    check(e, [sa, sb], [ra, rb], dims, SCALE)
    e.close()


@pytest.mark.parametrize("order", ["engine", "reference"])
@pytest.mark.parametrize("charges", ["mixed_signs", "wide", "q_ref_0"])
def test_charges(V, charges, order):
    """mixed signs of q inside one species; charges from 2^-12 q_ref to 2^10 q_ref in one species (the stated range: a
    deposit of 4.2 x 2^10 q_ref is below 2^48 quanta); q_ref = 0: the scale comes from the largest charge uploaded"""
    dims = (10, 9, 7)
    p = D.particles(8, 6000, dims, D.HOT)
    rng = np.random.default_rng(9)
    q_ref, scale = D.Q0, SCALE
    if charges == "mixed_signs":
        p["q"] *= rng.choice([-1.0, 1.0], len(p)).astype(np.float32)
    elif charges == "wide":
        p["q"] = (D.Q0 * 2.0 ** rng.uniform(-12, 10, len(p))).astype(np.float32)
        p["q"][:2] = np.float32(D.Q0) * np.array([2.0 ** -12, 2.0 ** 10], np.float32)
    else:
        q_ref, scale = 0.0, pyorc.fixed_scale(float(np.abs(p["q"]).max()))
        assert scale != pyorc.fixed_scale(1.0)
    one_push(V, dims, "reflect", p, order, q_ref=q_ref, scale=scale, what=charges)


@pytest.mark.parametrize("state", ["tile", "tile_only", "voxel"])
def test_light_particles_show_every_quantum(V, state, monkeypatch):
    """Charges of 2^-20 q_ref: a deposit is below 2^18 quanta and every sum below 2^24, so the float accumulator holds the
    integer sums THEMSELVES -- a float has 24 bits -- and one quantum too many or too few in one deposit of one particle
    changes a word.  (At charges near q_ref a sum is some 2^37 quanta, of which finalize keeps the upper 24 bits.)"""
    dims = (10, 9, 7)
    if state == "tile_only":
        monkeypatch.setenv("VPIC_HIP_TILE_COARSE", "1")                # (read when the engine is created)
    p = D.particles(15, 8000, dims, D.HOT, q0=-D.Q0 * 2.0 ** -20)
    ref = one_push(V, dims, "reflect_y_absorb_z", p, "reference" if state == "voxel" else "engine", what=state,
                   by_tile_only=None if state == "voxel" else int(state == "tile_only"))
    assert 2 ** 16 < np.abs(ref.a64).max() < 2 ** 24 and ref.nm > 0
    exact = pyorc.finalize(ref.a64, SCALE).view(np.float32).reshape(-1, 12).astype(np.float64) * SCALE
    assert np.array_equal(exact, ref.a64.astype(np.float64))


def test_a_chargeless_species_beside_a_charged_one(V):
    """it adds nothing, and its particles are still the oracle's"""
    dims = (10, 9, 7)
    e, og, fi = engine(V, dims, "reflect_y_absorb_z")
    pa = D.particles(10, 5000, dims, D.HOT)
    pb = D.particles(11, 5000, dims, D.HOT, first_tag=10 ** 6)
    pb["q"] = 0
    sa, sb = e.new_species(-1.0, 5064, 5064), e.new_species(-1.0, 5064, 5064)
    for sp, p in ((sa, pa), (sb, pb)):
        e.set_particles(sp, p)
        e.sort_p(sp)
    ra = D.Pushed(og, pa, fi, SCALE)
    rb = D.Pushed(og, pb, fi, SCALE, a64=ra.a64, streaks=ra.streaks)
    assert np.array_equal(rb.a64, ra.a64) and rb.streaks.sum() > ra.streaks.sum()
    e.clear_accumulators()
    e.advance_p(sb)
    e.advance_p(sa)
    check(e, [sa, sb], [ra, rb], dims, SCALE)
    e.close()


@pytest.mark.parametrize("light", [False, True])
def test_injection(V, light):
    """Injectors finish their move through the windowless fixed-point deposits (particles.hip: boundary_inject_kernel)
    against orc_boundary_p_inject with the switch on: the accumulator exact, the particles -- the species' own and the
    arrivals, which bring their tags -- and the movers of those that stop on an absorbing wall bit for bit."""
    dims = (10, 9, 7)
    e, og, fi = engine(V, dims, "absorb_x_reflect_z")
    n, n_inj = 1000, 20000            # (many: a wrong last bit of v5 shows only in the few words that are small by cancellation)
    p = D.particles(12, n, dims, D.HOT)
    sp = e.new_species(D.Q_M, n + n_inj + 64, n_inj + 64)
    e.set_particles(sp, p)
    e.sort_p(sp)
    # (light: charges of 2^-20 q_ref, sums below 2^24 quanta -- the accumulator then shows every quantum, see above)
    src = D.particles(13, n_inj, dims, D.HOT, first_tag=10 ** 6, q0=-D.Q0 * (2.0 ** -20 if light else 1.0))
    rng = np.random.default_rng(14)
    inj = np.zeros(n_inj, L.particle_injector_t)
    for c in ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q"):
        inj[c] = src[c]
    for c in ("dispx", "dispy", "dispz"):
        inj[c] = rng.uniform(-0.9, 0.9, n_inj).astype(np.float32)
    inj["sp_id"] = sp
    tags = np.zeros((n_inj, 2), np.int64)
    tags[:, 0] = src["tag"]
    e.clear_accumulators()
    e.inject_aged(inj, tags)
    # the oracle appends the injectors last to first (boundary_p.c:457-497)
    rp = np.zeros(n + n_inj, L.particle_t)
    rp[:n] = p
    rp["tag"][n:] = src["tag"][::-1]
    rpm = np.zeros(n_inj, L.particle_mover_t)
    ra = np.zeros(og.nv + 1, L.accumulator_t)
    with pyorc.fixed_accumulator(og, SCALE) as (a64, streaks):
        new_np, nm = pyorc.boundary_p_inject(rp, n, rpm, 0, inj, ra, og)
    assert new_np == n + n_inj and nm > 0 and streaks.sum() > n_inj
    assert not light or np.abs(a64).max() < 2 ** 24
    bad = D.describe_bad_words(e.get_accumulator(), a64, streaks, SCALE, dims)
    assert bad is None, bad
    got = e.get_particles(sp)
    assert bits_equal(D.by_tag(got), D.by_tag(rp))
    assert e.nm(sp) == nm
    tg, pm = movers_by_tag(e, sp, got, np.arange(len(got)))
    rt = rp["tag"][rpm["i"][:nm]]
    o = np.argsort(rt, kind="stable")
    assert np.array_equal(tg, rt[o]) and same_disp(pm, rpm[:nm][o])
    e.close()


# ---- full steps: fields bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["engine", "reference"])
@pytest.mark.parametrize("walls", ["periodic", "pec_z"])
def test_eight_steps_fields_bit_for_bit(V, walls, order):
    """8 x vpic_hip_step(k, 4) against pyorc.step(det_scale=...): the oracle's step with its accumulator replaced by the
    finalized exact sums before it is unloaded.  The per-voxel field kernels are bit-exact and the sums are exact, so
    every field component, jf included, is equal after every step, and the particles by tag at the end.  The oracle never
    sorts: exact sums do not care."""
    dims, ppc = (10, 9, 7), 8
    nx, ny, nz = dims
    dt = 0.95 / np.sqrt(3.0)
    fbc = [0, 0, L.PEC_FIELDS, 0, 0, L.PEC_FIELDS] if walls == "pec_z" else None
    pwalls = [0, 0, D.REFLECT, 0, 0, D.REFLECT] if walls == "pec_z" else "periodic"
    args, kw, og = D.grids(dims, pwalls, dt)
    if fbc:
        kw["fbc"] = fbc
        og = pyorc.make_grid(*args, **kw)
    e = V.Engine(V.make_grid(*args, **kw))
    e.set_vacuum()
    q0 = 0.004
    scale = pyorc.fixed_scale(q0)
    e.set_accumulation("deterministic", q0)
    e.set_sort_order(order)
    n = nx * ny * nz * ppc
    species, sps = [], []
    for k, drift in enumerate((0.2, -0.2)):
        p = D.particles(20 + k, n, dims, 0.1, q0=-q0, first_tag=1 + k * n)
        p["ux"] += np.float32(drift)
        sp = e.new_species(-1.0, n + 64, n)
        e.set_particles(sp, p)
        sps.append(sp)
        species.append(dict(p=p.copy(), np=n, q_m=-1.0, pm=np.zeros(n, L.particle_mover_t)))
    e.load_interpolator()
    f, fi, a = np.zeros(og.nv, L.field_t), np.zeros(og.nv, L.interpolator_t), np.zeros(og.nv + 1, L.accumulator_t)
    m = pyorc.vacuum_coefficients()
    for step in range(8):
        e.step(step, 4)
        pyorc.step(f, fi, a, m, species, og, det_scale=scale)
        got = e.get_fields()
        for c in ("jfx", "jfy", "jfz", "ex", "ey", "ez", "cbx", "cby", "cbz"):
            assert np.array_equal(got[c], f[c]), "step %d: %s differs in %d voxels" % (step, c, (got[c] != f[c]).sum())
    assert np.abs(f["ex"]).max() > 0 and np.abs(f["cbz"]).max() > 0
    for sp, r in zip(sps, species):
        assert bits_equal(D.by_tag(e.get_particles(sp)), D.by_tag(r["p"][:r["np"]]))
    e.close()


if __name__ == "__main__":                                          # the fresh child of the tile_only cases (run_child)
    assert sys.argv[1] == "tile_only" and os.environ.get("VPIC_HIP_TILE_COARSE") == "1"
    run_case(package(), CASES[int(sys.argv[2])], os.environ.__setitem__)
    print("child OK")
