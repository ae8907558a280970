"""The surface emitter (vpic_hip_emit) in test mode against the restatement of its arithmetic (GPU box only).

include/vpic_hip.h states what vpic_hip_emit computes from a table of draws (vpic_hip_set_emit_draws) operation by
operation; tests/source_ref.py restates it in numpy float32 / float64, one operation per line, and produces the injector
records, whose moves the oracle's orc_boundary_p_inject finishes.  Every operation is + - * / sqrt fabs, correctly rounded on
both sides, so equality is the criterion (tests/test_source_ref.py holds the restatement to the oracle's orc_child_langmuir,
pinned on the reference's own model: cell, position and momenta bit-equal, charge and displacements within derived bounds):

  the species' particles from before            untouched, in place
  the emitted particles (tag == tag2 == 0)      bit-equal, as a multiset of whole records
  movers                                        the same particles, displacements bit-equal
  rhob                                          per node within the bound of source_ref.rhob_bound; bit-equal at <= 2 terms
  every other field component                   untouched
  accumulator, deterministic mode               all 12 words of every voxel as uint32
  accumulator, float mode                       ACC_TOL of test_gpu_kernels.py
  one advance_p afterwards                      particles and movers bit-equal, the accumulator exact in deterministic mode

Emission into a species with dead slots (the tile_tail_holes state of species_states.py) is the last test of the file: the
new particles go behind the array's extent, the live ones and the dead slots stay where they are."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from conftest import bits_equal  # noqa: E402
import source_ref as S  # noqa: E402
from source_ref import D, L, pyorc  # noqa: E402
from species_states import package  # noqa: E402

pytestmark = pytest.mark.gpu
ACC_TOL = 2e-6
DIMS, BOX = (10, 9, 7), (10.0, 13.5, 5.25, 0.3)                     # unequal cells: 1, 1.5, 0.75
WALLS = [S.ABSORB, 0, S.REFLECT, S.ABSORB, 0, S.REFLECT]
UT_PERP, UT_PARA = 0.8, 1.2                                          # hot: some emitted particles reach a wall within their first step
RECORD = ("uz", "uy", "ux", "dz", "dy", "dx", "q", "tag", "i")


@pytest.fixture(scope="module")
def V():
    return package()


def rec_sorted(p, extra=None):
    """p (and extra, row for row) in an order that depends on the records alone"""
    o = np.lexsort([p[c].view(np.uint32) if p[c].dtype == np.float32 else p[c] for c in RECORD])
    return p[o] if extra is None else (p[o], extra[o])


def same_movers(got_p, got_pm, ref_p, ref_pm, what):
    assert len(got_pm) == len(ref_pm), what + ": %d movers, the reference has %d" % (len(got_pm), len(ref_pm))
    if len(ref_pm):
        gp, gm = rec_sorted(got_p[got_pm["i"]], got_pm)
        rp, rm = rec_sorted(ref_p[ref_pm["i"]], ref_pm)
        assert bits_equal(gp, rp) and all(bits_equal(gm[c], rm[c]) for c in ("dispx", "dispy", "dispz")), what + ": movers differ"


def check_accumulator(acc, a, a64, streaks, scale, og, mode, what):
    if mode == "deterministic":
        bad = D.describe_bad_words(acc, a64, streaks, scale, (og.nx, og.ny, og.nz))
        assert bad is None, what + "\n" + bad
    else:
        g = np.stack([acc[c] for c in ("jx", "jy", "jz")]).astype(np.float64)[:, :og.nv]
        w = np.stack([a[c] for c in ("jx", "jy", "jz")]).astype(np.float64)[:, :og.nv]
        assert np.abs(g - w).max() <= ACC_TOL * np.abs(w).max(), what + ": accumulator off by %.3g of %.3g" % (np.abs(g - w).max(), np.abs(w).max())


def world(seed, n_comp, dims=DIMS, box=BOX):
    """(oracle grid arguments, interpolator, components): faces of all six orientations, a third of them in cells on the
    domain's surface (the doubled rhob weights), volume codes among them; E uniform in (-2, 2): about half the faces pull
    the species out"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    nv = L.nv(nx, ny, nz)
    fi = np.zeros(nv, L.interpolator_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        fi[c] = rng.uniform(-2, 2, nv).astype(np.float32)
    codes = np.array(list(S.EMIT_FACES) + [13, 0])
    t = codes[np.arange(n_comp) % 8]
    t[n_comp - n_comp % 8:] = codes[:n_comp % 8]
    c = [rng.integers(1, m + 1, n_comp) for m in dims]
    for k in range(0, n_comp, 3):                                      # onto a surface plane of the face's own axis or another
        axis = int(rng.integers(0, 3))
        c[axis][k] = dims[axis] if rng.integers(0, 2) else 1
    comps = (L.voxel(c[0], c[1], c[2], nx, ny, nz).astype(np.int64) * 32 + t).astype(np.int32)
    return fi, rng.permutation(comps)


def slot_draws(seed, n):
    rng = np.random.default_rng(seed)
    d = np.zeros((n, 6))
    d[:, :2] = rng.uniform(0, 1, (n, 2))
    d[:, 2:5] = rng.standard_normal((n, 3))
    d[:, 5] = rng.uniform(0, 1, n)
    return d


def run_emit(V, dims, box, walls, fi, comps, n_emit, ut_perp, ut_para, q_m, coef, thresh, draws, mode, what,
             resident=0, fits_exactly=False, learn_scale=False):
    """One vpic_hip_emit against the restatement, then one advance_p.  resident: particles the species holds beforehand, in
    tile order.  fits_exactly: max_np == the particles afterwards.  learn_scale: deterministic mode without a reference
    charge -- in the emission the scale comes from the largest charge among the injectors; with mode == "float" the switch
    to deterministic follows the emission, and the push's scale comes from Species::q_max, which has to have learnt it."""
    kw = dict(pbc=list(walls))
    args = dims + box[:3] + (np.float32(box[3]),)
    og = pyorc.make_grid(*args, **kw)
    inj, left = S.emit_restatement(og, fi, comps, n_emit, ut_perp, ut_para, q_m, coef, thresh, draws)
    q_top = float(np.abs(inj["q"]).max()) if len(inj) else 0.0
    q_ref = 0.0 if learn_scale else 0.05
    scale = pyorc.fixed_scale(q_top if learn_scale else q_ref)
    e = V.Engine(V.make_grid(*args, **kw))
    e.set_vacuum()
    if mode == "deterministic":
        e.set_accumulation("deterministic", q_ref)
    e.set_sort_order("engine")
    e.set_interpolator(fi)
    e.set_emit_draws(draws)
    cap = resident + len(inj) + (0 if fits_exactly else 64)
    sp = e.new_species(q_m, max(cap, 1), max(cap, 1))
    if resident:
        p0 = D.particles(51, resident, dims, 0.3, q0=0.02 if q_m > 0 else -0.02)
        e.set_particles(sp, p0)
        e.sort_p(sp)
        assert e.species_order(sp) == "tile"
    before, f_before = e.get_particles(sp), e.get_fields()
    nb = len(before)
    e.clear_accumulators()
    e.emit(sp, comps, n_emit, ut_perp, ut_para, coef=coef, thresh=thresh)
    after, pm, acc, f_after = e.get_particles(sp), e.get_movers(sp), e.get_accumulator(), e.get_fields()
    # the reference: the restatement's injectors, their moves finished by the oracle
    ref = np.zeros(nb + len(inj), L.particle_t)
    ref[:nb] = before
    rpm = np.zeros(len(inj) + 1, L.particle_mover_t)
    a = np.zeros(og.nv + 1, L.accumulator_t)
    with pyorc.fixed_accumulator(og, scale) as (a64, streaks):
        new_np, nm = pyorc.boundary_p_inject(ref, nb, rpm, 0, inj, a, og)
    assert new_np == nb + len(inj)
    assert len(after) == new_np, what + ": np %d, the reference has %d" % (len(after), new_np)
    assert bits_equal(after[:nb], before), what + ": the particles from before changed"
    assert np.all(after["tag"][nb:] == 0) and np.all(after["tag2"][nb:] == 0), what
    gt, rt = rec_sorted(after[nb:]), rec_sorted(ref[nb:])
    if not bits_equal(gt, rt):
        bad = [k for k in range(len(gt)) if not bits_equal(gt[k:k + 1], rt[k:k + 1])]
        raise AssertionError(what + ": %d of %d emitted particles differ; first: got %s, restatement %s" % (len(bad), len(gt), gt[bad[0]], rt[bad[0]]))
    same_movers(after, pm, ref, rpm[:nm], what)
    bad = S.describe_rhob(f_after["rhob"], f_before["rhob"], left, og)
    assert bad is None, what + ": " + bad
    for name in f_after.dtype.names:
        if name != "rhob":
            assert bits_equal(f_after[name], f_before[name]), what + ": field component %s changed" % name
    if len(inj):
        check_accumulator(acc, a, a64, streaks, scale, og, mode, what)
    # the movers leave (absorbing and reflecting walls only: nothing comes back), then one more push
    if e.nm(sp):
        e.boundary_p_pack()
        assert e.nm(sp) == 0
    if learn_scale and mode == "float":
        mode = "deterministic"
        e.set_accumulation("deterministic", 0.0)
    p1 = e.get_particles(sp)
    e.clear_accumulators()
    e.advance_p(sp)
    r = D.Pushed(og, p1, fi, scale, q_m)
    got = e.get_particles(sp)
    w = what + ", the push after the emission"
    assert len(got) == len(r.p) and bits_equal(rec_sorted(got), rec_sorted(r.p)), w + ": particles differ from the oracle's"
    same_movers(got, e.get_movers(sp), r.p, r.pm, w)
    if len(p1):
        check_accumulator(e.get_accumulator(), r.a, r.a64, r.streaks, scale, og, mode, w)
    e.close()
    return inj, nm


def test_the_72_faces_of_the_fixture(V):
    """the faces, interpolator, parameters and draws of tests/golden/reflux.npz (the reference's own run of its model)"""
    g = np.load(os.path.join(HERE, "golden", "reflux.npz"))
    dims, box = tuple(int(v) for v in g["dims"]), tuple(float(v) for v in g["box"])
    n_emit, ut_perp, ut_para, q_m = [float(v) for v in g["emit_par"]]
    og = pyorc.make_grid(*dims, *box[:3], np.float32(box[3]))
    emits = S._emit_common(og, g["emit_fi"], g["emit_component"], int(n_emit), q_m, 0.0)[0]
    draws = S.slot_table(emits, g["emit_draws"])
    for mode in ("deterministic", "float"):
        inj, _ = run_emit(V, dims, box, [0] * 6, g["emit_fi"], g["emit_component"], int(n_emit), ut_perp, ut_para, q_m,
                          S.COEF["child_langmuir"], 0.0, draws, mode, "fixture, " + mode)
        assert len(inj) == len(g["emit_p"])


# (components, n_emit per face, coef, thresh, q_m, accumulation)
CASES = [
    (255, 1, "child_langmuir", 0.0, -1.0, "deterministic"),
    (128, 2, "child_langmuir", 0.0, -1.0, "float"),
    (257, 1, "ccube", 0.0, 0.5, "deterministic"),
    (90, 3, "ivory", 0.0, -1.0, "deterministic"),
    (85, 3, "child_langmuir", 1.0, -1.0, "float"),
    (257, 1, "ivory", 1.0, 0.5, "float"),
    (640, 3, "ccube", 0.5, -1.0, "deterministic"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s-thresh%g-qm%g-%s" % c)
def test_emission_on_unequal_cells(V, case):
    """faces of all six orientations in cells on the domain's surface and inside, volume codes, fields of the wrong sign
    and below the threshold, slot counts around the launch block (255, 256, 257, 270) and beyond, the three laws"""
    n_comp, n_emit, law, thresh, q_m, mode = case
    fi, comps = world(64 + n_comp, n_comp)                             # (a seed at which every case below meets its own conditions)
    draws = slot_draws(62, n_comp * n_emit)
    what = "%d components x %d, %s, thresh %g, q_m %g, %s" % case
    inj, nm = run_emit(V, DIMS, BOX, WALLS, fi, comps, n_emit, UT_PERP, UT_PARA, q_m, S.COEF[law], thresh, draws, mode, what)
    og = pyorc.make_grid(*DIMS, *BOX[:3], np.float32(BOX[3]), pbc=WALLS)
    emits, cell, axis, dirn, en = S._emit_common(og, fi, comps, n_emit, q_m, thresh)
    valid = axis >= 0
    assert 0 < emits.sum() == len(inj) < valid.sum() < len(emits)              # some emit, some pull the wrong way, some are volumes
    assert {int(a) * 2 + int(d > 0) for a, d in zip(axis[emits], dirn[emits])} == set(range(6))     # every orientation emits
    if thresh > 0:
        assert np.any(valid & (np.float32(q_m) * (dirn * en) > 0) & (np.abs(en) < thresh))          # ... and some are too weak
    x = cell[emits] % (DIMS[0] + 2)
    assert np.any(x == 1) and np.any(x == DIMS[0]) and np.any((x > 1) & (x < DIMS[0]))              # surface cells and inner ones


@pytest.mark.parametrize("mode", ["deterministic", "float"])
def test_emission_into_a_species_in_tile_order_that_then_fits_exactly(V, mode):
    fi, comps = world(71, 200)
    run_emit(V, DIMS, BOX, WALLS, fi, comps, 3, UT_PERP, UT_PARA, -1.0, S.COEF["child_langmuir"], 0.0, slot_draws(72, 600), mode,
             "tile order, fits exactly, " + mode, resident=4000, fits_exactly=True)


@pytest.mark.parametrize("mode", ["deterministic", "float"])
def test_the_scale_follows_the_emitted_charges(V, mode):
    """deterministic accumulation without a reference charge on a species that holds nothing but emitted particles: in the
    emission the scale comes from the largest charge among the injectors; after an emission in float mode the push's scale
    comes from Species::q_max, which has to have learnt the largest emitted |q| (or the engine knows no charge at all)"""
    fi, comps = world(81, 120)
    run_emit(V, DIMS, BOX, WALLS, fi, comps, 2, UT_PERP, UT_PARA, -1.0, S.COEF["child_langmuir"], 0.0, slot_draws(82, 240), mode,
             "no reference charge, " + mode, learn_scale=True)


# ---- emission into a species with dead slots ---------------------------------------------------------------------------------
def live(e, sp):
    """(the live particles, their slots in the species' array): a plain download of a species with dead slots would compact
    it first"""
    r = e.select(sp, index=True)
    assert r.count == e.np(sp) == len(r.particles)
    return r.particles, np.asarray(r.index, np.int64)


def rows_of(slots, wanted):
    """the rows of the live download that hold the array slots `wanted` (all of them must be live)"""
    o = np.argsort(slots)
    at = np.searchsorted(slots[o], wanted)
    assert np.all(at < len(slots)) and np.array_equal(slots[o][np.minimum(at, len(slots) - 1)], wanted), "a mover names a slot that holds no live particle"
    return o[at]


@pytest.mark.parametrize("mode", ["deterministic", "float"])
def test_emission_into_a_species_with_dead_slots(V, mode):
    """The tile_tail_holes state of species_states.py: tile order, an appended tail, and N_DOOMED dead slots left by one step
    of the resident exchange.  The emitted particles are appended behind the array's extent -- not into a dead slot, not
    over a live particle --, the live particles from before stay where they are, the dead slots stay dead; then one
    advance_p over the live particles, the dead slots and the new tail, against the oracle's push of the live particles."""
    from species_states import N_DOOMED, N_TAIL, build_state
    dims, dt, q_m, q_ref, n_emit = (10, 9, 7), 0.4, -1.0, 0.05, 3
    what = "dead slots, " + mode
    # (cold and away from the x faces: the state's one step removes the N_DOOMED particles placed for it and no other)
    p = D.particles(91, 6000, dims, D.COLD)
    tail = D.particles(92, N_TAIL, dims, D.COLD, first_tag=10 ** 6)
    for q in (p, tail):
        q["dx"] = np.clip(q["dx"], -0.9, 0.9)
    e, sp = build_state(V, "tile_tail_holes", p, dims, tail, dt, 0.9)
    assert e.species_stats(sp)["dead_slots"] == N_DOOMED and e.species_order(sp) == "tile"
    kw = dict(pbc=[S.ABSORB, 0, 0, S.ABSORB, 0, 0])
    og = pyorc.make_grid(*dims, *[float(v) for v in dims], np.float32(dt), **kw)
    scale = pyorc.fixed_scale(q_ref)
    if mode == "deterministic":
        e.set_accumulation("deterministic", q_ref)
    fi, comps = world(93, 200, dims=dims)
    draws = slot_draws(94, len(comps) * n_emit)
    e.set_interpolator(fi)
    e.set_emit_draws(draws)
    inj, left = S.emit_restatement(og, fi, comps, n_emit, UT_PERP, UT_PARA, q_m, S.COEF["child_langmuir"], 0.0, draws)
    assert len(inj) > 100
    before, slots_b = live(e, sp)
    extent = e.capacity(sp)[0]
    assert extent == len(before) + N_DOOMED
    f_before = e.get_fields()
    e.clear_accumulators()
    e.emit(sp, comps, n_emit, UT_PERP, UT_PARA)
    after, slots_a = live(e, sp)
    pm, acc, f_after = e.get_movers(sp), e.get_accumulator(), e.get_fields()
    assert e.species_stats(sp)["dead_slots"] == N_DOOMED, what + ": the dead slots changed"
    assert len(after) == len(before) + len(inj), what + ": %d live particles, expected %d" % (len(after), len(before) + len(inj))
    assert e.capacity(sp)[0] == extent + len(inj), what + ": the extent is not the old one plus the emitted particles"
    old = rows_of(slots_a, slots_b)
    assert bits_equal(after[old], before), what + ": a live particle from before changed or moved"
    new = np.ones(len(after), bool)
    new[old] = False
    assert np.all(slots_a[new] >= extent), what + ": an emitted particle was put below the old extent"
    assert np.all(after["tag"][new] == 0) and np.all(after["tag2"][new] == 0)
    ref = np.zeros(len(inj), L.particle_t)
    rpm = np.zeros(len(inj) + 1, L.particle_mover_t)
    a = np.zeros(og.nv + 1, L.accumulator_t)
    with pyorc.fixed_accumulator(og, scale) as (a64, streaks):
        new_np, nm = pyorc.boundary_p_inject(ref, 0, rpm, 0, inj, a, og)
    gt, rt = rec_sorted(after[new]), rec_sorted(ref)
    if not bits_equal(gt, rt):
        bad = [k for k in range(len(gt)) if not bits_equal(gt[k:k + 1], rt[k:k + 1])]
        raise AssertionError(what + ": %d of %d emitted particles differ; first: got %s, restatement %s" % (len(bad), len(gt), gt[bad[0]], rt[bad[0]]))
    got_pm = pm.copy()
    got_pm["i"] = rows_of(slots_a, pm["i"].astype(np.int64))
    same_movers(after, got_pm, ref, rpm[:nm], what)
    bad = S.describe_rhob(f_after["rhob"], f_before["rhob"], left, og)
    assert bad is None, what + ": " + bad
    check_accumulator(acc, a, a64, streaks, scale, og, mode, what)
    # the movers leave through the absorbing walls (the host-count round compacts nothing it should not), then one push
    if e.nm(sp):
        e.boundary_p_pack()
        assert e.nm(sp) == 0
    p1, _ = live(e, sp)
    assert len(p1) == len(after) - nm
    e.clear_accumulators()
    e.advance_p(sp)
    r = D.Pushed(og, p1, fi, scale, q_m)
    got, slots = live(e, sp)
    w = what + ", the push after the emission"
    assert len(got) == len(r.p) and bits_equal(rec_sorted(got), rec_sorted(r.p)), w + ": particles differ from the oracle's"
    got_pm = e.get_movers(sp)
    got_pm["i"] = rows_of(slots, got_pm["i"].astype(np.int64))
    same_movers(got, got_pm, r.p, r.pm, w)
    check_accumulator(e.get_accumulator(), r.a, r.a64, r.streaks, scale, og, mode, w)
    e.close()
