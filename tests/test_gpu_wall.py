"""Absorbing walls that tally and record what they take (vpic_hip_wall_*), on the device, against tests/wall_ref.py (GPU box only).

Driven as tests/test_gpu_reflux.py drives its cases: one advance_p of seeded hot particles, then boundary_p_pack() until no
species has movers; particles and movers are downloaded before each round and the round is predicted from that state.  What
test_gpu_reflux.py holds for a round is held again by its own one_round -- np and nm, survivors as a multiset, refluxed
particles and their draws, rhob within source_ref.rhob_bound, the rest of the field array untouched -- with the oracle's grid
carrying VPIC_ABSORB_PARTICLES in the walls' place.  On top of it, after every round:

  every word of the tally table        == wall_ref.tally of the movers wall_ref.absorbed_faces calls absorbed, cumulative over
                                       the rounds, again by a clearing read, and zero after it
  the records                          == wall_ref.records as a multiset of bytes (particle, both tags, face, species); those of
                                       an earlier round precede those of a later one; dropped == 0

Further: movers parked on two faces at once in every pairing of the wall kinds, a record buffer too small by 10, quanta that
refuse some particles, the device-resident exchange (exchange_ref.absorbing_world), eight whole steps, the error paths, and a
table that no wall feeds."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import exchange_ref as R  # noqa: E402
import source_ref as S  # noqa: E402
import wall_ref as W  # noqa: E402
import test_gpu_exchange as XT  # noqa: E402   (Dev, Msg, knobs: the engines of a reference world)
import test_gpu_reflux as RX  # noqa: E402     (make_engine, one_round, final_push: a round held to the oracle)
from source_ref import D, L, pyorc  # noqa: E402
from species_states import package, run_child  # noqa: E402

pytestmark = pytest.mark.gpu
ABSORB, REFLECT = W.ABSORB, W.REFLECT


@pytest.fixture(scope="module")
def V():
    return package()


# ---- what the walls must hold after a round ---------------------------------------------------------------------------------------
class Expect:
    """the table and the records the walls of an engine must hold: cumulative since the last clearing read"""

    def __init__(self, n_species, quanta=W.QUANTA):
        self.n_species, self.quanta = n_species, quanta
        self.table = np.zeros((W.ROWS, n_species), L.wall_tally_t)
        self.records = np.zeros(0, L.wall_record_t)

    def take(self, before, codes, walled, reflux=(), rank=0):
        """the movers of the state `before` ([(p, pm)] per species) that a round absorbs; returns the round's records"""
        this = []
        for s, (p, pm) in enumerate(before):
            faces = W.absorbed_faces(p, pm, codes, walled, reflux, rank)
            gone = faces >= 0
            rec = p[pm["i"][gone]]
            W.tally(rec, faces[gone], s, codes, walled, self.quanta, table=self.table)
            this.append(W.records(rec, faces[gone], s, codes, walled))
        return np.concatenate(this)


def table_of(t):
    out = np.zeros(t.count.shape, L.wall_tally_t)
    out["count"], out["refused"] = t.count, t.refused
    out["isum"][..., 0], out["isum"][..., 1] = t.isum_q, t.isum_qke
    return out


def check_walls(e, ex, this, what, dropped=0):
    """the engine's table is ex.table; its records are ex.records (earlier rounds) followed by `this`, as multisets"""
    t = e.wall_tally()
    got = table_of(t)
    assert W.same_table(got, ex.table), what + ": the tally differs: " + W.describe_table(got, ex.table)
    assert np.array_equal(t.sum_q, t.isum_q * ex.quanta[0]) and np.array_equal(t.sum_qke, t.isum_qke * ex.quanta[1]), what
    r = e.wall_records(clear=False)
    assert r.dropped == dropped, what + ": %d records dropped" % r.dropped
    n0 = len(ex.records)
    assert len(r.records) == n0 + len(this), what + ": %d records, %d predicted" % (len(r.records), n0 + len(this))
    assert W.same_records(r.records[:n0], ex.records), what + ": the records of the earlier rounds changed"
    assert W.same_records(r.records[n0:], this), what + ": the records of this round differ from the predicted ones"
    ex.records = np.concatenate([ex.records, this])


def check_clearing_read(e, ex, what):
    got = table_of(e.wall_tally(clear=True))
    assert W.same_table(got, ex.table), what + ": the clearing read differs: " + W.describe_table(got, ex.table)
    r = e.wall_records(clear=True)
    assert W.same_records(r.records, ex.records) and r.dropped == 0, what
    ex.table[...] = np.zeros((), L.wall_tally_t)
    ex.records = np.zeros(0, L.wall_record_t)
    got = table_of(e.wall_tally())
    assert W.same_table(got, ex.table), what + ": not zero after a clearing read: " + W.describe_table(got, ex.table)
    r = e.wall_records(clear=False)
    assert len(r.records) == 0 and r.dropped == 0, what


def set_walls(e, walled, cap, quanta=W.QUANTA):
    e.wall_setup(quanta[0], quanta[1], cap)
    for code, flags in sorted(walled.items()):
        e.set_wall(code, record=bool(flags & W.RECORD))


def wall_round(e, sps, og, codes, walled, handlers, draws, mode, what, ex):
    """one boundary_p_pack(): test_gpu_reflux's round, then the walls"""
    before = [(e.get_particles(sp), e.get_movers(sp)) for sp in sps]
    RX.one_round(e, sps, og, handlers, draws, mode, what)
    reflux = sorted(set(h[0] for hs in handlers for h in hs))
    this = ex.take(before, codes, walled, reflux)
    check_walls(e, ex, this, what)
    return before, this


# ---- the pushed cases -------------------------------------------------------------------------------------------------------------
def run_case(V, c, setenv):
    case = W.case_of(c)
    what = W.case_id(c)
    state, mode, codes, walled = case["state"], case["mode"], case["walls"], case["walled"]
    if state in S.TAIL_SORT_MIN:
        setenv("VPIC_HIP_TAIL_SORT_MIN", str(S.TAIL_SORT_MIN[state]))
    args, kw, og = W.grids(case)
    species = S.SPECIES[case["species"]]
    n = S.N_PARTICLES[case["dims"]]
    draws = S.draw_table(n + 64)
    e = RX.make_engine(V, args, kw, mode, "reference" if state == "voxel" else "engine",
                       S.HANDLERS[case["handlers"]] if case["handlers"] else {}, len(species), draws)
    set_walls(e, walled, len(species) * n)
    fi = D.interpolator(og)
    e.set_interpolator(fi)
    sps, ps = [], []
    for s, (q_m, _) in enumerate(species):
        p = S.species_particles(case, s)
        sp = e.new_species(q_m, n + 64, n + 64)
        assert sp == s
        if state in S.TAIL_SORT_MIN:
            e.set_particles(sp, p[:n - S.N_TAIL])
            e.sort_p(sp)
            assert e.species_order(sp) == "tile", what
            e.append_particles(sp, p[n - S.N_TAIL:])
        else:
            e.set_particles(sp, p)
            if state != "unsorted":
                e.sort_p(sp)
                assert e.species_order(sp) == ("voxel" if state in ("voxel", "thin") else "tile"), what
        if state in ("tile", "tile_only") + tuple(S.TAIL_SORT_MIN) and species[s][1] != 0:
            assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0), what
        sps.append(sp)
        ps.append(p)
    e.clear_accumulators()
    for s, sp in enumerate(sps):                       # the push (held exactly by test_gpu_det_exact.py; here the premise of the rounds)
        e.advance_p(sp)
        ref = D.Pushed(og, ps[s], fi, S.SCALE, species[s][0])
        assert RX.bits_equal(S.ordered(e.get_particles(sp)), S.ordered(ref.p)), what + ": the push differs from the oracle's"
        assert e.nm(sp) == ref.nm > 0, what
    ex = Expect(len(species))
    check_walls(e, ex, ex.records, what + ", before the first round")                 # the push itself tallies nothing
    handlers = [W.handlers_of(case, s) for s in range(len(species))]
    rounds = 0
    while any(e.nm(sp) for sp in sps):
        assert rounds < S.MAX_ROUNDS, what + ": movers left after %d rounds" % S.MAX_ROUNDS
        rounds += 1
        wall_round(e, sps, og, codes, walled, handlers, draws, mode, "%s, round %d" % (what, rounds), ex)
        if rounds == 1:
            for f in range(6):                                                           # (the coverage tests/test_wall_ref.py holds on the oracle)
                if codes[f] in walled:
                    assert np.all(ex.table["count"][f] >= 20), what
            for s in range(len(species)):
                if species[s][1] == 0:                                                   # a chargeless copy: counts, sums of exactly zero, records by tag
                    assert ex.table["count"][:, s].sum() > 0 and not ex.table["isum"][:, s].any() and not ex.table["refused"][:, s].any()
                    mine = ex.records[ex.records["sp"] == s]
                    got = e.wall_records(clear=False).records
                    got = got[got["sp"] == s]
                    assert np.all(mine["q"] == 0) and len(np.unique(mine["tag"])) == len(mine)
                    assert np.array_equal(np.sort(got["tag"]), np.sort(mine["tag"])), what
    assert int(ex.table["count"].sum()) == sum(len(p) for p in ps) - sum(e.np(sp) for sp in sps), what + ": the rows do not account for every absorption"
    check_clearing_read(e, ex, what)
    RX.final_push(e, sps, og, fi, [q for q, _ in species], mode, what)
    check_walls(e, ex, ex.records, what + ", after one more push")
    e.close()


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_pushed_rounds(V, c, monkeypatch):
    if W.case_of(c)["state"] == "tile_only":
        run_child(__file__, ["tile_only", W.CASES.index(c)], 120)
    else:
        run_case(V, c, monkeypatch.setenv)


# ---- parked movers ----------------------------------------------------------------------------------------------------------------
def parked(V, codes, walled, reflux, p, pm, mode="deterministic", cap=None, quanta=W.QUANTA, record_cap=4096):
    """(engine, species, the oracle's grid, draws, handlers of the species) with p and pm uploaded and the walls registered"""
    e, sp, _, draws = RX.parked_engine(V, codes, mode, p, pm, handlers={-3: [(0.11, 0.04)]} if reflux else {}, cap=cap)
    _, _, og = D.grids(S.PARKED_DIMS, W.oracle_codes(codes, walled))
    if walled is not None:
        set_walls(e, walled, record_cap, quanta)
    return e, sp, og, draws, (W.PARKED_HANDLERS if reflux else [])


def parked_rounds(e, sp, og, codes, walled, h, draws, mode, what, ex):
    rounds = 0
    while e.nm(sp):
        assert rounds < S.MAX_ROUNDS, what
        rounds += 1
        wall_round(e, [sp], og, codes, walled, [h], draws, mode, "%s, round %d" % (what, rounds), ex)
    return rounds


@pytest.mark.parametrize("first,second,codes,walled,reflux", W.parked_pairings(), ids=lambda v: v if isinstance(v, str) else "")
def test_parked_on_two_faces_at_once(V, first, second, codes, walled, reflux):
    """movers on the faces -x and -y at once: the first face in order that takes, takes -- a wall after a face that passes the
    mover on tallies in its own row, a wall behind a face that took it sees nothing"""
    p, pm = S.parked_on((0, 1), 8, S.PARKED_DIMS, 17, n_rest=40)
    e, sp, og, draws, h = parked(V, codes, walled, reflux, p, pm)
    ex = Expect(1)
    if not walled:                                                                  # no wall in this pairing: nothing is tallied, row 6 included
        while e.nm(sp):
            RX.one_round(e, [sp], og, [h], draws, "deterministic", "parked %s then %s" % (first, second))
        check_walls(e, ex, ex.records, "parked %s then %s" % (first, second))
    else:
        assert parked_rounds(e, sp, og, codes, walled, h, draws, "deterministic", "parked %s then %s" % (first, second), ex) >= 1
        takes = lambda kind: kind in ("wall_record", "wall", "absorb", "reflux")
        if not (first == "reflux" or (second == "reflux" and not takes(first))):
            assert ex.table["count"].sum() >= len(pm)                                   # (a refluxed mover may be absorbed in a later round)
    e.close()


@pytest.mark.parametrize("nm", [1, 63, 64, 65, 255, 256, 257])
def test_parked_mover_counts(V, nm):
    """one mover; a wavefront of the classifying kernel less one, exactly, plus one; the same for a workgroup.  The movers
    sit on three faces in turn (walls that record, tally only, and a plain absorbing face): a wavefront holds several rows."""
    codes, walled = [-3, -4, ABSORB, REFLECT, REFLECT, REFLECT], {-3: W.TALLY, -4: W.TALLY | W.RECORD}
    parts = [S.parked_on((f,), (nm + 2 - f) // 3, S.PARKED_DIMS, 18 + f, n_rest=100, first=1000 * f) for f in range(3)]
    ps = [x[0] for x in parts if len(x[1])]
    off = np.cumsum([0] + [len(x) for x in ps])
    p = np.concatenate(ps)
    pm = np.concatenate([x[1] for x in parts if len(x[1])])
    pm["i"] += np.repeat(off[:-1], [len(x[1]) for x in parts if len(x[1])])
    o = np.random.default_rng(nm).permutation(len(p))                                   # the faces mixed within a wavefront:
    new_place = np.empty(len(p), np.int64)                                             # the particles shuffled, the movers' list ascending
    new_place[o] = np.arange(len(p))
    p = np.ascontiguousarray(p[o])
    pm["i"] = new_place[pm["i"]]
    pm = np.ascontiguousarray(pm[np.argsort(pm["i"])])
    assert len(pm) == nm and len(np.unique(p["q"])) == len(p)
    p["tag"], p["tag2"] = np.arange(len(p)) + 1, -np.arange(len(p)) - 7
    e, sp, og, draws, h = parked(V, codes, walled, False, p, pm)
    ex = Expect(1)
    assert parked_rounds(e, sp, og, codes, walled, h, draws, "deterministic", "nm = %d" % nm, ex) == 1
    assert ex.table["count"].sum() == nm
    e.close()


def test_small_record_buffer(V):
    """a record_cap 10 below the predicted count: exactly cap records come back, each one of the predicted and no two the
    same; dropped is the difference; the tallies are unaffected; after a clearing read the cursor restarts"""
    codes, walled = [-3, -4, ABSORB, -3, -4, ABSORB], W.LAYOUTS["wall6"]["walled"]
    p, pm = S.parked_on((1,), 300, S.PARKED_DIMS, 31, n_rest=200)
    p["tag"] = np.arange(len(p)) + 1
    ex = Expect(1)
    want = ex.take([(p, pm)], codes, walled)
    assert len(want) == 300
    cap = len(want) - 10
    e, sp, og, draws, h = parked(V, codes, walled, False, p, pm, record_cap=cap)
    RX.one_round(e, [sp], og, [h], draws, "deterministic", "small buffer")
    got = table_of(e.wall_tally())
    assert W.same_table(got, ex.table), W.describe_table(got, ex.table)
    r = e.wall_records(clear=False)
    assert len(r.records) == cap and r.dropped == 10
    assert R.sub_multiset(r.records, want, W.R_WORDS) and R.all_different(r.records, W.R_WORDS)
    few = e.wall_records(clear=False, cap=7)                                           # a caller's buffer smaller than the device's
    assert len(few.records) == 7 and few.dropped == 10 and W.same_records(few.records, r.records[:7])
    again = e.wall_records(clear=True)
    assert W.same_records(again.records, r.records) and again.dropped == 10
    p2, pm2 = S.parked_on((4,), 7, S.PARKED_DIMS, 32, n_rest=50)
    e.set_particles(sp, p2)
    e.set_movers(sp, pm2)
    want2 = ex.take([(p2, pm2)], codes, walled)
    RX.one_round(e, [sp], og, [h], draws, "deterministic", "after the clearing read")
    r = e.wall_records(clear=False)
    assert r.dropped == 0 and len(want2) == 7 and W.same_records(r.records, want2)
    got = table_of(e.wall_tally())
    assert W.same_table(got, ex.table), W.describe_table(got, ex.table)              # (the tallies were not cleared: both rounds)
    e.close()


def test_refused_sums(V):
    """the quanta of the CPU test: refused is == the prediction, strictly between 0 and count; the counts are those of
    quanta that refuse nothing"""
    c = W.CASES[0]
    case = W.case_of(c)
    args, kw, og = W.grids(case)
    n = S.N_PARTICLES[case["dims"]]
    e = RX.make_engine(V, args, kw, "float", "engine", {}, 1, None)
    set_walls(e, case["walled"], n, W.REFUSING_QUANTA)
    fi = D.interpolator(og)
    e.set_interpolator(fi)
    sp = e.new_species(-1.0, n + 64, n + 64)
    e.set_particles(sp, S.species_particles(case, 0))
    e.sort_p(sp)
    e.clear_accumulators()
    e.advance_p(sp)
    ex = Expect(1, W.REFUSING_QUANTA)
    wall_round(e, [sp], og, case["walls"], case["walled"], [[]], S.draw_table(n + 64), "float", "refusing quanta", ex)
    for j in range(2):
        refused, count = int(ex.table["refused"][:, 0, j].sum()), int(ex.table["count"][:, 0].sum())
        assert 0 < refused < count, (j, refused, count)
    e.close()


# ---- the device-resident exchange ------------------------------------------------------------------------------------------------
RESIDENT_WALLED = {ABSORB: W.TALLY | W.RECORD}


@pytest.mark.parametrize("dims", R.GRIDS, ids=["%dx%dx%d" % d for d in R.GRIDS])
@pytest.mark.parametrize("order", XT.ORDERS)
def test_resident_path(V, dims, order):
    """exchange_ref.absorbing_world with VPIC_ABSORB_PARTICLES registered with records: tallies and records are the prediction
    from the world's state; dead slots, messages and rhob as test_gpu_exchange.test_absorbing_faces holds them"""
    w = R.absorbing_world(dims)
    with XT.knobs(order), XT.Dev(V, w, order) as dev:
        e, d = dev.engines[0], w.domains[0]
        set_walls(e, RESIDENT_WALLED, 4 * R.N_HOT)
        nm = w.push(0, 0)
        s = d.species[0]
        p, pm = s["p"][:s["np"]].copy(), s["pm"][:nm].copy()
        ex = Expect(1)
        want = ex.take([(p, pm)], d.pbc, RESIDENT_WALLED, rank=0)
        faces = W.absorbed_faces(p, pm, d.pbc, RESIDENT_WALLED, rank=0)
        assert np.array_equal(faces >= 0, np.array([f < 0 or d.pbc[f] == ABSORB for f in R.faces_of_movers(d, 0)]))
        assert all(ex.table["count"][f, 0] > 0 for f in (0, 2, 5)) and ex.table["count"][[1, 3, 4], 0].sum() == 0
        nodes, addends = R.absorbed_addends(d, 0)
        sent = w.pack(0)
        assert len(nodes) >= 64 and len(sent[3]) > 0 and int(ex.table["count"].sum()) == len(nodes) >= len(want) > 0
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        msgs = dev.pack(0, [len(x) + 8 for x in sent])
        e.exchange_finish([msgs[3].ptr])
        assert e.exchange_flags == 0 and e.nm(0) == 0
        for f in (0, 1, 2, 4, 5):
            assert msgs[f].untouched(), f
        msgs[3].check(len(sent[3]), len(sent[3]), sent[3], "absorbing")
        assert e.species_stats(0)["dead_slots"] == nm and e.np(0) == d.species[0]["np"]
        got, _ = dev.live(0, 0)
        assert R.same_multiset(got, d.live(0), R.P_TAGGED)
        exact, bound = R.rhob_bound(d.og.nv, nodes, addends)
        rhob = e.get_fields()["rhob"].astype(np.float64)
        assert np.all(np.abs(rhob - exact) <= bound)
        assert np.all(rhob[bound == 0] == exact[bound == 0])
        check_walls(e, ex, want, "resident %s %s" % (dims, order))
        check_clearing_read(e, ex, "resident %s %s" % (dims, order))


def test_resident_path_still_refuses_reflux(V):
    w = R.absorbing_world((4, 4, 4))
    with XT.Dev(V, w, "voxel") as dev:
        e = dev.engines[0]
        set_walls(e, RESIDENT_WALLED, 16)
        ut = np.full(32, 0.1, np.float32)
        e.set_maxwellian_reflux(-3, ut, ut)
        e.exchange_begin()
        with pytest.raises(V.VpicHipError, match="custom particle boundary handlers"):
            e.exchange_pack([0] * 6, [0] * 6, 64)


# ---- whole steps ------------------------------------------------------------------------------------------------------------------
def test_eight_steps(V):
    """Eight Engine.step() calls on 10x9x7, the x faces walled with records, y and z periodic, two tagged species with
    q_m = 0 and distinct charges: fields never act and momenta never change.  The tags missing at the end are exactly the
    records' tags, the tallies are the rule applied to the initial records of those tags, and the counts add up to the
    particles lost."""
    dims, n = (10, 9, 7), 4000
    codes, walled = [-3, 0, 0, -3, 0, 0], {-3: W.TALLY | W.RECORD}
    args, kw, og = D.grids(dims, codes)
    e = V.Engine(V.make_grid(*args, **kw))
    e.set_vacuum()
    e.set_sort_order("engine")
    set_walls(e, walled, 2 * n)
    ps = []
    for s, q0 in enumerate((-D.Q0, 2.5 * D.Q0)):
        p = D.particles(51 + s, n, dims, 0.6, q0=q0, first_tag=1 + s * 10 ** 6)
        sp = e.new_species(0.0, n + 64, n + 64)
        e.set_particles(sp, p)
        ps.append(p)
    e.load_interpolator()
    for step in range(8):
        e.step(step, 4)
    r = e.wall_records(clear=False)
    assert r.dropped == 0
    t = table_of(e.wall_tally())
    ex = Expect(2)
    lost = 0
    for s, p in enumerate(ps):
        left = e.get_particles(s)
        missing = np.setdiff1d(p["tag"], left["tag"])
        mine = r.records[r.records["sp"] == s]
        assert len(missing) > 100 and np.array_equal(np.sort(mine["tag"]), missing), s
        by_tag = p[np.argsort(p["tag"])]
        first = by_tag[np.searchsorted(by_tag["tag"], missing)]
        faces = np.where(first["ux"] < 0, 0, 3)
        W.tally(first, faces, s, codes, walled, W.QUANTA, table=ex.table)
        # a record holds the particle as it was stored when it was absorbed: on its wall, with the momenta and charge it began with
        mine = mine[np.argsort(mine["tag"])]
        for c in ("ux", "uy", "uz", "q"):
            assert RX.bits_equal(mine[c], first[c]), (s, c)
        assert np.array_equal(mine["face"], faces) and np.all(mine["dx"] == np.where(faces == 0, -1, 1))
        lost += len(p) - len(left)
    assert W.same_table(t, ex.table), W.describe_table(t, ex.table)
    assert int(t["count"].sum()) == lost == len(r.records)
    e.close()


# ---- host paths -------------------------------------------------------------------------------------------------------------------
def test_error_paths_are_refused_and_change_nothing(V):
    import ctypes as C
    args, kw, og = D.grids(S.PARKED_DIMS, [-3, -4, ABSORB, -3, -4, ABSORB])
    e = V.Engine(V.make_grid(*args, **kw))
    bad = lambda: pytest.raises(V.VpicHipError)
    raw, h = e._l, e._h
    n, dr = C.c_int64(0), C.c_int64(0)
    t1 = np.zeros((W.ROWS, 1), L.wall_tally_t)
    with bad():
        e.set_wall(-3)                                                              # before wall_setup
    with bad():
        e.wall_tally()
    with bad():
        e.wall_records()
    for q, qke, cap in ((0.0, 1.0, 0), (1.0, -1.0, 0), (float("nan"), 1.0, 0), (1.0, float("inf"), 0), (1.0, 1.0, -1)):
        with bad():
            e.wall_setup(q, qke, cap)
    with bad():
        e.set_wall(-3)                                                              # a refused setup is no setup
    sp = e.new_species(-1.0, 1024, 1024)
    e.wall_setup(W.QUANTA[0], W.QUANTA[1], 128)
    ut = np.full(32, 0.1, np.float32)
    e.set_maxwellian_reflux(-7, ut, ut)
    for code in (0, -1, 1, 5):
        with bad():
            e.set_wall(code)
    with bad():
        e.set_wall(-7)                                                              # a reflux handler
    assert raw.vpic_hip_set_wall(h, -3, 4) != 0                                      # unknown flag bits
    for code in (-3, -4, ABSORB, -5):
        e.set_wall(code, record=code == -4)
    e.set_wall(-5, record=True)                                                     # the same code again: replaced, not a fifth
    with bad():
        e.set_wall(-6)                                                              # a fifth code
    with bad():
        e.set_maxwellian_reflux(-3, ut, ut)                                         # a wall cannot become a reflux handler
    e.set_wall(-5, tally=False)                                                     # unregistered: there is room again
    e.set_wall(-6)
    e.set_wall(-6, tally=False)
    e.set_wall(-9, tally=False)                                                     # unregistering what is no wall is no error
    assert raw.vpic_hip_wall_tally(h, None, 1, 0) != 0
    assert raw.vpic_hip_wall_tally(h, t1.ctypes.data_as(C.c_void_p), 0, 0) != 0      # fewer columns than species
    assert raw.vpic_hip_wall_records(h, None, 4, C.byref(n), C.byref(dr), 0) != 0
    assert raw.vpic_hip_wall_records(h, t1.ctypes.data_as(C.c_void_p), -1, C.byref(n), C.byref(dr), 0) != 0
    assert raw.vpic_hip_wall_records(h, t1.ctypes.data_as(C.c_void_p), 1, None, C.byref(dr), 0) != 0
    assert raw.vpic_hip_wall_records(h, t1.ctypes.data_as(C.c_void_p), 1, C.byref(n), None, 0) != 0
    assert e._l.vpic_hip_last_error()
    # more columns than species: the ones beyond are zero
    wide = np.zeros((W.ROWS, 40), L.wall_tally_t)
    wide["count"] = -1
    assert raw.vpic_hip_wall_tally(h, wide.ctypes.data_as(C.c_void_p), 40, 0) == 0 and not wide["count"].any()
    # the state is what the accepted calls left: -3 tally, -4 record, ABSORB tally -- a round is the prediction's
    walled = {-3: W.TALLY, -4: W.TALLY | W.RECORD, ABSORB: W.TALLY}
    e.set_vacuum()
    e.set_interpolator(D.interpolator(og))
    p, pm = S.parked_on((1,), 70, S.PARKED_DIMS, 41, n_rest=30)
    e.set_particles(sp, p)
    e.set_movers(sp, pm)
    ex = Expect(1)
    want = ex.take([(p, pm)], [-3, -4, ABSORB, -3, -4, ABSORB], walled)
    e.boundary_p_pack()
    check_walls(e, ex, want, "after the refused calls")
    assert len(want) == 70
    e.close()


def test_no_walls(V):
    """wall_setup without any set_wall: a full absorbing case leaves every tally zero and no record"""
    codes = [ABSORB] * 6
    p, pm = S.parked_on((3,), 200, S.PARKED_DIMS, 43, n_rest=100)
    e, sp, og, draws, h = parked(V, codes, {}, False, p, pm)
    ex = Expect(1)
    RX.one_round(e, [sp], og, [h], draws, "deterministic", "no walls")
    assert e.np(sp) == 100
    check_walls(e, ex, ex.records, "no walls")
    e.set_wall(ABSORB)                                                              # ... and registered, the same movers are tallied
    e.set_particles(sp, p)
    e.set_movers(sp, pm)
    want = ex.take([(p, pm)], codes, {ABSORB: W.TALLY})
    RX.one_round(e, [sp], og, [h], draws, "deterministic", "registered afterwards")
    check_walls(e, ex, want, "registered afterwards")
    assert ex.table["count"][3, 0] == 200
    e.close()


if __name__ == "__main__":                                          # the fresh child of the tile_only cases (run_child)
    assert sys.argv[1] == "tile_only" and os.environ.get("VPIC_HIP_TILE_COARSE") == "1"
    run_case(package(), W.CASES[int(sys.argv[2])], os.environ.__setitem__)
    print("child OK")
