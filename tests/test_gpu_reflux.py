"""Maxwellian reflux walls on the device against the oracle, record by record (GPU box only).

One advance_p of seeded hot particles, then rounds of boundary_p_pack() until no species has movers.  Before each round
the particles and movers of every species are downloaded; the oracle's orc_boundary_p_reflux_round -- pinned on the
reference's own boundary_p by tests/test_oracle_golden.py -- predicts the round from that state (tests/source_ref.py), so
the array order is the device's and nothing depends on the order of a back-fill.  The device's logf is not the host's:
the magnitude of each refluxed particle's new normal momentum is read from the particle it became (found by its charge),
held within 4 float ulps of ut_para * sqrt(2) * sqrt(-log(d)) in float64, and handed to the oracle; everything downstream
of that one number is exact float arithmetic, so every other comparison is `==`:

  refluxed particles after their move (cell, dx dy dz, momenta, q; tag == tag2 == 0)   bit-equal, found by q
  particles that were not movers                                                      bit-equal, the same multiset below the new np
  np and nm of every species                                                          equal
  the movers left for the next round                                                  the same particles by q, displacements bit-equal
  accumulator of the round, deterministic mode                                        all 12 words of every voxel as uint32
  accumulator of the round, float mode                                                ACC_TOL of test_gpu_kernels.py
  rhob                                                                                per node within the bound of source_ref.rhob_bound;
                                                                                      bit-equal where a node has at most two terms
  every other component of the field array                                            untouched

The accumulator is cleared before every round: in deterministic mode a download rounds the sums so far into the float words.
After the last round one more advance_p runs on the device and on the oracle from the downloaded particles: particles
bit-equal by q, movers too, the accumulator exact in deterministic mode -- the species' bookkeeping after a refluxing round
(tile ranges, back-filled slots, the appended tail, partition_valid, hist_valid).

A chargeless copy of a species (q == 0: the chargeless instance of the push, injectors that deposit nothing) has no charge
to be found by: its particles are found by their tags and its refluxed ones by their two tangential momenta, ut_perp * draw,
which are the same bits on both sides (source_ref.match_refluxed).  The emitter (vpic_hip_emit) is held by tests/test_gpu_emit.py."""
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
from species_states import package, run_child  # noqa: E402

pytestmark = pytest.mark.gpu
ACC_TOL = 2e-6                                   # test_gpu_kernels.py: |a_hip - a_ref| <= ACC_TOL * max|a_ref|
WORST = {"ulps": 0.0}                            # the worst normal-momentum error seen in this session, in float ulps


@pytest.fixture(scope="module")
def V():
    return package()


def same_disp(a, b):
    return all(bits_equal(a[c], b[c]) for c in ("dispx", "dispy", "dispz"))


def make_engine(V, og_args, kw, mode, order, handlers, n_species, draws):
    """(engine with the random interpolator loaded, that interpolator); handlers: {code: [(ut_para, ut_perp) per species]}"""
    e = V.Engine(V.make_grid(*og_args, **kw))
    e.set_vacuum()
    if mode == "deterministic":
        e.set_accumulation("deterministic", D.Q0)
    e.set_sort_order(order)
    register(e, handlers, n_species)
    if draws is not None:
        e.set_reflux_draws(draws)
    return e


def register(e, handlers, n_species):
    for code, ut in sorted(handlers.items(), reverse=True):
        para, perp = np.zeros(32, np.float32), np.zeros(32, np.float32)
        for s in range(n_species):
            para[s], perp[s] = ut[s]
        e.set_maxwellian_reflux(code, para, perp, seed=1)


def one_round(e, sps, og, handlers, draws, mode, what):
    """One boundary_p_pack() of the engine against the oracle's prediction from the state before it.  handlers[s]: the
    (code, ut_para, ut_perp) list of species s.  Returns the particles of every species after the round."""
    before = [(e.get_particles(sp), e.get_movers(sp)) for sp in sps]
    f_before = e.get_fields()
    e.clear_accumulators()
    e.boundary_p_pack()
    after = [e.get_particles(sp) for sp in sps]
    f_after, acc = e.get_fields(), e.get_accumulator()
    f = np.zeros(og.nv, L.field_t)
    f["rhob"] = f_before["rhob"]
    a = np.zeros(og.nv + 1, L.accumulator_t)
    absorbed = []
    with pyorc.fixed_accumulator(og, S.SCALE) as (a64, streaks):
        for s, sp in enumerate(sps):
            (p, pm), got = before[s], after[s]
            w = "%s, species %d" % (what, s)
            assert len(np.unique(p)) == len(p), w + ": two particles are the same record"
            assert not np.any(p["q"] != 0) or len(np.unique(p["q"])) == len(p), w + ": charges are not distinct"
            r = S.predict_round(og, p, pm, sp, handlers[s], draws, f, a, after=got, fixed=(a64, streaks))
            absorbed.append(r.absorbed)
            # np and nm
            assert len(got) == len(r.p), w + ": np %d, the oracle has %d" % (len(got), len(r.p))
            assert e.nm(sp) == len(r.pm), w + ": nm %d, the oracle has %d" % (e.nm(sp), len(r.pm))
            # the new normal momenta: within NORMAL_ULPS of the float64 expression
            if len(r.ulps):
                WORST["ulps"] = max(WORST["ulps"], float(r.ulps.max()))
                k = int(np.argmax(r.ulps))
                assert r.ulps.max() <= S.NORMAL_ULPS, w + ": new normal momentum off by %.2f float ulps: %s" % (
                    r.ulps.max(), S.describe_mover(p, pm, r.who[k], r.face[k], og))
            # the new tangential momenta: one float product each (a reflecting wall met on the way only changes a sign)
            if len(r.inj):
                tail, inj, face, slot = got[r.n_keep:][r.match], r.inj, r.face, pm["i"][r.who]
                perp = np.array([dict((h[0], h[2]) for h in handlers[s])[og.pbc[fc]] for fc in face], np.float32)
                for j, col in ((1, 1), (2, 2)):
                    want = np.abs(perp * draws[slot, col])
                    comp = (face % 3 + j) % 3
                    have = np.abs(np.choose(comp, [tail["ux"], tail["uy"], tail["uz"]]))
                    assert bits_equal(have, want.astype(np.float32)), w + ": a tangential momentum is not ut_perp * draw"
                assert bits_equal(np.abs(np.choose(face % 3, [inj["ux"], inj["uy"], inj["uz"]])),
                                  np.abs(np.choose(face % 3, [tail["ux"], tail["uy"], tail["uz"]])))
            # survivors: the same multiset below the new np; refluxed particles: bit-equal, untagged
            assert bits_equal(S.ordered(got[:r.n_keep]), S.ordered(r.p[:r.n_keep])), w + ": particles that were not movers differ"
            assert np.all(got["tag"][r.n_keep:] == 0) and np.all(got["tag2"][r.n_keep:] == 0), w + ": a refluxed particle kept a tag"
            gt, rt = S.ordered(got[r.n_keep:]), S.ordered(r.p[r.n_keep:])
            if not bits_equal(gt, rt):
                bad = [k for k in range(len(gt)) if not bits_equal(gt[k:k + 1], rt[k:k + 1])]
                raise AssertionError(w + ": %d refluxed particles differ from the oracle's; first: got %s, oracle %s" % (len(bad), gt[bad[0]], rt[bad[0]]))
            # the movers left for the next round
            if len(r.pm):
                gq, gpm = S.movers_keyed(got, e.get_movers(sp))
                rq, rpm = S.movers_keyed(r.p, r.pm)
                assert bits_equal(gq, rq) and same_disp(gpm, rpm), w + ": the movers left differ from the oracle's"
    # accumulator of the round
    if mode == "deterministic":
        bad = D.describe_bad_words(acc, a64, streaks, S.SCALE, (og.nx, og.ny, og.nz))
        assert bad is None, what + "\n" + bad
    else:
        g = np.stack([acc[c] for c in ("jx", "jy", "jz")]).astype(np.float64)[:, :og.nv]
        w = np.stack([a[c] for c in ("jx", "jy", "jz")]).astype(np.float64)[:, :og.nv]
        assert np.abs(g - w).max() <= ACC_TOL * np.abs(w).max(), what + ": accumulator off by %.3g of %.3g" % (np.abs(g - w).max(), np.abs(w).max())
    # rhob, and nothing else of the fields
    gone = np.concatenate(absorbed)
    bad = S.describe_rhob(f_after["rhob"], f_before["rhob"], gone, og)
    assert bad is None, what + ": " + bad
    if len(gone) == 0:
        assert bits_equal(f_after["rhob"], f_before["rhob"]), what
    for name in f_after.dtype.names:
        if name != "rhob":
            assert bits_equal(f_after[name], f_before[name]), what + ": field component %s changed" % name
    return after


def final_push(e, sps, og, fi, q_ms, mode, what):
    """one more advance_p on the device and on the oracle from the downloaded particles"""
    ps = [e.get_particles(sp) for sp in sps]
    e.clear_accumulators()
    refs, a64, streaks = [], None, None
    for sp, p, q_m in zip(sps, ps, q_ms):
        assert e.nm(sp) == 0
        e.advance_p(sp)
        refs.append(D.Pushed(og, p, fi, S.SCALE, q_m, a64=a64, streaks=streaks))
        a64, streaks = refs[-1].a64, refs[-1].streaks
    if mode == "deterministic":
        bad = D.describe_bad_words(e.get_accumulator(), a64, streaks, S.SCALE, (og.nx, og.ny, og.nz))
        assert bad is None, what + ", the push after the rounds\n" + bad
    for s, (sp, r) in enumerate(zip(sps, refs)):
        got = e.get_particles(sp)
        w = "%s, species %d, the push after the rounds" % (what, s)
        assert len(got) == len(r.p) and bits_equal(S.ordered(got), S.ordered(r.p)), w + ": particles differ from the oracle's"
        assert e.nm(sp) == r.nm, w + ": %d movers, the oracle has %d" % (e.nm(sp), r.nm)
        if r.nm:
            gq, gpm = S.movers_keyed(got, e.get_movers(sp))
            rq, rpm = S.movers_keyed(r.p, r.pm)
            assert bits_equal(gq, rq) and same_disp(gpm, rpm), w + ": movers differ from the oracle's"


def run_case(V, c, setenv):
    case = S.case_of(c)
    what = S.case_id(c)
    state, mode = case["state"], case["mode"]
    if state in S.TAIL_SORT_MIN:
        setenv("VPIC_HIP_TAIL_SORT_MIN", str(S.TAIL_SORT_MIN[state]))
    args, kw, og = S.grids(case)
    species = S.SPECIES[case["species"]]
    n = S.N_PARTICLES[case["dims"]]
    draws = S.draw_table(n + 64)
    e = make_engine(V, args, kw, mode, "reference" if state == "voxel" else "engine", S.HANDLERS[case["handlers"]], len(species), draws)
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
        if state in ("tile", "tile_only") + tuple(S.TAIL_SORT_MIN) and species[s][1] != 0:   # (a chargeless species is sorted by tile only: it deposits nothing)
            assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0), what
        sps.append(sp)
        ps.append(p)
    # the push (held exactly by test_gpu_det_exact.py; here the premise of the rounds): particles and movers are the oracle's
    e.clear_accumulators()
    for s, sp in enumerate(sps):
        e.advance_p(sp)
        ref = D.Pushed(og, ps[s], fi, S.SCALE, species[s][0])
        got = e.get_particles(sp)
        assert bits_equal(S.ordered(got), S.ordered(ref.p)), what + ": the push differs from the oracle's"
        assert e.nm(sp) == ref.nm > 0, what
    handlers = [S.handlers_of(case, s) for s in range(len(species))]
    rounds = 0
    while any(e.nm(sp) for sp in sps):
        assert rounds < S.MAX_ROUNDS, what + ": movers left after %d rounds" % S.MAX_ROUNDS
        rounds += 1
        one_round(e, sps, og, handlers, draws, mode, "%s, round %d" % (what, rounds))
    if case["dims"] == (1, 6, 5):
        assert rounds >= 3, what
    final_push(e, sps, og, fi, [q for q, _ in species], mode, what)
    print("%s: %d rounds, worst normal momentum error so far %.2f float ulps" % (what, rounds, WORST["ulps"]))
    e.close()


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_pushed_rounds(V, c, monkeypatch):
    if S.case_of(c)["state"] == "tile_only":
        run_child(__file__, ["tile_only", S.CASES.index(c)], 120)
    else:
        run_case(V, c, monkeypatch.setenv)


# ---- parked movers: what a push produces only by coincidence --------------------------------------------------------------------
def parked_engine(V, walls, mode, p, pm, handlers=None, draws=None, cap=None):
    args, kw, og = D.grids(S.PARKED_DIMS, walls)
    handlers = {-3: [(0.11, 0.04)]} if handlers is None else handlers
    draws = S.draw_table((cap or len(p)) + 64, seed=6) if draws is None else draws
    e = make_engine(V, args, kw, mode, "engine", handlers, 1, draws)
    e.set_interpolator(D.interpolator(og))
    sp = e.new_species(-1.0, (cap or len(p)) + 64, (cap or len(p)) + 64)
    e.set_particles(sp, p)
    e.set_movers(sp, pm)
    return e, sp, og, draws


def rounds_until_done(e, sp, og, handlers, draws, mode, what):
    rounds = 0
    while e.nm(sp):
        assert rounds < S.MAX_ROUNDS, what
        rounds += 1
        one_round(e, [sp], og, [handlers], draws, mode, "%s, round %d" % (what, rounds))
    return rounds


H1 = [(-3, np.float32(0.11), np.float32(0.04))]


@pytest.mark.parametrize("first,second,walls", S.parked_pairings(), ids=lambda v: v if isinstance(v, str) else "")
def test_parked_on_two_faces_at_once(V, first, second, walls):
    """movers on the faces -x and -y at once, every pairing of {registered handler, unregistered code, absorb, reflect, this
    same domain}: the reference tries the faces in order and falls through at a face nothing claims (boundary_p.c:268-277),
    so `unregistered` (or reflect, or this same domain) first and a registered handler second is a reflux at the second
    face, not an absorption"""
    p, pm = S.parked_on((0, 1), 8, S.PARKED_DIMS, 17, n_rest=40)
    e, sp, og, draws = parked_engine(V, walls, "deterministic", p, pm)
    rounds_until_done(e, sp, og, H1, draws, "deterministic", "parked %s then %s" % (first, second))
    e.close()


@pytest.mark.parametrize("nm", [1, 255, 256, 257])
def test_parked_mover_counts(V, nm):
    """one mover, and a workgroup of the classifying kernel less one, exactly, plus one"""
    p, pm = S.parked_on((3,), nm, S.PARKED_DIMS, 18, n_rest=300)
    e, sp, og, draws = parked_engine(V, S.WALLS["reflux_absorb_reflect"], "deterministic", p, pm)
    assert rounds_until_done(e, sp, og, H1, draws, "deterministic", "nm = %d" % nm) >= 1
    e.close()


@pytest.mark.parametrize("where", ["every_particle", "all_in_the_tail", "none_in_the_tail"])
def test_parked_movers_and_the_tail(V, where):
    """every particle of the species a mover (nm == np: nothing survives, nothing to back-fill with); every mover in the
    tail [np - nm, np) (no hole below the new np); none there (every hole is filled from the tail)"""
    n, nm = 600, 200
    if where == "every_particle":
        p, pm = S.parked_on((0,), n, S.PARKED_DIMS, 19)
    else:
        p, pm = S.parked_on((0,), nm, S.PARKED_DIMS, 19, n_rest=n - nm)
        mv = np.zeros(n, bool)
        mv[pm["i"]] = True
        order = np.concatenate([np.flatnonzero(~mv), np.flatnonzero(mv)] if where == "all_in_the_tail" else
                               [np.flatnonzero(mv), np.flatnonzero(~mv)])
        p = p[order]
        pm["i"] = np.arange(n - nm, n) if where == "all_in_the_tail" else np.arange(nm)
    e, sp, og, draws = parked_engine(V, S.WALLS["reflux_absorb_reflect"], "float", p, pm)
    assert rounds_until_done(e, sp, og, H1, draws, "float", where) >= 1
    e.close()


# ---- host paths ------------------------------------------------------------------------------------------------------------
def test_handler_registered_after_the_buffers_were_sized_then_more_movers_then_new_parameters(V):
    """A first boundary_p_pack with absorbing movers only sizes the send buffers while no handler exists (no local buffer);
    then a handler is registered (the local_buf branch of k_boundary_p_pack), then a round has more movers than the
    buffers were sized for, then the handler's parameters are replaced under the same code: every round is the oracle's."""
    walls = S.WALLS["reflux_absorb_reflect"]
    cap = 6000
    p, pm = S.parked_on((1,), 10, S.PARKED_DIMS, 20, n_rest=100)                    # face -y absorbs
    e, sp, og, draws = parked_engine(V, walls, "deterministic", p, pm, handlers={}, cap=cap)
    one_round(e, [sp], og, [[]], draws, "deterministic", "absorbing movers, no handler yet")
    assert e.np(sp) == 100 and e.nm(sp) == 0
    register(e, {-3: [(0.11, 0.04)]}, 1)
    p, pm = S.parked_on((0,), 40, S.PARKED_DIMS, 21, n_rest=100)
    e.set_particles(sp, p)
    e.set_movers(sp, pm)
    rounds_until_done(e, sp, og, H1, draws, "deterministic", "handler registered after the buffers were sized")
    p, pm = S.parked_on((3,), 3000, S.PARKED_DIMS, 22, n_rest=2000)                 # 10 + 10 / 4 + 1024 slots were sized
    e.set_particles(sp, p)
    e.set_movers(sp, pm)
    rounds_until_done(e, sp, og, H1, draws, "deterministic", "more movers than the buffers were sized for")
    register(e, {-3: [(0.5, 0.3)]}, 1)
    p, pm = S.parked_on((0,), 300, S.PARKED_DIMS, 23, n_rest=300)
    e.set_particles(sp, p)
    e.set_movers(sp, pm)
    rounds_until_done(e, sp, og, [(-3, np.float32(0.5), np.float32(0.3))], draws, "deterministic", "parameters replaced under the same code")
    e.close()


def test_bad_handler_arguments_are_refused_without_a_launch(V):
    import ctypes as C
    args, kw, og = D.grids(S.PARKED_DIMS, S.WALLS["reflux6"])
    e = V.Engine(V.make_grid(*args, **kw))
    ut = np.full(32, 0.1, np.float32)
    for code in (-3, -4, -5, -6):
        e.set_maxwellian_reflux(code, ut, ut)
    e.set_maxwellian_reflux(-4, 2 * ut, ut)                                        # the same code again: replaced, not a fifth
    with pytest.raises(V.VpicHipError):
        e.set_maxwellian_reflux(-7, ut, ut)                                        # a fifth code
    with pytest.raises(V.VpicHipError):
        e.set_maxwellian_reflux(-2, ut, ut)                                        # not a handler code
    raw, h, ptr = e._l.vpic_hip_set_maxwellian_reflux, e._h, ut.ctypes.data_as(C.c_void_p)
    big = np.full(33, 0.1, np.float32).ctypes.data_as(C.c_void_p)
    assert raw(h, -3, ptr, ptr, 0, 1) != 0 and raw(h, -3, big, big, 33, 1) != 0    # n_species of 0 and of 33
    assert raw(h, -3, None, ptr, 32, 1) != 0 and raw(h, -3, ptr, None, 32, 1) != 0  # null arrays
    e.close()


# ---- the engine's own generator (no draw table) ---------------------------------------------------------------------------
def test_own_generator_differs_by_species_call_mover_and_seed(V):
    """two species that hold identical particles get different momenta; so do two successive calls, two movers of one call,
    and another seed; every normal momentum points into the domain and none is zero"""
    def refluxed(seed, calls=1):
        p, pm = S.parked_on((0,), 64, S.PARKED_DIMS, 24, n_rest=36)
        args, kw, og = D.grids(S.PARKED_DIMS, S.WALLS["reflux6"])
        e = V.Engine(V.make_grid(*args, **kw))
        e.set_vacuum()
        e.set_interpolator(D.interpolator(og))
        ut = np.full(32, 0.2, np.float32)
        e.set_maxwellian_reflux(-3, ut, ut, seed=seed)
        sps = [e.new_species(-1.0, 256, 256) for _ in range(2)]
        out = []
        for _ in range(calls):
            for sp in sps:
                e.set_particles(sp, p)
                e.set_movers(sp, pm)
            e.clear_accumulators()
            e.boundary_p_pack()
            out.append([S.ordered(e.get_particles(sp)[len(p) - len(pm):]) for sp in sps])
        e.close()
        return out
    (a0, b0), (a1, b1) = refluxed(1, calls=2)
    (c0, _), = refluxed(2)
    for x in (a0, b0, a1, b1, c0):
        assert len(x) == 64 and np.all(x["ux"] > 0) and np.all(x["tag"] == 0)
        assert len(np.unique(x["ux"])) == 64 and len(np.unique(x["uy"])) == 64       # two movers of one call
    assert bits_equal(a0["q"], b0["q"]) and bits_equal(a0["q"], a1["q"]) and bits_equal(a0["q"], c0["q"])
    assert not np.any(a0["ux"] == b0["ux"])                                       # two species
    assert not np.any(a0["ux"] == a1["ux"])                                       # two calls
    assert not np.any(a0["ux"] == c0["ux"])                                       # two seeds


if __name__ == "__main__":                                          # the fresh child of the tile_only cases (run_child)
    assert sys.argv[1] == "tile_only" and os.environ.get("VPIC_HIP_TILE_COARSE") == "1"
    run_case(package(), S.CASES[int(sys.argv[2])], os.environ.__setitem__)
    print("child OK")
