"""The reference world of tests/test_gpu_reflux.py on the CPU alone (tests/source_ref.py): every case of the GPU test is run
on the oracle -- orc_advance_p, then rounds of orc_boundary_p_reflux_round with the oracle's own logf -- and must meet the
coverage conditions, so that no GPU case can pass by having nothing to check; the numpy restatement of accumulate_rhob and
its node bound are held to the oracle's C, which tests/test_oracle_golden.py pins on the reference."""
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


def test_the_cases_cover_every_grid_wall_layout_state_and_both_modes():
    cases = [S.case_of(c) for c in S.CASES]
    assert len(set(S.CASES)) == len(S.CASES) >= 24
    assert {c["dims"] for c in cases} == set(S.N_PARTICLES)
    assert {c["walls"] for c in cases} == set(S.WALLS)
    assert {c["handlers"] for c in cases} == set(S.HANDLERS)
    assert {c["species"] for c in cases} == set(S.SPECIES)
    assert {c["state"] for c in cases} == set(S.STATES)
    for dims in S.N_PARTICLES:
        assert {c["mode"] for c in cases if c["dims"] == dims} == {"deterministic", "float"}, dims
    for c in cases:
        assert (c["state"] == "thin") == (c["dims"] in S.THIN)
        codes = {w for w in S.WALLS[c["walls"]] if w <= -3}
        assert (codes - set(S.HANDLERS[c["handlers"]]) == {-5}) == (c["walls"] == "unregistered")
    assert S.TAIL_SORT_MIN["tail_below"] < S.N_TAIL < S.TAIL_SORT_MIN["tail_above"]


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_coverage_of_a_pushed_case(c):
    case = S.case_of(c)
    og, rounds, movers = S.oracle_world(c)
    walls = S.WALLS[case["walls"]]
    registered = set(S.HANDLERS[case["handlers"]])
    assert 1 <= len(rounds) <= S.MAX_ROUNDS, "movers left after %d rounds" % S.MAX_ROUNDS
    per_face = np.zeros(6, np.int64)
    absorbed = 0
    for this in rounds:
        for r in this:
            if r is not None:
                per_face += np.bincount(r.face, minlength=6)
                absorbed += len(r.absorbed)
                assert len(r.p) == r.n_keep + len(r.inj) and np.all(r.p["tag"][r.n_keep:] == 0)
    print(S.case_id(c), "refluxed per face", list(per_face), "absorbed", absorbed, "movers before each round", movers)
    for face in range(6):
        if walls[face] in registered:
            assert per_face[face] >= 50, "face %d refluxes %d" % (face, per_face[face])
        else:
            assert per_face[face] == 0
    if any(w == S.ABSORB or (w <= -3 and w not in registered) for w in walls):
        assert absorbed >= 20
    else:
        assert absorbed == 0
    if case["dims"] == (1, 6, 5):
        assert len(movers) >= 3 and sum(movers[1]) >= 10 and sum(movers[2]) >= 1
    if case["species"] == "with_chargeless_copy":                      # the copy refluxes and is absorbed, and deposits nothing
        r = rounds[0][1]
        assert len(r.inj) >= 100 and not r.inj["q"].any() and not r.p["q"].any() and np.all(r.p["tag"][:r.n_keep] > 10 ** 6)
        assert len(r.absorbed) >= 20 and np.any(r.inj["dispx"] != 0)
        p1 = S.species_particles(case, 1)
        pushed = D.Pushed(og, p1, D.interpolator(og), S.SCALE, -1.0)
        assert not pushed.a64.any() and pushed.nm == len(r.inj) + len(r.absorbed)
        f1, a1 = np.zeros(og.nv, L.field_t), np.zeros(og.nv + 1, L.accumulator_t)
        with pyorc.fixed_accumulator(og, S.SCALE) as (a64, _):
            S.predict_round(og, pushed.p, pushed.pm, 1, S.handlers_of(case, 1), S.draw_table(len(p1) + 64), f1, a1)
        assert not a64.any() and all(np.all(a1[c] == 0) for c in ("jx", "jy", "jz")) and np.all(f1["rhob"] == 0)
        # ... and its refluxed particles are told apart by their tangential momenta alone
        at = S.match_refluxed(r.inj, r.face, r.p[r.n_keep:], by_charge=False)
        assert np.array_equal(np.sort(at), np.arange(len(r.inj)))
    if case["handlers"] == "zero_second":                         # momentum and displacement exactly zero
        z = [r for this in rounds for r in this[1:] if r is not None]
        assert z and all(not r.inj[k].any() for r in z for k in ("ux", "uy", "uz", "dispx", "dispy", "dispz"))


def test_rhob_restatement_and_node_bound_against_the_oracle():
    """rhob_terms is accumulate_rhob: one particle at a time, its eight weights are the oracle's bit for bit (every surface
    cell kind of a grid with unequal cells: the doubled weights); and many particles into few nodes stay within the node
    bound of the float64 sum, which is not vacuous (it is below 1e-4 of the largest node value)."""
    rng = np.random.default_rng(3)
    og = pyorc.make_grid(4, 3, 2, 4.0, 4.5, 1.5, np.float32(0.3))
    n = 600
    p = D.particles(3, n, (4, 3, 2), 1.0)
    p["dx"][:50] = 1.0
    p["dy"][50:100] = -1.0
    nodes, w = S.rhob_terms(p, og)
    for k in range(n):
        f = np.zeros(og.nv, L.field_t)
        pyorc.accumulate_rhob(f, p[k:k + 1], og)
        want = np.zeros(og.nv, np.float32)
        np.add.at(want, nodes[k], w[k])
        assert bits_equal(f["rhob"], want), k
    prior = np.zeros(og.nv, np.float32)
    prior[rng.integers(0, og.nv, 20)] = 0.01
    f = np.zeros(og.nv, L.field_t)
    f["rhob"] = prior
    pyorc.accumulate_rhob(f, p, og)
    assert S.describe_rhob(f["rhob"], prior, p, og) is None
    s, bound, s32, cnt = S.rhob_bound(prior, p, og)
    busy = cnt > 10
    assert busy.sum() > 20 and np.all(bound[busy] < 1e-4 * np.abs(s[busy]).max()) and np.all(bound[busy] > 0)
    off = f["rhob"].copy()
    v = int(np.flatnonzero(busy)[0])
    off[v] += np.float32(2 * bound[v]) + np.spacing(off[v])           # twice the bound off at a busy node: seen
    assert S.describe_rhob(off, prior, p, og) is not None
    f2 = np.zeros(og.nv, L.field_t)                                    # two particles: nodes of one and of two terms
    pyorc.accumulate_rhob(f2, p[:2], og)
    zero = np.zeros(og.nv, np.float32)
    assert S.describe_rhob(f2["rhob"], zero, p[:2], og) is None
    v = int(np.flatnonzero(f2["rhob"])[0])
    off = f2["rhob"].copy()
    off[v] = np.nextafter(off[v], np.float32(np.inf))                  # one ulp off where order cannot matter: seen
    assert S.describe_rhob(off, zero, p[:2], og) is not None


def test_expected_normal_momentum_and_the_ulp_measure():
    """the oracle's own float draw is within the bound of the float64 expression (glibc's logf is within 1 ulp)"""
    d = S.draw_table(20000, seed=9)
    for face, para in ((0, 0.11), (4, 2.0)):
        u = np.array([pyorc.maxwellian_reflux_draw(d[k], para, 0.3, face)[0] for k in range(0, 20000, 10)])
        want = S.expected_normal(d[::10, 0], para)
        ulps = np.abs(np.abs(u).astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
        print("face %d: worst host error %.2f ulps" % (face, ulps.max()))
        assert ulps.max() <= S.NORMAL_ULPS and np.all((u < 0) == (face >= 3))


@pytest.mark.parametrize("first,second,walls", S.parked_pairings(), ids=lambda v: v if isinstance(v, str) else "")
def test_parked_pairings_on_the_oracle(first, second, walls):
    """movers on the faces -x and -y at once, every pairing of wall kinds: what the reference's face order and fall-through
    (boundary_p.c:240-316) make of them, stated here pairing by pairing"""
    args, kw, og = D.grids(S.PARKED_DIMS, walls)
    p, pm = S.parked_on((0, 1), 8, S.PARKED_DIMS, 17, n_rest=40)
    f, a = np.zeros(og.nv, L.field_t), np.zeros(og.nv + 1, L.accumulator_t)
    r = S.predict_round(og, p, pm, 0, [(-3, np.float32(0.11), np.float32(0.04))], S.draw_table(len(p)), f, a)
    falls = lambda kind: kind in ("unregistered", "reflect", "self")
    fate = "absorb" if first == "absorb" else "reflux0" if first == "handler" else \
        "absorb" if second == "absorb" or falls(second) else "reflux1"
    assert len(pm) >= 4
    if fate == "absorb":
        assert len(r.inj) == 0 and len(r.absorbed) == len(pm) and np.abs(f["rhob"]).sum() > 0
    else:
        assert len(r.inj) == len(pm) and np.all(r.face == int(fate[-1])) and not f["rhob"].any()


# ---- the emitter's arithmetic, restated ------------------------------------------------------------------------------------
U = 2.0 ** -24                                   # the unit roundoff of a float: one correctly rounded operation is within U
# Charge: both sides share e3 = ((q_m E) E) E and pre = ((eps0 dY) dZ) dt in float.  The device then takes coef as a float (U;
# 0 for coef = 1), a float product and a float quotient under the root (U each; the root halves the three: 1.5 U), sqrtf
# (U), and the product with pre and the division by n (2 U): 4.5 U.  The reference does all of it in double and rounds
# once: U.  Together 5.5 U = 3.3e-7 -- and the check may not be looser than the 2e-7 it replaces, so 2e-7 it is.
CHARGE_BOUND = min(5.5 * U * (1 + 1e-6), 2e-7)
# Displacement: g = u.u + 1 is a float sum of positive terms on both sides, in x y z order on the device and from the
# face's axis on cyclically in the reference (4 U each; the root halves their difference: 4 U); sqrtf, the quotient and the
# product with the age on the device (3 U) against one rounding of the double expression (U); u * age on both sides (2 U);
# * rd against / d, where rd and d are each the float nearest their ratio (2 U), and the last operation on both sides (2 U):
# 14 U of the displacement, which for displacements below 12 cells stays inside the 1e-5 of a cell it replaces.
DISP_BOUND = 14 * U * (1 + 1e-6)


def emit_world(seed, n_faces, n_emit, dims=(6, 5, 4), box=(6.0, 7.5, 3.0, 0.3)):
    rng = np.random.default_rng(seed)
    og = pyorc.make_grid(*dims, *box[:3], np.float32(box[3]))
    fi = np.zeros(og.nv, L.interpolator_t)
    for c in ("ex", "ey", "ez"):
        fi[c] = rng.uniform(-2, 2, og.nv).astype(np.float32)
    types = np.array(list(S.EMIT_FACES))[rng.integers(0, 6, n_faces)]
    cells = L.voxel(rng.integers(2, dims[0], n_faces), rng.integers(2, dims[1], n_faces), rng.integers(2, dims[2], n_faces), *dims)
    comps = (cells.astype(np.int64) * 32 + types).astype(np.int32)
    d = np.zeros((n_faces * n_emit, 6))
    d[:, :2] = rng.uniform(0, 1, (len(d), 2))
    d[:, 2:5] = rng.standard_normal((len(d), 3))
    d[:, 5] = rng.uniform(0, 1, len(d))
    return og, fi, comps, d


def worst_differences(og, fi, comps, n_emit, ut_perp, ut_para, q_m, d):
    inj, left = S.emit_restatement(og, fi, comps, n_emit, ut_perp, ut_para, q_m, S.COEF["child_langmuir"], 0.0, d)
    ref = S.emit_reference(og, fi, comps, n_emit, ut_perp, ut_para, q_m, d)
    assert len(inj) == len(ref) > 0
    for c in ("i", "dx", "dy", "dz", "ux", "uy", "uz", "sp_id"):         # the same double expressions, one rounding each
        assert bits_equal(inj[c], ref[c]), c
    assert bits_equal(left["q"], -inj["q"]) and bits_equal(left["dx"], inj["dx"])
    dq = np.abs(inj["q"].astype(np.float64) / ref["q"].astype(np.float64) - 1).max()
    dd = max(np.abs((inj[c].astype(np.float64) - ref[c]) / np.where(ref[c] == 0, 1, ref[c]).astype(np.float64)).max() for c in ("dispx", "dispy", "dispz"))
    da = max(np.abs(inj[c].astype(np.float64) - ref[c]).max() for c in ("dispx", "dispy", "dispz"))
    for c in ("dispx", "dispy", "dispz"):
        assert np.all((ref[c] == 0) == (inj[c] == 0)) and np.abs(ref[c]).max() < 12
    return dq, dd, da


def test_every_emitter_case_emits_from_every_orientation_on_the_restatement_alone():
    """the cases of tests/test_gpu_emit.py without a GPU: every one emits from faces of all six orientations, in surface
    cells and inner ones, keeps some faces from emitting (wrong sign, a volume code, below the threshold), and its emitted
    particles go through the oracle's injection (some stop on a wall: movers)"""
    import test_gpu_emit as E
    og = pyorc.make_grid(*E.DIMS, *E.BOX[:3], np.float32(E.BOX[3]), pbc=E.WALLS)
    assert {c[0] * c[1] for c in E.CASES} >= {255, 256, 257, 270} and {c[2] for c in E.CASES} == set(S.COEF)
    assert {c[1] for c in E.CASES} >= {1, 3} and {c[5] for c in E.CASES} == {"deterministic", "float"}
    movers = 0
    for n_comp, n_emit, law, thresh, q_m, mode in E.CASES:
        fi, comps = E.world(64 + n_comp, n_comp)
        emits, cell, axis, dirn, en = S._emit_common(og, fi, comps, n_emit, q_m, thresh)
        assert {int(a) * 2 + int(d > 0) for a, d in zip(axis[emits], dirn[emits])} == set(range(6))
        assert 0 < emits.sum() < (axis >= 0).sum() < len(emits)
        x = cell[emits] % (E.DIMS[0] + 2)
        assert np.any(x == 1) and np.any(x == E.DIMS[0]) and np.any((x > 1) & (x < E.DIMS[0]))
        inj, left = S.emit_restatement(og, fi, comps, n_emit, E.UT_PERP, E.UT_PARA, q_m, S.COEF[law], thresh, E.slot_draws(62, n_comp * n_emit))
        assert len(inj) == emits.sum() and np.all(np.isfinite(inj["q"])) and np.all(inj["q"] * q_m > 0)
        p, pm = np.zeros(len(inj), L.particle_t), np.zeros(len(inj) + 1, L.particle_mover_t)
        _, nm = pyorc.boundary_p_inject(p, 0, pm, 0, inj, np.zeros(og.nv + 1, L.accumulator_t), og)
        movers += nm
        print(n_comp, n_emit, "emitted", len(inj), "movers", nm)
    assert movers > 0


def test_emit_reference_form_is_the_oracles_child_langmuir():
    """emit_reference + orc_boundary_p_inject leaves the particles of orc_child_langmuir -- which tests/golden/reflux.npz pins
    on the reference's own model -- bit for bit, on the 72 faces of the fixture"""
    g = np.load(os.path.join(HERE, "golden", "reflux.npz"))
    og = pyorc.make_grid(*[int(v) for v in g["dims"]], *[float(v) for v in g["box"][:3]], np.float32(g["box"][3]))
    n_emit, ut_perp, ut_para, q_m = [float(v) for v in g["emit_par"]]
    n_emit = int(n_emit)
    comps, fi = g["emit_component"], g["emit_fi"]
    emits = S._emit_common(og, fi, comps, n_emit, q_m, 0.0)[0]
    assert emits.sum() == len(g["emit_p"])
    d = S.slot_table(emits, g["emit_draws"])
    ref = S.emit_reference(og, fi, comps, n_emit, ut_perp, ut_para, q_m, d)
    p, pm = np.zeros(len(ref), L.particle_t), np.zeros(len(ref), L.particle_mover_t)
    a = np.zeros(og.nv + 1, L.accumulator_t)
    new_np, nm = pyorc.boundary_p_inject(p, 0, pm, 0, ref, a, og)
    assert new_np == len(ref) and nm == 0
    want = g["emit_p"]
    key = lambda x: x[np.lexsort([x[c].view(np.uint32) for c in ("dz", "dy", "dx", "q")] + [x["i"]])]
    for c in ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q"):
        assert bits_equal(key(p)[c], key(want)[c]), c
    assert len({int(c) & 31 for c, e in zip(comps, emits[::n_emit]) if e}) == 6          # every orientation emits


def test_emit_restatement_against_the_reference_form_within_the_derived_bounds():
    """the float restatement of vpic_hip_emit against the double form: cell, position on the face and momenta bit-equal;
    charge within CHARGE_BOUND (relative) and displacements within DISP_BOUND (relative), the worst cases printed -- on
    the 72 faces of the fixture and on 10^5 seeded faces"""
    g = np.load(os.path.join(HERE, "golden", "reflux.npz"))
    og = pyorc.make_grid(*[int(v) for v in g["dims"]], *[float(v) for v in g["box"][:3]], np.float32(g["box"][3]))
    n_emit, ut_perp, ut_para, q_m = [float(v) for v in g["emit_par"]]
    emits = S._emit_common(og, g["emit_fi"], g["emit_component"], int(n_emit), q_m, 0.0)[0]
    d = S.slot_table(emits, g["emit_draws"])
    worst = [worst_differences(og, g["emit_fi"], g["emit_component"], int(n_emit), ut_perp, ut_para, q_m, d)]
    og2, fi2, comps2, d2 = emit_world(41, 100000, 1)
    worst.append(worst_differences(og2, fi2, comps2, 1, 0.05, 0.12, -1.0, d2))
    worst.append(worst_differences(og2, fi2, comps2[:30000], 3, 0.4, 0.9, 0.5, d2[:90000]))
    for name, w in zip(("fixture", "1e5 faces", "3e4 faces x 3, q_m > 0"), worst):
        print("%s: charge %.3g relative (bound %.3g), displacement %.3g relative (bound %.3g), %.3g of a cell"
              % (name, w[0], CHARGE_BOUND, w[1], DISP_BOUND, w[2]))
        assert w[0] <= CHARGE_BOUND <= 2e-7
        assert w[1] <= DISP_BOUND and w[2] <= 1e-5
