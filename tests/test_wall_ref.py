"""The restatement of the absorbing walls that tally and record (tests/wall_ref.py) against the oracle, on the CPU.

  oracle agreement   for every case the particles the taker rule calls absorbed (faces 0..6) are Round.absorbed of
                     source_ref.predict_round on the grid that has VPIC_ABSORB_PARTICLES in the walls' place, bit for bit
  parked movers      corner movers on the faces -x and -y at once, every ordered pairing of wall+record, wall, plain absorb,
                     a code registered nowhere, reflux, reflect and this same domain: the first face in order that takes,
                     takes; who is absorbed is the oracle's
  coverage           no GPU case of tests/test_gpu_wall.py passes with nothing to check
  refused sums       a quantum that refuses some particles and keeps others"""
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
from source_ref import D, L, pyorc  # noqa: E402

WORLDS = sorted(set((c[0], c[1], c[2]) for c in W.CASES))


def world_id(k):
    return "%dx%dx%d-%s-%s" % (k[0] + k[1:])


def case_with(key):
    return next(c for c in W.CASES if (c[0], c[1], c[2]) == key)


def test_record_layouts():
    assert L.wall_tally_t.itemsize == 40 and L.wall_record_t.itemsize == 56
    assert [L.wall_record_t.fields[n][1] for n in ("dx", "i", "ux", "q", "tag", "tag2", "face", "sp")] == [0, 12, 16, 28, 32, 40, 48, 52]
    assert [L.wall_tally_t.fields[n][1] for n in ("count", "isum", "refused")] == [0, 8, 24]


@pytest.mark.parametrize("key", WORLDS, ids=world_id)
def test_the_taker_rule_absorbs_what_the_oracle_absorbs(key):
    c = case_with(key)
    case = W.case_of(c)
    og, rounds = W.oracle_world(c)
    assert len(rounds) >= 1
    for n, this in enumerate(rounds):
        for s, x in enumerate(this):
            if x is None:
                continue
            p, pm, r = x
            faces = W.absorbed_faces(p, pm, case["walls"], case["walled"], W.reflux_codes(case))
            mine = p[pm["i"][faces >= 0]]
            assert len(mine) == len(r.absorbed), (n, s, len(mine), len(r.absorbed))
            assert R.same_multiset(mine, r.absorbed, R.P_TAGGED), (n, s)
            # ... and the movers it does not call absorbed are the ones a handler took
            assert np.array_equal(np.sort(np.flatnonzero(faces < 0)), np.sort(r.who)), (n, s)


@pytest.mark.parametrize("key", WORLDS, ids=world_id)
def test_coverage_of_the_first_round(key):
    """every walled face takes at least 20 particles of every species in the first round, row 6 at least 20 in the layouts
    that have an unregistered absorbing face or an unregistered code, and every recording wall has something to record"""
    c = case_with(key)
    case = W.case_of(c)
    og, rounds = W.oracle_world(c)
    codes, walled = case["walls"], case["walled"]
    for s, x in enumerate(rounds[0]):
        assert x is not None
        p, pm, r = x
        faces = W.absorbed_faces(p, pm, codes, walled, W.reflux_codes(case))
        t = W.tally(p[pm["i"][faces >= 0]], faces[faces >= 0], 0, codes, walled, W.QUANTA)
        for f in range(6):
            if codes[f] in walled:
                assert t["count"][f, 0] >= 20, (f, s, int(t["count"][f, 0]))
            else:
                assert t["count"][f, 0] == 0
        if c[1] in ("mixed", "nowhere"):
            assert t["count"][6, 0] >= 20, (s, int(t["count"][6, 0]))
        assert int(t["count"].sum()) == int((faces >= 0).sum())
        assert not t["refused"].any()
        if any(v & W.RECORD for v in walled.values()):
            assert len(W.records(p[pm["i"][faces >= 0]], faces[faces >= 0], s, codes, walled)) >= 20
        if S.SPECIES[c[2]][s][1] == 0:                                  # a chargeless copy: counts, and sums of exactly zero
            assert not t["isum"].any()
        else:
            assert t["isum"][..., 0].any() and t["isum"][..., 1].any()


def test_coverage_of_the_case_list():
    layouts = set(c[1] for c in W.CASES)
    assert layouts == set(W.LAYOUTS)
    for lay in layouts:
        assert set(c[4] for c in W.CASES if c[1] == lay) == {"float", "deterministic"}, lay
        assert set(c[0] for c in W.CASES if c[1] == lay) == set(S.N_PARTICLES), lay
        assert set(c[2] for c in W.CASES if c[1] == lay) == set(S.SPECIES), lay
    assert set(c[3] for c in W.CASES) == set(S.STATES)
    for c in W.CASES:
        assert (c[3] == "thin") == (c[0] in S.THIN), c


@pytest.mark.parametrize("first,second,codes,walled,reflux", W.parked_pairings(), ids=lambda v: v if isinstance(v, str) else "")
def test_parked_on_two_faces_at_once(first, second, codes, walled, reflux):
    p, pm = S.parked_on((0, 1), 8, S.PARKED_DIMS, 17, n_rest=40)
    _, _, og = D.grids(S.PARKED_DIMS, W.oracle_codes(codes, walled))
    handlers = W.PARKED_HANDLERS if reflux else []
    faces = W.absorbed_faces(p, pm, codes, walled, [-3] if reflux else [])
    # the first face in order that takes, takes
    takes = lambda kind: kind in ("wall_record", "wall", "absorb", "reflux")
    want = 0 if takes(first) else 1 if takes(second) else 6
    if (want == 0 and first == "reflux") or (want == 1 and second == "reflux"):
        want = -1
    assert np.all(faces == want), (first, second, faces)
    f, a = np.zeros(og.nv, L.field_t), np.zeros(og.nv + 1, L.accumulator_t)
    r = S.predict_round(og, p, pm, 0, handlers, S.draw_table(len(p) + 64, seed=6), f, a)
    assert R.same_multiset(p[pm["i"][faces >= 0]], r.absorbed, R.P_TAGGED)
    # rows and records: a wall's own row, row 6 for plain absorb and "none"; a record only at wall_record
    if want >= 0:
        t = W.tally(p[pm["i"]], faces, 0, codes, walled, W.QUANTA)
        row = want if want < 6 and (first, second)[want] in ("wall_record", "wall") else 6
        assert t["count"][row, 0] == len(pm) and t["count"].sum() == len(pm)
        rec = W.records(p[pm["i"]], faces, 0, codes, walled)
        assert len(rec) == (len(pm) if want < 6 and (first, second)[want] == "wall_record" else 0)


def test_refused_sums():
    """REFUSING_QUANTA refuse some particles of a row and keep others, for either value; the counts do not change"""
    c = W.CASES[0]
    case = W.case_of(c)
    og, rounds = W.oracle_world(c)
    p, pm, r = rounds[0][0]
    faces = W.absorbed_faces(p, pm, case["walls"], case["walled"])
    rec, fc = p[pm["i"][faces >= 0]], faces[faces >= 0]
    t = W.tally(rec, fc, 0, case["walls"], case["walled"], W.REFUSING_QUANTA)
    keep = W.tally(rec, fc, 0, case["walls"], case["walled"], W.QUANTA)
    assert np.array_equal(t["count"], keep["count"])
    for j in range(2):
        refused, count = int(t["refused"][:, 0, j].sum()), int(t["count"][:, 0].sum())
        assert 0 < refused < count, (j, refused, count)
    for row in range(6):
        assert 0 < t["refused"][row, 0, 0] < t["count"][row, 0], row


def test_the_tally_is_additive_and_order_free():
    c = W.CASES[0]
    case = W.case_of(c)
    og, rounds = W.oracle_world(c)
    p, pm, r = rounds[0][0]
    faces = W.absorbed_faces(p, pm, case["walls"], case["walled"])
    rec, fc = p[pm["i"][faces >= 0]], faces[faces >= 0]
    whole = W.tally(rec, fc, 0, case["walls"], case["walled"], W.QUANTA)
    o = np.random.default_rng(1).permutation(len(rec))
    half = len(rec) // 2
    parts = W.tally(rec[o[:half]], fc[o[:half]], 0, case["walls"], case["walled"], W.QUANTA)
    parts = W.tally(rec[o[half:]], fc[o[half:]], 0, case["walls"], case["walled"], W.QUANTA, table=parts)
    assert W.same_table(whole, parts)
    # the quantised sums are the float64 sums within half a quantum per particle
    q = rec["q"].astype(np.float64)
    for row in range(7):
        m = np.array([f == row for f in fc])
        assert abs(float(whole["isum"][row, 0, 0]) * W.QUANTA[0] - q[m].sum()) <= 0.5 * W.QUANTA[0] * m.sum() + 1e-18
