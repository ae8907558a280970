"""The exact reference of the hydro moments and rho (tests/moments_exact.py; oracle/vpic_oracle.h: orc_set_fixed_moments)
pinned on the oracle itself, without a GPU: the switch changes no float, the integers are the oracle's own floats rounded
(a deck where every node receives one contribution shows them one by one; tests/golden's k10 ties those floats to the
compiled reference), they do not depend on the order of the particles, and the oracle's own float sums lie within the
float bound the GPU test holds the engine to."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import moments_exact as X  # noqa: E402
from moments_exact import L, pyorc  # noqa: E402

DECKS = [(g, q_m) for g in X.GRIDS for q_m in X.Q_MS]


def deck_id(d):
    return "%s-q_m%+.2f" % d


@functools.lru_cache(maxsize=None)
def deck(grid, q_m):
    """(oracle grid, particles, reference) of one deck, computed once and left unchanged"""
    og = X.oracle_grid(grid)
    p = X.particles(31, X.N_PARTICLES[grid], grid)
    p.setflags(write=False)
    return og, p, X.Reference(og, p, q_m, X.interpolator(grid))


def plain(og, p, q_m, fi):
    """the oracle's float hydro and rhof with the switch off"""
    p = np.array(p)
    h, f = np.zeros(og.nv, L.hydro_t), np.zeros(og.nv, L.field_t)
    pyorc.accumulate_hydro_p(h, p, len(p), q_m, np.array(fi), og)
    pyorc.accumulate_rho_p(f, p, len(p), og)
    return h, f["rhof"].copy()


def test_the_decks_are_what_the_issue_asks_for():
    for grid in X.GRIDS:
        p = X.particles(31, X.N_PARTICLES[grid], grid)
        n = len(p)
        assert 4 * X.nv_of(grid) <= n <= 16000 and X.N_SPARSE < 4 * X.nv_of("10x9x7")
        assert (p["q"] > 0).sum() > n / 3 and (p["q"] < 0).sum() > n / 3 and 0.01 * n < (p["q"] == 0).sum() < 0.03 * n
        for c in ("dx", "dy", "dz"):
            for edge in (-1.0, 0.0, 1.0):
                assert (p[c] == edge).sum() >= 3, (grid, c, edge)
        speed = np.sqrt(sum(p[c].astype(np.float64) ** 2 for c in ("ux", "uy", "uz")))
        assert (speed < 1e-5).sum() > n / 4 and ((speed > 0.01) & (speed < 3)).sum() > n / 4 and (speed > 10).sum() > n / 4
    og = X.oracle_grid("10x9x7-stretched")
    for q_m in X.Q_MS:                              # off the powers of two: r8V, c, and the scales differ between the moments
        assert np.log2(8 * X.r8V_of(og)) % 1 != 0 and og.cvac == 2.0
        assert len(set(X.hydro_scales(0.015, q_m, og))) > 1
    assert X.rho_scale(og) != X.rho_scale(X.oracle_grid("10x9x7"))
    assert float(np.float32(X.Q_MS[1])) != X.Q_MS[1]


@pytest.mark.parametrize("d", DECKS, ids=deck_id)
def test_the_switch_changes_no_float(d):
    og, p, ref = deck(*d)
    h, rhof = plain(og, p, d[1], X.interpolator(d[0]))
    assert ref.h.tobytes() == h.tobytes() and ref.rhof.tobytes() == rhof.tobytes()
    assert np.abs(X.float_view(h)).max() > 0 and ref.m.count.sum() == ref.m.rcount.sum() == 8 * len(p)


@pytest.mark.parametrize("d", DECKS, ids=deck_id)
def test_one_contribution_per_node_is_the_oracles_float_rounded(d):
    """the float array holds the single contribution itself: h64 == llrint(float * scale), exactly (x * 2^k is exact in
    double, np.rint rounds to nearest even as llrint does)"""
    grid, q_m = d
    og = X.oracle_grid(grid)
    p = X.one_per_odd_cell(32, grid)
    ref = X.Reference(og, p, q_m, X.interpolator(grid), q_max=0.015)
    assert ref.m.count.max() == 1 and ref.m.rcount.max() == 1 and ref.m.count.sum() == 8 * len(p)
    want = np.rint(X.float_view(ref.h).astype(np.float64) * ref.m.scales).astype(np.int64)
    assert np.array_equal(ref.m.h64, want) and np.array_equal(ref.m.habs64, np.abs(want))
    want = np.rint(ref.rhof.astype(np.float64) * ref.m.rho_scale).astype(np.int64)
    assert np.array_equal(ref.m.r64, want) and np.array_equal(ref.m.rabs64, np.abs(want))
    assert np.abs(ref.m.h64).max(axis=0).min() > 2 ** 20                # every moment is resolved


@pytest.mark.parametrize("d", DECKS, ids=deck_id)
def test_the_integer_sums_do_not_depend_on_the_order(d):
    og, p, ref = deck(*d)
    for seed in (1, 2, 3):
        again = X.Reference(og, p[np.random.default_rng(seed).permutation(len(p))], d[1], X.interpolator(d[0]))
        for name in ("h64", "habs64", "count", "r64", "rabs64", "rcount"):
            assert np.array_equal(getattr(again.m, name), getattr(ref.m, name)), name
        assert again.hydro_words().tobytes() == ref.hydro_words().tobytes()


@pytest.mark.parametrize("d", DECKS, ids=deck_id)
def test_the_oracles_own_float_sums_lie_within_the_float_bound(d):
    og, p, ref = deck(*d)
    for what, got, rho in (("hydro", ref.h, False), ("rhof", ref.rhof, True)):
        worst, words, bad = X.float_errors(got, [ref], rho)
        print("%s %s: worst error / bound %.3f over %d words" % (deck_id(d), what, worst, words))
        assert bad is None, bad
        assert words == og.nv * (1 if rho else 14)
    # ... and the finalized words are within it too (one rounding of a sum that is exact to n q / 2)
    assert X.float_errors(ref.hydro_words(), [ref])[2] is None and X.float_errors(ref.rho_words(), [ref], True)[2] is None


def test_finalize_adds_onto_what_is_there_and_leaves_zero_sums_alone():
    og, p, ref = deck("10x9x7", -1.0)
    prev = np.zeros(og.nv, L.hydro_t)
    prev["jx"], prev["txy"] = np.float32(-0.0), np.float32(0.125)
    out = pyorc.finalize_moments(prev, ref.m.h64, ref.m.scales)
    zero = ref.m.h64 == 0
    assert zero.any() and (~zero).any()
    assert np.array_equal(X.float_view(out).view(np.uint32)[zero], X.float_view(prev).view(np.uint32)[zero])
    once = X.float_view(ref.hydro_words())
    want = np.where(zero, X.float_view(prev), X.float_view(prev) + once)
    assert np.array_equal(X.float_view(out).view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert not prev["rho"].any() and out["_pad"].tobytes() == prev["_pad"].tobytes()


def test_a_contribution_out_of_range_is_counted_and_not_added():
    og = X.oracle_grid("4x4x4")
    p = X.particles(33, 10, "4x4x4")
    p["q"], p["ux"] = 0.01, 0.0
    p["ux"][3] = 2.0 ** 40
    scales = X.hydro_scales(0.01, -1.0, og)
    h = np.zeros(og.nv, L.hydro_t)
    with pyorc.fixed_moments(og, scales, X.rho_scale(og)) as m:
        pyorc.accumulate_hydro_p(h, p, len(p), -1.0, np.array(X.interpolator("4x4x4")), og)
    assert m.skipped[0] > 0 and m.skipped[1] == 0 and np.abs(m.h64).max() < 2 ** 51 * 10
