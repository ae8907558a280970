"""tests/collide_ref.py, the numpy restatement of vpic_hip_collide's rule (include/vpic_hip.h), pinned on the model it
states: the ranks are a permutation, who pairs with whom, |g + D| = |g| and momentum for every pair, and one constructed
case for each of the four guards.

THE MEASURED BASE of the GPU conservation bounds (tests/test_gpu_collide.py cites these figures).  Per pair of equal
weights, over the drifting Maxwellians and the mass ratios 1, 100 and 1836 of test_per_pair_conservation, the worst
deviations seen, in units of 2^-24:
    | |g + D| - |g| | / |g|                                                        : WORST_G = 4.63
    max_c |d(m_f u_f + m_s u_s)_c| / max(m_f |u_f|, m_s |u_s|)                     : WORST_P = 1.32
    |d(m_f u_f^2 + m_s u_s^2)| / max(m_f u_f^2, m_s u_s^2)                         : WORST_E = 9.77
(|u| the modulus of the particle's momentum; d: after minus before, evaluated in double from the float32 values; the
figures are the measured ones rounded up in the second decimal, and test_per_pair_conservation asserts that its pairs
stay within them.)  The GPU test takes K = 4 WORST_P for the momentum sums and K = 4 WORST_E for the energy sums."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collide_ref as R  # noqa: E402

F = np.float32
ULP = 2.0 ** -24
WORST_G, WORST_P, WORST_E = 4.63, 1.32, 9.77


def test_mix32_is_the_engines():
    """two values worked by hand from the definition, and injectivity on a run of consecutive counters"""
    def slow(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xffffffff; x ^= x >> 15; x = x * 0x846ca68b & 0xffffffff; x ^= x >> 16
        return x
    for x in (0, 1, 0x9e3779b9, 0xffffffff, 123456789):
        assert int(R.mix32(x)) == slow(x)
    assert len(np.unique(R.mix32(np.arange(1 << 16) + 0xfffffff0))) == 1 << 16          # (the counter wraps: still no tie)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1024])
def test_perm_is_a_permutation_and_the_pairs_of_one_species(n):
    c0 = R.cell_c0(7, 3, 1, 0, 41 + n)
    p = R.perm(c0, n)
    assert sorted(p.tolist()) == list(range(n))
    k = R.keys(c0, n)
    assert all(k[p[r]] < k[p[r + 1]] for r in range(n - 1))
    prs = R.pairs_same(p)
    firsts = [a for a, _, _, _ in prs]
    assert len(set(firsts)) == len(firsts)                       # first particle of at most one pair
    assert [j for _, _, j, _ in prs] == list(range(len(prs)))    # the pairs' numbers count up
    count = np.zeros(n, int)
    for a, b, _, half in prs:
        assert a != b
        count[a] += 1
        count[b] += 1
    if n < 2:
        assert prs == []
    elif n % 2 == 0:
        assert (count == 1).all() and not any(h for *_, h in prs)
    else:
        triple = set(p[:3].tolist())
        assert all(count[k] == (2 if k in triple else 1) for k in range(n))
        assert [(a, b) for a, b, _, _ in prs[:3]] == [(p[0], p[1]), (p[1], p[2]), (p[2], p[0])]
        assert [h for *_, h in prs] == [True] * 3 + [False] * (len(prs) - 3)


@pytest.mark.parametrize("n_a,n_b", [(0, 5), (5, 0), (1, 1), (1, 7), (7, 1), (64, 64), (64, 65), (65, 3), (3, 65), (200, 7), (256, 300), (1024, 1)])
def test_pairs_of_two_species(n_a, n_b):
    pa, pb = R.perm(R.cell_c0(1, 2, 0, 0, 9), n_a), R.perm(R.cell_c0(1, 2, 1, 0, 9), n_b)
    swap, prs = R.pairs_two(pa, pb)
    assert swap == (n_b > n_a)                                   # a on a tie
    n_l, n_s = max(n_a, n_b), min(n_a, n_b)
    if n_s == 0:
        assert prs == []
        return
    assert len(prs) == n_l and [j for _, _, j in prs] == list(range(n_l))
    assert sorted(kl for kl, _, _ in prs) == list(range(n_l))    # every L particle in exactly one pair, as its first particle
    per_s = np.bincount([ks for _, ks, _ in prs], minlength=n_s)
    assert set(per_s.tolist()) <= {n_l // n_s, -(-n_l // n_s)} and per_s.sum() == n_l
    pl, ps = (pb, pa) if swap else (pa, pb)
    assert all(kl == pl[j] and ks == ps[j % n_s] for kl, ks, j in prs)


def maxwellian_pairs(rng, n, drift, vth):
    return (np.asarray(drift, F) + vth * rng.standard_normal((n, 3))).astype(F), (np.asarray(drift, F) + vth * rng.standard_normal((n, 3))).astype(F)


def random_draws(rng, n):
    phi = rng.uniform(0, 2 * np.pi, n)
    return np.stack([rng.standard_normal(n), np.cos(phi), np.sin(phi), rng.uniform(0, 1, n)], 1).astype(F)


def pair_figures(uf, us, nf, ns, m_f, m_s, D):
    """the three deviations of the docstring, in units of 2^-24, from the float32 values in double"""
    uf, us, nf, ns, D = (np.asarray(x, np.float64) for x in (uf, us, nf, ns, D))
    g = uf - us
    fig_g = abs(np.linalg.norm(g + D) - np.linalg.norm(g)) / np.linalg.norm(g)
    dp = (m_f * nf + m_s * ns) - (m_f * uf + m_s * us)
    fig_p = np.abs(dp).max() / max(m_f * np.linalg.norm(uf), m_s * np.linalg.norm(us))
    de = (m_f * nf @ nf + m_s * ns @ ns) - (m_f * uf @ uf + m_s * us @ us)
    fig_e = abs(de) / max(m_f * uf @ uf, m_s * us @ us)
    return fig_g / ULP, fig_p / ULP, fig_e / ULP


def test_per_pair_conservation():
    """every pair: |g + D| against |g|, and with equal weights m_f u_f + m_s u_s and the energy before and after; the
    worst figures are printed, asserted against the bounds above and recorded in this module's docstring"""
    rng = np.random.default_rng(11)
    worst = np.zeros(3)
    for m_f, m_s in ((1.0, 1.0), (1.0, 100.0), (100.0, 1.0), (1.0, 1836.0)):
        m_ab = (F(m_f) * F(m_s)) / (F(m_f) + F(m_s))
        for drift, vth, cvar in (((0.05, -0.02, 0.1), 0.02, 1e-7), ((0.0, 0.0, 0.0), 0.05, 1e-5), ((0.2, 0.0, 0.0), 0.01, 1e-9), ((0.0, 0.0, 0.1), 0.003, 1e-4)):
            uf, us = maxwellian_pairs(rng, 600, drift, vth)
            dr = random_draws(rng, 600)
            for k in range(600):
                nf, ns, status, D = R.scatter(uf[k], us[k], 2.0, 2.0, m_ab / F(m_f), m_ab / F(m_s), cvar, 64, 0.3, (F(1.0) * m_ab) * m_ab, k % 7 == 0, dr[k])
                assert status == (True, True)
                worst = np.maximum(worst, pair_figures(uf[k], us[k], nf, ns, m_f, m_s, D))
    print("worst per-pair deviations in units of 2^-24: |g+D| %.2f, momentum %.2f, energy %.2f" % tuple(worst))
    assert worst[0] <= WORST_G and worst[1] <= WORST_P and worst[2] <= WORST_E


def test_guard_no_relative_velocity():
    u = np.array([0.1, -0.2, 0.3], F)
    nf, ns, status, D = R.scatter(u, u, 1, 1, 0.5, 0.5, 1e-3, 4, 0.1, 0.25, False, (0.3, 1, 0, 0.5))
    assert status == "skipped" and D is None and (nf.view(np.uint32) == u.view(np.uint32)).all() and (ns.view(np.uint32) == u.view(np.uint32)).all()


@pytest.mark.parametrize("gz", [0.25, -0.25])
def test_guard_g_along_z(gz):
    """gp == 0: D = (gm sin cos phi, gm sin sin phi, -gz (1 - cos)), gz WITH ITS SIGN -- with gm in its place a pair that
    approaches along -z would leave with |g + D| != |g|"""
    uf, us = np.array([0.1, 0.1, 0.1 + gz], F), np.array([0.1, 0.1, 0.1], F)
    c, s = F(np.cos(0.7)), F(np.sin(0.7))
    nf, ns, status, D = R.scatter(uf, us, 1, 1, 0.5, 0.5, 2e-3, 4, 0.1, 0.25, False, (1.5, c, s, 0.5))
    assert status == (True, True)
    g = (uf - us).astype(np.float64)
    assert g[0] == 0 and g[1] == 0 and abs(D[0]) > 1e-3 and abs(D[2]) > 1e-4
    assert abs(np.linalg.norm(g + D) - np.linalg.norm(g)) <= WORST_G * ULP * np.linalg.norm(g)
    assert np.sign(D[2]) == -np.sign(gz)
    assert np.allclose(D[0] * s, D[1] * c, rtol=1e-6)            # the azimuth is phi


def test_guard_overflowing_angle():
    """t = d^2 not below 2^64 (here infinite): sin = 0, 1 - cos = 2, the relative velocity is reversed exactly"""
    uf, us = np.array([0.3, 0.0, -0.1], F), np.array([-0.1, 0.2, 0.1], F)
    nf, ns, status, D = R.scatter(uf, us, 1, 1, 0.5, 0.5, 1e30, 4, 1e10, 1e-20, False, (1.0, 1, 0, 0.5))
    g = uf - us
    assert status == (True, True) and (D == F(-2) * g).all()
    assert np.array_equal(nf, uf + F(0.5) * D) and np.allclose(nf, us, atol=1e-7) and np.allclose(ns, uf, atol=1e-7)
    # ... and a NaN (draw 0 times an infinite s2) takes the same branch
    _, _, status, D = R.scatter(uf, us, 1, 1, 0.5, 0.5, 1e30, 4, 1e10, 1e-20, False, (0.0, 1, 0, 0.5))
    assert status == (True, True) and (D == F(-2) * g).all()
    # just below the guard the formulas hold: t = 2^62
    nf, ns, status, D = R.scatter(uf, us, 1, 1, 0.5, 0.5, 1.0, 1, 1.0, 1.0, False, (2.0 ** 31 * float(np.linalg.norm(g.astype(np.float64))) ** 1.5, 1, 0, 0.5))
    assert np.isfinite(D).all() and abs(np.linalg.norm(g + D.astype(np.float64)) - np.linalg.norm(g)) < 1e-6


def test_guard_one_sided_update():
    """weights 1 and 4: the light particle is always turned, the heavy one iff U * 4 < 1"""
    uf, us = np.array([0.3, 0.0, -0.1], F), np.array([-0.1, 0.2, 0.1], F)
    for wf, ws, u, want in ((1, 4, 0.5, (True, False)), (1, 4, 0.1, (True, True)), (4, 1, 0.5, (False, True)), (4, 1, 0.2, (True, True)),
                            (2, 2, 0.999, (True, True))):
        nf, ns, status, D = R.scatter(uf, us, wf, ws, 0.5, 0.5, 1e-3, 4, 0.1, 0.25, False, (0.8, 0.6, 0.8, u))
        assert status == want
        assert np.array_equal(nf, uf) == (not want[0]) and np.array_equal(ns, us) == (not want[1])
        # the larger weight enters the variance: the same D whichever of the two is the heavy one
    d1 = R.scatter(uf, us, 1, 4, 0.5, 0.5, 1e-3, 4, 0.1, 0.25, False, (0.8, 0.6, 0.8, 0.1))[3]
    d2 = R.scatter(uf, us, 4, 1, 0.5, 0.5, 1e-3, 4, 0.1, 0.25, False, (0.8, 0.6, 0.8, 0.1))[3]
    assert np.array_equal(d1, d2)


def test_triple_runs_in_order_at_half_the_variance_and_cells_must_be_contiguous():
    """a cell of three: pairs (p0,p1), (p1,p2), (p2,p0) each see what the one before left; collide() counts them"""
    L = np.dtype([("i", "i4"), ("ux", "f4"), ("uy", "f4"), ("uz", "f4"), ("q", "f4")])
    p = np.zeros(3, L)
    p["i"], p["q"] = 30, -0.5
    p["ux"], p["uy"], p["uz"] = [0.1, -0.1, 0.0], [0.0, 0.05, 0.02], [0.03, 0.0, -0.04]
    dr = random_draws(np.random.default_rng(2), 3)
    kw = dict(m_a=1.0, wq_a=2.0, cvar=1e-4, dt=0.5, seed=5, call=9, volume=F(1.0), draws=dr)
    log = []
    ua, _, st = R.collide(p, None, log=log, **kw)
    assert st == dict(cells=1, pairs=3, skipped=0, one_sided=0, fullest_cell=3)
    pm = R.perm(R.cell_c0(5, 9, 0, 0, 30), 3)
    assert [(a, b) for _, a, b, _, _, _ in log] == [(pm[0], pm[1]), (pm[1], pm[2]), (pm[2], pm[0])]
    u = np.stack([p["ux"], p["uy"], p["uz"]], 1)
    for a, b in ((pm[0], pm[1]), (pm[1], pm[2]), (pm[2], pm[0])):
        u[a], u[b], _, _ = R.scatter(u[a], u[b], 1.0, 1.0, 0.5, 0.5, 1e-4, 3, 0.5, F(0.25), True, dr[a])
    assert np.array_equal(u.view(np.uint32), ua.view(np.uint32))
    assert np.allclose(ua.sum(0), np.stack([p["ux"], p["uy"], p["uz"]], 1).sum(0), atol=1e-7)
    q = np.zeros(3, L)
    q["i"] = [30, 31, 30]
    with pytest.raises(AssertionError, match="not contiguous"):
        R.collide(q, None, **kw)
