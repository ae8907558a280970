"""tests/collide_rel_ref.py, the numpy restatement of vpic_hip_collide_relativistic's pair (include/vpic_hip.h), pinned on the
model it states: |q| = |p*| and the pair's sum m u and sum m gamma before the final rounding, a hand-worked pair, Lorentz
covariance along the polar axis, the cold limit against tests/collide_ref.py, and one constructed case for each guard.

THE MEASURED FIGURES (tests/test_gpu_collide_rel.py and tests/test_gpu_collide_rel_deck.py cite them; measured by this
module on the CPU, numpy float64, rounded up in the second significant digit, and asserted by the test named):
  test_cold_limit: drifting Maxwellians at |u| ~ 1e-3, mass ratios 1, 100 and 1836, the worst difference between the new
    momenta of this pair and of collide_ref.scatter (float32, non-relativistic), over both particles and three components,
    in units of |g| = |u_f - u_s|:                                                           WORST_COLD = 6.5e-7
  test_conservation_after_rounding: equal weights, |u| log-uniform in 1e-2 .. 30 in random directions, mass ratios 1, 100
    and 1836 (both ways round), 6000 pairs, from the float32 values in double, in units of 2^-24:
    max_c |d(m_f u_f + m_s u_s)_c| / max(m_f |u_f|, m_s |u_s|)                              : WORST_P_REL = 1.11
    |d(m_f gamma_f + m_s gamma_s)| / (m_f (gamma_f - 1) + m_s (gamma_s - 1))                : WORST_E_REL = 1.95
(gamma - 1 evaluated as u^2 / (gamma + 1).)  The GPU tests take K = 4 WORST_P_REL and K = 4 WORST_E_REL."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collide_ref as R0  # noqa: E402
import collide_rel_ref as R  # noqa: E402

F, D = np.float32, np.float64
ULP = 2.0 ** -24
EPS = 2.0 ** -53
WORST_COLD, WORST_P_REL, WORST_E_REL = 6.5e-7, 1.11, 1.95
RATIOS = ((1.0, 1.0), (1.0, 100.0), (100.0, 1.0), (1.0, 1836.0), (1836.0, 1.0))


def random_draws(rng, n):
    phi = rng.uniform(0, 2 * np.pi, n)
    return np.stack([rng.standard_normal(n), np.cos(phi), np.sin(phi), rng.uniform(0, 1, n)], 1).astype(F)


def log_uniform_momenta(rng, n, lo=1e-2, hi=30.0):
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (d * np.exp(rng.uniform(np.log(lo), np.log(hi), n))[:, None]).astype(F)


def gamma(u):
    u = np.asarray(u, D)
    return np.sqrt(1.0 + u @ u)


def kinetic(u):
    """gamma - 1 without the cancellation"""
    u = np.asarray(u, D)
    return (u @ u) / (gamma(u) + 1.0)


def test_the_shared_parts_are_the_existing_ones():
    for name in ("mix32", "perm", "pairs_same", "pairs_two", "cell_ranges", "cell_c0"):
        assert getattr(R, name) is getattr(R0, name)


def test_invariants_before_rounding():
    """|q| == |p*| to 16 x 2^-53, and the unrounded new momenta keep the pair's sum m u (per component) and sum m gamma to a
    few double ulps of E = sum m gamma: 16 x 2^-53 gC^2 E.  The factor gC^2: gamma*_f = gC (g_f - v_C.u_f) of the header
    subtracts two numbers that agree to 1 / (2 gC^2) for a particle that moves with the pair's frame, so an ulp of g_f is
    gC^2 ulps of the difference, and sum m gamma* times gC is E again.  gC reaches 30 here (900 ulps: 1e-13 E, still a
    millionth of a float32 ulp).  The pairs whose frame is slow, gC < 1.5, are also held to the plain 16 x 2^-53 E.
    That holds for an azimuth whose (cos phi, sin phi) is a unit vector exactly -- here the four axes; a draw rounded to
    float32 has cos^2 + sin^2 = 1 + e with |e| up to 2^-23, and then |q|^2 = |p*|^2 (1 + e sin_t^2), held in the second half."""
    rng = np.random.default_rng(5)
    worst, slow, n_slow = np.zeros(4), np.zeros(2), 0
    axes = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], F)
    for m_f, m_s in RATIOS:
        uf, us, dr = log_uniform_momenta(rng, 400), log_uniform_momenta(rng, 400), random_draws(rng, 400)
        for k in range(400):
            det, rough = {}, {}
            cvar = 10.0 ** rng.uniform(-8, 0)
            draw = (dr[k, 0],) + tuple(axes[k % 4]) + (dr[k, 3],)
            _, _, status = R.scatter(uf[k], us[k], 2.0, 2.0, m_f, m_s, cvar, 64, 0.3, 1.0, k % 7 == 0, draw, det)
            assert status == (True, True)
            E = float(det["E"])
            worst[0] = max(worst[0], abs(np.linalg.norm(det["q"]) - det["pm"]) / det["pm"] / EPS)
            dp = (m_f * det["nf"] + m_s * det["ns"]) - (m_f * uf[k].astype(D) + m_s * us[k].astype(D))
            worst[1] = max(worst[1], np.abs(dp).max() / E / EPS / det["gC"] ** 2)
            de = abs(m_f * gamma(det["nf"]) + m_s * gamma(det["ns"]) - E)
            worst[2] = max(worst[2], de / E / EPS / det["gC"] ** 2)
            if det["gC"] < 1.5:
                slow, n_slow = np.maximum(slow, [np.abs(dp).max() / E / EPS, de / E / EPS]), n_slow + 1
            R.scatter(uf[k], us[k], 2.0, 2.0, m_f, m_s, cvar, 64, 0.3, 1.0, k % 7 == 0, dr[k], rough)
            e = D(dr[k, 1]) ** 2 + D(dr[k, 2]) ** 2 - 1
            want = rough["pm"] * np.sqrt(1 + e * rough["sin_t"] ** 2)
            worst[3] = max(worst[3], abs(np.linalg.norm(rough["q"]) - want) / want / EPS)
    print("before rounding, in units of 2^-53: | |q| - |p*| | / |p*| %.2f, |d sum m u| / gC^2 E %.2f, |d sum m gamma| / gC^2 E %.2f; with float32 azimuths "
          "| |q| - |p*| sqrt(1 + e sin_t^2) | / |p*| %.2f" % tuple(worst))
    print("the %d pairs with gC < 1.5, unscaled: |d sum m u| / E %.2f, |d sum m gamma| / E %.2f" % (n_slow, slow[0], slow[1]))
    assert worst.max() <= 16 and slow.max() <= 16 and n_slow > 400


def test_hand_worked_equal_masses_opposite_momenta():
    """v_C = 0: p* = m u, s2 = cvar w N dt / V x p / (2 m gamma) x (m^2 gamma^2 / p^2 + 1)^2 / (m^2 gamma^2), and the result is
    u turned by theta with tan(theta / 2) = draw_N sqrt(s2) about an axis at azimuth phi: |u_f'| = |u|, u_s' = -u_f'"""
    m, w, cvar, N, dt, V = 3.0, 2.0, 2e-3, 6, 0.25, 0.5
    u = np.array([0.75, -1.5, 2.25], F)
    det = {}
    c, s = F(np.cos(1.1)), F(np.sin(1.1))
    nf, ns, status = R.scatter(u, -u, w, w, m, m, cvar, N, dt, V, False, (0.5, c, s, 0.5), det)
    assert status == (True, True)
    ud = u.astype(D)
    p, g = m * np.linalg.norm(ud), gamma(ud)
    s2 = D(F(cvar)) * w * N * dt / V * p / (2 * m * g) * (m * m * g * g / (p * p) + 1) ** 2 / (m * m * g * g)
    assert np.all(det["v"] == 0) and det["gC"] == 1 and np.array_equal(det["p"], m * ud)
    assert abs(det["s2"] - s2) <= 8 * EPS * s2 and abs(det["pm"] - p) <= 2 * EPS * p
    t = (0.5 * np.sqrt(s2)) ** 2
    cos_theta = (det["nf"] @ ud) / (ud @ ud)
    assert abs(cos_theta - (1 - t) / (1 + t)) <= 1e-14
    e = D(c) ** 2 + D(s) ** 2 - 1                               # (the float32 azimuth is a unit vector to 2^-24 only)
    assert abs(np.linalg.norm(det["nf"]) - np.linalg.norm(ud) * np.sqrt(1 + e * det["sin_t"] ** 2)) <= 8 * EPS * np.linalg.norm(ud)
    assert np.allclose(det["ns"], -det["nf"], rtol=0, atol=8 * EPS * np.linalg.norm(ud))
    # the azimuth: the turned part, in the basis (e1, e2) orthogonal to u that the header's D spans, points along phi
    e3 = ud / np.linalg.norm(ud)
    e1 = np.array([e3[0] * e3[2], e3[1] * e3[2], -(e3[0] ** 2 + e3[1] ** 2)]) / np.hypot(e3[0], e3[1])
    e2 = np.cross(e3, e1)
    assert abs(np.arctan2(det["nf"] @ e2, det["nf"] @ e1) - 1.1) <= 1e-6          # (cos phi, sin phi were rounded to float32)
    assert np.array_equal(nf, det["nf"].astype(F)) and np.array_equal(ns, det["ns"].astype(F))


def boost_z(u, B):
    """the momentum per mass u seen from a frame that moves with velocity B along z"""
    u = np.asarray(u, D)
    G = 1.0 / np.sqrt(1.0 - B * B)
    return np.array([u[0], u[1], G * (u[2] - B * gamma(u))], D)


@pytest.mark.parametrize("B", [0.6, -0.9])
def test_covariance_along_the_polar_axis(B):
    """A pair whose total momentum lies along z (the polar axis of the rotation's phi), seen from a second lab frame that
    moves along z: both frames reach the SAME centre-of-momentum frame, so p*, pm, q and the angle are the same, and s2 is
    the same once dt carries the factor (g_f' g_s') / (g_f g_s) that n dt / (g_f g_s) needs to be invariant at a fixed N / V.
    The second frame's momenta and dt are handed in as doubles; outputs compared in double, 1e-12 relative."""
    m_f, m_s = 1.0, 128.0
    uf = np.array([0.5, -0.25, 1.5], F)
    us = np.array([-0.5 / 128, 0.25 / 128, -0.02], F)            # m_f uf + m_s us is along z, exactly
    assert np.all((m_f * uf.astype(D) + m_s * us.astype(D))[:2] == 0)
    draw = (0.8, 0.0, -1.0, 0.5)       # (an azimuth that is a unit vector exactly: with a rounded one |q| != |p*| by 2^-24 sin_t^2, in both frames alike)
    a, b = {}, {}
    R.scatter(uf, us, 1.0, 1.0, m_f, m_s, 1e-2, 8, 0.5, 1.0, False, draw, a)
    uf2, us2 = boost_z(uf, B), boost_z(us, B)
    dt2 = D(0.5) * (gamma(uf2) * gamma(us2)) / (gamma(uf) * gamma(us))
    R.scatter(uf2, us2, 1.0, 1.0, m_f, m_s, 1e-2, 8, dt2, 1.0, False, draw, b)
    rel = lambda x, y: np.abs(np.asarray(x) - np.asarray(y)).max() / np.abs(np.asarray(x)).max()   # noqa: E731
    print("pm %.3e, s2 %.3e, p* %.3e, q %.3e" % (rel(a["pm"], b["pm"]), rel(a["s2"], b["s2"]), rel(a["p"], b["p"]), rel(a["q"], b["q"])))
    assert rel(a["pm"], b["pm"]) <= 1e-12 and rel(a["s2"], b["s2"]) <= 1e-12 and rel(a["p"], b["p"]) <= 1e-12 and rel(a["q"], b["q"]) <= 1e-12
    assert rel(a["omc"], b["omc"]) <= 1e-12 and a["omc"] > 1e-3                     # the deflection angle, and there is one
    assert rel(boost_z(a["nf"], B), b["nf"]) <= 1e-12 and rel(boost_z(a["ns"], B), b["ns"]) <= 1e-12


def test_cold_limit():
    """drifting Maxwellians at |u| ~ 1e-3: the relativistic pair against the existing non-relativistic one (float32), the
    worst difference of a new momentum in units of |g|; printed, asserted against WORST_COLD of the docstring.  What it
    holds: the existing pair's own float32 rounding (WORST_G of tests/test_collide_ref.py is 4.6 x 2^-24 = 2.8e-7 |g|, on D
    alone, and its u + f D is rounded to an ulp of |u|) and the relativistic terms themselves, of the order u^2 ~ 1e-6 times
    the change of the momentum (a few hundredths of |g| here)."""
    rng = np.random.default_rng(23)
    worst, turned = 0.0, []
    for m_f, m_s in RATIOS:
        m_ab = (F(m_f) * F(m_s)) / (F(m_f) + F(m_s))
        for drift, vth, cvar in (((3e-4, -2e-4, 4e-4), 4e-4, 1e-13), ((0.0, 0.0, 0.0), 6e-4, 1e-12), ((7e-4, 0.0, 0.0), 2e-4, 1e-14)):
            uf = (np.asarray(drift) + vth / np.sqrt(m_f) * rng.standard_normal((300, 3))).astype(F)
            us = (-np.asarray(drift) + vth / np.sqrt(m_s) * rng.standard_normal((300, 3))).astype(F)
            dr = random_draws(rng, 300)
            for k in range(300):
                nf, ns, status = R.scatter(uf[k], us[k], 2.0, 2.0, m_f, m_s, cvar, 64, 0.3, 1.0, k % 7 == 0, dr[k])
                of, os_, ostatus, _ = R0.scatter(uf[k], us[k], 2.0, 2.0, m_ab / F(m_f), m_ab / F(m_s), cvar, 64, 0.3, (F(1.0) * m_ab) * m_ab, k % 7 == 0, dr[k])
                assert status == (True, True) == ostatus
                g = np.linalg.norm(uf[k].astype(D) - us[k].astype(D))
                worst = max(worst, np.abs(nf.astype(D) - of).max() / g, np.abs(ns.astype(D) - os_).max() / g)
                turned.append(max(np.linalg.norm(nf.astype(D) - uf[k]), np.linalg.norm(ns.astype(D) - us[k])) / g)
    print("cold limit: worst difference to collide_ref.scatter %.3e |g|; median change of a momentum %.3e |g|" % (worst, np.median(turned)))
    assert worst <= WORST_COLD and np.median(turned) > 1e-2     # (the pairs are really turned: ten thousand times the difference)


def test_conservation_after_rounding():
    """the two figures of the docstring, printed and asserted"""
    rng = np.random.default_rng(31)
    worst = np.zeros(2)
    n = 1200
    for m_f, m_s in RATIOS:
        uf, us, dr = log_uniform_momenta(rng, n), log_uniform_momenta(rng, n), random_draws(rng, n)
        for k in range(n):
            nf, ns, status = R.scatter(uf[k], us[k], 2.0, 2.0, m_f, m_s, 10.0 ** rng.uniform(-8, 0), 64, 0.3, 1.0, k % 7 == 0, dr[k])
            assert status == (True, True)
            a, b, c, d = (x.astype(D) for x in (uf[k], us[k], nf, ns))
            dp = (m_f * c + m_s * d) - (m_f * a + m_s * b)
            worst[0] = max(worst[0], np.abs(dp).max() / max(m_f * np.linalg.norm(a), m_s * np.linalg.norm(b)) / ULP)
            de = (m_f * kinetic(c) + m_s * kinetic(d)) - (m_f * kinetic(a) + m_s * kinetic(b))
            worst[1] = max(worst[1], abs(de) / (m_f * kinetic(a) + m_s * kinetic(b)) / ULP)
    print("after rounding, in units of 2^-24: momentum %.3f, energy %.3f" % tuple(worst))
    assert worst[0] <= WORST_P_REL and worst[1] <= WORST_E_REL


# ---- the guards ----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


@pytest.mark.parametrize("m_s", [1.0, 1836.0])
def test_guard_identical_momenta(m_s):
    u = np.array([0.1, -2.0, 30.0], F)
    nf, ns, status = R.scatter(u, u, 1, 1, 1.0, m_s, 1e-3, 4, 0.1, 0.25, False, (0.3, 1, 0, 0.5))
    assert status == "skipped" and same_bits(nf, u) and same_bits(ns, u)
    nf, ns, status = R.scatter(np.zeros(3, F), -np.zeros(3, F), 1, 1, 1.0, m_s, 1e-3, 4, 0.1, 0.25, False, (0.3, 1, 0, 0.5))
    assert status == "skipped" and same_bits(ns, -np.zeros(3, F))      # (0 == -0 as floats: skipped, the signs kept)


def test_guard_pm_zero():
    """momenta that differ and a p* that is exactly 0: the first particle 2^200 times heavier and slow, so that E = m_f,
    v_C = u_f exactly and c_f = -1 -- the first particle rests in the pair's frame"""
    uf, us = np.array([1e-20, 0, 0], F), np.zeros(3, F)
    det = {}
    nf, ns, status = R.scatter(uf, us, 1, 1, 2.0 ** 100, 2.0 ** -100, 1e-3, 4, 0.1, 0.25, False, (0.3, 1, 0, 0.5), det)
    assert status == "skipped" and det == {} and same_bits(nf, uf) and same_bits(ns, us)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_guard_p_along_z(sign):
    """gp == 0: D = (pm sin cos phi, pm sin sin phi, -pz (1 - cos)), pz WITH ITS SIGN"""
    uf, us = np.array([0, 0, sign * 1.5], F), np.array([0, 0, -sign * 0.5], F)
    det = {}
    c, s = F(np.cos(0.7)), F(np.sin(0.7))
    nf, ns, status = R.scatter(uf, us, 1, 1, 1.0, 4.0, 5e-2, 4, 0.1, 0.25, False, (1.5, c, s, 0.5), det)
    assert status == (True, True) and det["gp"] == 0 and np.sign(det["p"][2]) == sign
    Dv = det["q"] - det["p"]
    e = D(c) ** 2 + D(s) ** 2 - 1                               # (the float32 azimuth is a unit vector to 2^-24 only)
    assert abs(np.linalg.norm(det["q"]) - det["pm"] * np.sqrt(1 + e * det["sin_t"] ** 2)) <= 4 * EPS * det["pm"]
    assert abs(Dv[0]) > 1e-3 and np.sign(Dv[2]) == -sign and abs(Dv[0] * s - Dv[1] * c) <= 1e-7 * abs(Dv[0])
    assert abs(nf[0]) > 1e-3 and abs(1.0 * nf[0].astype(D) + 4.0 * ns[0].astype(D)) <= 4 * ULP * abs(nf[0])


def test_guard_large_t_back_scatter():
    """t = d^2 not below 2^64, and a NaN (draw 0 times an infinite sqrt(s2): in double s2 overflows only for momenta near
    the smallest floats): sin = 0, 1 - cos = 2, q = -p* -- with equal masses and opposite momenta the two particles swap
    their momenta; just below the guard the formulas hold"""
    for u, dn in ((np.array([0.3, -1.0, 0.1], F), 1.0), (np.array([3e-42, -1e-42, 1e-42], F), 1.0), (np.array([3e-42, -1e-42, 1e-42], F), 0.0)):
        det = {}
        nf, ns, status = R.scatter(u, -u, 3e38, 3e38, 1e-19, 1e-19, 3e38, 1024, 3e38, 1e-38, False, (dn, 1, 0, 0.5), det)
        assert status == (True, True) and not det["t"] < R.TWO64 and np.array_equal(det["q"], -det["p"])
        assert np.isnan(det["t"]) == (dn == 0.0) and (np.isinf(det["s2"]) or u[0] > 0.1)
        assert same_bits(nf, -u) and same_bits(ns, u)
    u = np.array([0.3, -1.0, 0.1], F)
    det, d = {}, {}
    R.scatter(u, -u, 1, 1, 1.0, 1.0, 1.0, 1, 1.0, 1.0, False, (1.0, 1, 0, 0.5), d)
    R.scatter(u, -u, 1, 1, 1.0, 1.0, 1.0, 1, 1.0, 1.0, False, (F(2.0 ** 31 / np.sqrt(d["s2"])), 1, 0, 0.5), det)
    assert 2.0 ** 61 < det["t"] < R.TWO64 and np.isfinite(det["q"]).all() and abs(np.linalg.norm(det["q"]) - det["pm"]) <= 4 * EPS * det["pm"]


def test_guard_one_sided_update():
    """weights 1 and 4: the light particle is always turned, the heavy one iff U * 4 < 1; the larger weight enters s2"""
    uf, us = np.array([0.3, 0.0, -1.1], F), np.array([-0.1, 2.2, 0.1], F)
    for wf, ws, u, want in ((1, 4, 0.5, (True, False)), (1, 4, 0.1, (True, True)), (4, 1, 0.5, (False, True)), (4, 1, 0.2, (True, True)),
                            (2, 2, 0.999, (True, True))):
        nf, ns, status = R.scatter(uf, us, wf, ws, 1.0, 100.0, 1e-3, 4, 0.1, 0.25, False, (0.8, 0.6, 0.8, u))
        assert status == want
        assert same_bits(nf, uf) == (not want[0]) and same_bits(ns, us) == (not want[1])
    a, b = {}, {}
    R.scatter(uf, us, 1, 4, 1.0, 100.0, 1e-3, 4, 0.1, 0.25, False, (0.8, 0.6, 0.8, 0.1), a)
    R.scatter(uf, us, 4, 1, 1.0, 100.0, 1e-3, 4, 0.1, 0.25, False, (0.8, 0.6, 0.8, 0.1), b)
    assert a["s2"] == b["s2"] and np.array_equal(a["q"], b["q"])


def test_collide_walks_the_cells_like_the_existing_reference():
    """a cell of three and a cell of two: the triple in order at half the variance, the counts, the log"""
    L = np.dtype([("i", "i4"), ("ux", "f4"), ("uy", "f4"), ("uz", "f4"), ("q", "f4")])
    p = np.zeros(5, L)
    p["i"], p["q"] = [30, 30, 30, 31, 31], -0.5
    p["ux"], p["uy"], p["uz"] = [0.1, -1.1, 0.0, 0.7, 0.7], [0.0, 0.5, 2.0, 0.1, 0.1], [0.3, 0.0, -0.4, -3.0, -3.0]
    dr = random_draws(np.random.default_rng(2), 5)
    kw = dict(m_a=1.0, wq_a=2.0, cvar=1e-2, dt=0.5, seed=5, call=9, volume=F(1.0), draws=dr)
    log = []
    ua, _, st = R.collide(p, None, log=log, **kw)
    assert st == dict(cells=2, pairs=3, skipped=1, one_sided=0, fullest_cell=3)      # (the cell of two holds identical momenta)
    pm = R.perm(R.cell_c0(5, 9, 0, 0, 30), 3)
    assert [(a, b) for _, a, b, _, _, _ in log[:3]] == [(pm[0], pm[1]), (pm[1], pm[2]), (pm[2], pm[0])]
    u = np.stack([p["ux"], p["uy"], p["uz"]], 1)
    for a, b in ((pm[0], pm[1]), (pm[1], pm[2]), (pm[2], pm[0])):
        u[a], u[b], _ = R.scatter(u[a], u[b], 1.0, 1.0, 1.0, 1.0, 1e-2, 3, 0.5, F(1.0), True, dr[a])
    assert np.array_equal(u.view(np.uint32), ua.view(np.uint32))
