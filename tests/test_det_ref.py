"""The exact reference of the engine's deterministic accumulation, checked on the CPU (no GPU): the oracle's fixed-point
switch (oracle/vpic_oracle.h: orc_set_fixed_accumulator) and pyorc's fixed_scale / finalize, which restate the rule of
include/vpic_hip.h (vpic_hip_set_accumulation).  tests/test_gpu_det_exact.py holds the HIP push to these sums word for
word; here the sums themselves are pinned: the switch changes nothing else, the sums do not depend on the array order,
every streak is counted once, and a lone particle's sums are the compiled reference's own floats, rounded."""
import os

import numpy as np
import pytest

from conftest import bits_equal
import det_exact as D
from det_exact import L, pyorc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libvpic_ref.so")
SCALE = pyorc.fixed_scale(D.Q0)


def golden_case(golden, case):
    """(oracle grid, particles, interpolator, scale) of K2 / K3a / K3b of tests/golden/kernels.npz"""
    nx, ny, nz = [int(v) for v in golden["k1_dims"]]
    kw = dict(fbc=[int(x) for x in golden["k3b_fbc"]], pbc=[int(x) for x in golden["k3b_pbc"]]) if case == "k3b" else {}
    og = pyorc.make_grid(nx, ny, nz, 6.0, 5.0, 4.0, np.float32(0.3), **kw)
    p = golden["k2_p_in" if case == "k2" else "k3_p_in"].copy()
    p["tag"] = np.arange(len(p)) + 1
    return og, p, golden["k2_fi"], pyorc.fixed_scale(float(np.abs(p["q"]).max()))


def reflecting_case(n=600):
    """(5, 3, 2) with reflecting walls on all six faces, n particles.  Momenta N(0, 0.15): at DT a particle moves
    0.95 * 0.15 ~ 0.14 of a cell per axis and step, so about one in seven hits a wall on some axis (measured below, under
    the cap of a quarter that the reference pin needs)."""
    _, _, og = D.grids((5, 3, 2), "reflect")
    return og, D.particles(11, n, (5, 3, 2), 0.15), D.interpolator(og), SCALE


def the_case(golden, case):
    return reflecting_case() if case == "reflect" else golden_case(golden, case)


@pytest.mark.parametrize("case", ["k2", "k3a", "k3b", "reflect"])
def test_the_switch_changes_nothing_else(golden, case):
    """particles, movers and the float accumulator with the switch on: bit for bit those of a run with it off
    (which tests/test_oracle_golden.py pins on the reference's)"""
    og, p, fi, scale = the_case(golden, case)
    on = D.Pushed(og, p, fi, scale)
    off_p, off_pm, off_a = p.copy(), np.zeros(len(p) + 1, L.particle_mover_t), np.zeros(og.nv + 1, L.accumulator_t)
    nm = pyorc.advance_p(off_p, len(p), D.Q_M, off_pm, off_a, fi, og)
    assert nm == on.nm and (case not in ("k3b",) or nm > 0)
    assert bits_equal(on.p, off_p) and bits_equal(on.pm, off_pm[:nm]) and bits_equal(on.a, off_a)
    assert on.streaks.sum() >= len(p) and np.abs(on.a64).max() > 0
    # the switch is off again: another push leaves the arrays it was given alone
    before = on.a64.copy()
    pyorc.advance_p(p.copy(), len(p), D.Q_M, off_pm, off_a, fi, og)
    assert np.array_equal(on.a64, before)


@pytest.mark.parametrize("case", ["k2", "k3a", "k3b", "reflect"])
def test_the_sums_do_not_depend_on_the_array_order(golden, case):
    og, p, fi, scale = the_case(golden, case)
    a = D.Pushed(og, p, fi, scale)
    b = D.Pushed(og, p[np.random.default_rng(3).permutation(len(p))], fi, scale)
    assert np.array_equal(a.a64, b.a64) and np.array_equal(a.streaks, b.streaks)
    assert bits_equal(D.by_tag(a.p), D.by_tag(b.p))
    # ... which the float sums do: the reason for the fixed-point mode
    assert case == "k2" or not bits_equal(a.a, b.a)


def cell_coords(i, og):
    sx, sy = og.nx + 2, og.ny + 2
    return np.stack([i % sx, (i // sx) % sy, i // (sx * sy)], axis=1)


def segments(p_in, p_out, og):
    """How many straight streaks each particle made, from what it did -- the faces it crossed, from the change of its cell,
    and the walls it bounced off -- plus one.  Needs: less than a cell per axis and step, at least two cells on a periodic
    axis, no absorbing wall.  A bounce on an axis: the particle is still in its cell at the wall, and where it ended is
    where the folded path ends (2 - dx - d for the upper wall), not where the straight one does (dx +- d); d from the
    momentum it ended with, in double."""
    n = np.array([og.nx, og.ny, og.nz])
    c0, c1 = cell_coords(p_in["i"], og), cell_coords(p_out["i"], og)
    dc = np.abs(c1 - c0)
    crossed = np.where(dc == 0, 0, 1)
    assert np.all((dc <= 1) | (dc == n - 1))
    u = np.stack([p_out[c].astype(np.float64) for c in ("ux", "uy", "uz")], axis=1)
    cdt = float(og.cvac) * float(og.dt) * np.array([float(og.rdx), float(og.rdy), float(og.rdz)])
    d = 2 * np.abs(u) * cdt / np.sqrt(1 + (u * u).sum(axis=1))[:, None]
    x0 = np.stack([p_in[c].astype(np.float64) for c in ("dx", "dy", "dz")], axis=1)
    x1 = np.stack([p_out[c].astype(np.float64) for c in ("dx", "dy", "dz")], axis=1)
    bounced = np.zeros_like(crossed)
    for axis in range(3):
        for hi in (0, 1):
            if og.pbc[axis + 3 * hi] != D.REFLECT:
                continue
            s = 1.0 if hi else -1.0
            at_wall = (c0[:, axis] == (n[axis] if hi else 1)) & (dc[:, axis] == 0)
            folded = s * 2 - x0[:, axis] - s * d[:, axis]
            straight = np.minimum(np.abs(x1[:, axis] - (x0[:, axis] + d[:, axis])), np.abs(x1[:, axis] - (x0[:, axis] - d[:, axis])))
            hit = at_wall & (s * (x0[:, axis] + s * d[:, axis]) > 1) & (np.abs(x1[:, axis] - folded) < straight)
            bounced[:, axis] += hit
    return crossed.sum(axis=1) + bounced.sum(axis=1) + 1, bounced.sum(axis=1)


@pytest.mark.parametrize("case", ["k2", "k3a", "reflect"])
def test_every_streak_is_counted_once(golden, case):
    """sum(streaks) = the particles that stayed in their cell + the segments of those that did not, counted from what the
    particles did, not from what the oracle says it deposited; and per voxel the count is at least the particles that
    started there"""
    og, p, fi, scale = the_case(golden, case)
    r = D.Pushed(og, p, fi, scale)
    seg, bounces = segments(p, r.p, og)
    assert r.nm == 0
    assert int(r.streaks.sum()) == int(seg.sum())
    assert int((seg == 1).sum()) + int(seg[seg > 1].sum()) == int(seg.sum())
    if case == "k2":
        assert np.all(seg == 1) and np.array_equal(r.streaks, np.bincount(p["i"], minlength=og.nv))
    else:
        assert (seg > 1).sum() > len(p) // 8 and seg.max() >= 3
    assert (bounces.sum() > 0) == (case == "reflect")
    assert np.all(r.streaks >= np.bincount(p["i"], minlength=og.nv))
    # ghost voxels receive nothing
    c = cell_coords(np.arange(og.nv), og)
    ghost = np.any((c == 0) | (c == np.array([og.nx, og.ny, og.nz]) + 1), axis=1)
    assert not r.streaks[ghost].any() and not r.a64[ghost].any()


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libvpic_ref.so is not built (make -C oracle ref needs the reference's sources)")
@pytest.mark.parametrize("case", ["k3a", "reflect"])
def test_a_lone_particles_sums_are_the_compiled_references_floats_rounded(golden, case):
    """Each particle alone through the compiled reference's advance_p into a cleared accumulator, and alone through the
    oracle with the switch on: where a voxel got one streak, the reference's 12 floats ARE that streak, so
    llrint(float * scale) must be the oracle's integers; a voxel with no streak is zero in both.  Voxels with more than
    one streak hold a float sum the integers cannot be read from and are left out: none on the periodic grid (a particle
    never enters a voxel twice in one step there), only those of bouncing particles on the reflecting one, under a quarter
    of the set.  The lone sums add up to the whole set's."""
    from oracle import pyref
    og, p, fi, scale = the_case(golden, case)
    p = p[:400]
    lx, ly, lz = (6.0, 5.0, 4.0) if case == "k3a" else (5.0, 3.0, 2.0)
    g = pyref.new_periodic_grid(og.nx, og.ny, og.nz, lx, ly, lz, np.float32(og.dt))
    if case == "reflect":
        for face in range(6):
            pyref.set_face_bc(g, face, L.PEC_FIELDS, L.REFLECT_PARTICLES)
    stride = (og.nv + 1) & ~1
    a_ref = np.zeros((1 + pyref.n_pipeline()) * stride, L.accumulator_t)
    pm = np.zeros(16, L.particle_mover_t)
    whole = D.Pushed(og, p, fi, scale)
    _, bounces = segments(p, whole.p, og)
    total = np.zeros_like(whole.a64)
    left_out = 0
    for k in range(len(p)):
        lone = D.Pushed(og, p[k:k + 1], fi, scale)
        one = p[k:k + 1].copy()
        a_ref[:] = 0
        assert pyref.advance_p(one, 1, D.Q_M, pm, a_ref, fi, g) == 0
        pyref.reduce_accumulators(a_ref, g)
        assert bits_equal(one, lone.p)
        r = a_ref[:og.nv].view(np.float32).reshape(-1, 12).astype(np.float64)
        assert not a_ref[og.nv:].view(np.uint32).any()
        once, never = lone.streaks == 1, lone.streaks == 0
        assert np.array_equal(np.rint(r[once] * scale).astype(np.int64), lone.a64[once]), k     # (np.rint: to nearest even, as llrint)
        assert not r[never].any() and not lone.a64[never].any()
        if not (once | never).all():
            left_out += 1
            assert bounces[k] > 0, k
        total += lone.a64
    assert np.array_equal(total, whole.a64)
    if case == "k3a":
        assert left_out == 0
    else:
        assert 0 < left_out < len(p) // 4 and int((bounces > 0).sum()) < len(p) // 4


def test_fixed_scale_restates_the_engines_rule():
    """2^(37 - e) with 4.2 q_ref = m 2^e, 0.5 <= m < 1: a deposit of 4.2 q_ref lands in [2^36, 2^37)"""
    for q in (1.0, 0.01, 0.004, 2.0 ** -20, 3.7e5, 1 / 4.2, np.nextafter(1 / 4.2, 1)):
        s = pyorc.fixed_scale(q)
        assert s == 2.0 ** round(np.log2(s))
        assert 2.0 ** 36 <= 4.2 * q * s < 2.0 ** 37
    assert pyorc.fixed_scale(0.01) == 2.0 ** 41 and pyorc.fixed_scale(1.0) == 2.0 ** 34


def test_finalize_against_python_integers():
    """finalize(a64, scale) = float32(float64(sum) / scale) word by word, from Python's exact integers and fractions:
    one rounding to float below 2^53; above it int64 -> double rounds first (to nearest even), which the expected values
    spell out."""
    from fractions import Fraction
    scale = 2.0 ** 41
    sums = [0, 1, -1, 3, (1 << 24) + 1, -(1 << 24) - 1, (1 << 25) + 1, (1 << 25) + 3, (1 << 37) + (1 << 12), (1 << 37) + (1 << 13) + (1 << 12),
            (1 << 53) - 1, (1 << 53) + 1, (1 << 53) + 3, -(1 << 53) - 1, (1 << 54) + (1 << 30) + 2, (1 << 54) + (1 << 30) + 1, (1 << 62) + 12345, -(1 << 62) - 12345,
            (1 << 53) + (1 << 29) + 1, 0, 0, 0, 0, 0]
    a64 = np.array(sums, np.int64).reshape(2, 12)
    got = pyorc.finalize(a64, scale).view(np.float32).reshape(-1)
    assert got.dtype == np.float32 and pyorc.finalize(a64, scale).dtype == L.accumulator_t

    def nearest_even(x, bits):
        """the integer x rounded to `bits` significant bits, ties to even"""
        if x == 0:
            return 0
        s, x = (-1 if x < 0 else 1), abs(x)
        drop = max(x.bit_length() - bits, 0)
        q, r = x >> drop, x & ((1 << drop) - 1)
        half = 1 << (drop - 1) if drop else 0
        if drop and (r > half or (r == half and q & 1)):
            q += 1
        return s * (q << drop)

    for x, g in zip(sums, got):
        want = Fraction(nearest_even(nearest_even(x, 53), 24), 1 << 41)
        assert Fraction(float(g)) == want, x
    assert np.signbit(got[sums.index(0)]) == 0                       # a zero sum is +0.0
    # the two roundings are not one: 2^53 + 2^29 + 1 rounds to 2^53 + 2^29 as a double (a tie for the float: to even,
    # 2^53), while one rounding of the integer would go up
    x = (1 << 53) + (1 << 29) + 1
    assert nearest_even(x, 24) == (1 << 53) + (1 << 30) and nearest_even(nearest_even(x, 53), 24) == 1 << 53
    assert float(got[sums.index(x)]) == float(1 << 53) / scale
    # above 2^53 the conversion int64 -> double rounds: 2^53 + 1 is not a double
    assert float(np.int64((1 << 53) + 1).astype(np.float64)) == float(1 << 53)
