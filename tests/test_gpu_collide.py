"""vpic_hip_collide on the device against tests/collide_ref.py, the numpy restatement of the rule in include/vpic_hip.h.

1  BIT FOR BIT with recorded draws: on the 10 x 7 x 3 grid of test_gpu_moments.py (an axis thinner than a tile: the states in
   tile order are made under VPIC_HIP_WINDOW=tile), decks whose cells hold exactly the counts of SAME_COUNTS (within one
   species) and TWO_COUNTS (two species), q drawn from four values (unequal weights: one-sided updates), in six array
   states.  ux, uy, uz of every particle are compared as uint32 with the reference applied to the particles as they lay
   when the kernel ran; every other word is unchanged; a state with exact ranges keeps its order and reports no sort.
2  CONSERVATION with the device's own draws, bounds from the per-pair figures recorded in tests/test_collide_ref.py.
3  THE DISTRIBUTION of the device's draws on two cold counter-streaming beams.
4  Seeds, 5 arguments."""
import contextlib
import functools
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import collide_ref as R  # noqa: E402
from species_states import package, run_child  # noqa: E402
from test_collide_ref import WORST_E, WORST_P  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
GRID = (10, 7, 3)
CAP = R.MAX_CELL
SAME_COUNTS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, CAP]
TWO_COUNTS = [(0, 5), (5, 0), (1, 1), (1, 7), (7, 1), (64, 64), (64, 65), (65, 3), (3, 65), (200, 7), (256, 300), (CAP, 1)]
Q_VALUES = np.array([-0.005, -0.01, -0.02, -0.04], F)           # weights 0.5, 1, 2, 4 at wq = 100
N_TAIL, N_DOOMED = 150, 40
STATES = ["voxel", "tile", "unsorted", "tile_only", "tile_tail_holes", "tile_pushed"]
IN_PLACE = ("voxel", "tile")
TILE_STATES = ("tile", "tile_only", "tile_tail_holes", "tile_pushed")
KINDS = {"one": dict(m_a=1.0, wq_a=100.0), "two_1": dict(m_a=1.0, m_b=1.0, wq_a=100.0, wq_b=100.0),
         "two_1836": dict(m_a=1.0, m_b=1836.0, wq_a=100.0, wq_b=50.0)}
COMMON = dict(cvar=3e-4, dt=0.7, seed=20261019, call=5)


@contextlib.contextmanager
def environment(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def cell_voxels():
    L = importlib.import_module("old-vpic_amd.layout")
    nx, ny, nz = GRID
    x, y, z = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1), indexing="ij")
    return L.voxel(x.ravel(), y.ravel(), z.ravel(), nx, ny, nz)


def cell_counts(kind, limit=CAP, over=False):
    """per species, the particles of every cell: the listed counts (those above `limit` left out) in cells drawn once, 0 to 6
    in the others; over: one more cell at CAP + 1"""
    rng = np.random.default_rng(77)
    cells = rng.permutation(GRID[0] * GRID[1] * GRID[2])
    n_sp = 1 if kind == "one" else 2
    counts = rng.integers(0, 7, (n_sp, len(cells)))
    listed = [(c,) for c in SAME_COUNTS] if kind == "one" else TWO_COUNTS
    for cell, c in zip(cells, listed):
        if max(c) <= limit:
            counts[:, cell] = c
    if over:
        counts[n_sp - 1, cells[len(listed)]] = CAP + 1
    return counts


def make_particles(counts, seed, first_tag=1):
    L = importlib.import_module("old-vpic_amd.layout")
    rng = np.random.default_rng(seed)
    n = int(counts.sum())
    p = np.zeros(n, L.particle_t)
    p["i"] = np.repeat(cell_voxels(), counts)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-0.9, 0.9, n).astype(F)
    for c in ("ux", "uy", "uz"):
        p[c] = (rng.standard_normal(n) * 0.3).astype(F)
    p["q"] = Q_VALUES[rng.integers(0, 4, n)]
    p["tag"] = np.arange(n) + first_tag
    p["tag2"] = rng.integers(1, 1 << 40, n)
    return p


@functools.lru_cache(maxsize=None)
def deck(kind, limit=CAP, over=False):
    """the particle arrays of the deck (one per species), made once and left unchanged"""
    counts = cell_counts(kind, limit, over)
    out = tuple(make_particles(counts[k], 500 + k, 1 + k * 10 ** 6) for k in range(len(counts)))
    for a in out:
        a.setflags(write=False)
    return out


def build(state, arrays, dt=0.02):
    """(engine, [species]) with the arrays in the state asked for.  "tile_tail_holes": N_TAIL of every array's particles are
    appended after the sort (so that the cells hold the deck's counts again), and N_DOOMED extra ones leave through the
    absorbing +x wall in one push with zero fields, which moves nobody else out of his cell and leaves their slots dead.
    "tile_pushed": tile order, then one advance_p in non-zero fields with a step that takes a third of the particles out
    of their cells."""
    V = package()
    L = V.layout
    nx, ny, nz = GRID
    holes = state == "tile_tail_holes"
    kw = dict(pbc=[L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0]) if holes else {}
    grid = V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), F(0.5 if state == "tile_pushed" else dt), **kw)
    with environment(**(dict(VPIC_HIP_WINDOW="tile") if state in TILE_STATES else {})):
        e = V.Engine(grid)
    e.set_vacuum()
    e.load_interpolator()
    sps, tails = [], []
    for k, p in enumerate(arrays):
        p = np.array(p)
        rng = np.random.default_rng(900 + k)
        sp = e.new_species(-1.0, len(p) + N_DOOMED + 4096, 8192)
        if holes:
            pick = rng.permutation(len(p))
            tails.append(p[pick[:N_TAIL]])
            p = p[pick[N_TAIL:]]
            d = np.zeros(N_DOOMED, L.particle_t)
            d["i"] = L.voxel(nx, rng.integers(1, ny + 1, N_DOOMED), rng.integers(1, nz + 1, N_DOOMED), nx, ny, nz)
            d["dx"], d["ux"], d["q"] = 0.99, 3.0, -0.01     # 0.99 + 2 * 0.95 * 0.02 > 1; the others move 0.012 per sigma of u and start 0.1 from their cell's faces
            d["tag"] = np.arange(N_DOOMED) + 10 ** 7
            p = np.concatenate([p, d])
        e.set_particles(sp, p[rng.permutation(len(p))])
        sps.append(sp)
    for sp in sps:
        if state == "voxel":
            e.sort_p(sp)
            assert e.species_order(sp) == "voxel"
        if state in TILE_STATES:
            e.set_sort_order("engine")
            e.sort_p(sp)
            assert e.species_order(sp) == "tile"
            assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0)
    if holes:
        for sp, t in zip(sps, tails):
            e.append_particles(sp, t)
        e.clear_accumulators()
        e.exchange_begin()
        for sp in sps:
            e.advance_p_async(sp)
        e.exchange_pack([0] * 6, [0] * 6, 8192)
        e.exchange_finish([])
        assert e.exchange_flags == 0
        for sp, p in zip(sps, arrays):
            assert e.species_stats(sp)["dead_slots"] == N_DOOMED and e.np(sp) == len(p)
    if state == "tile_pushed":
        fi = np.zeros(e.nv, L.interpolator_t)
        rng = np.random.default_rng(3)
        for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
            fi[c] = (rng.standard_normal(e.nv) * 0.2).astype(F)
        e.set_interpolator(fi)
        e.clear_accumulators()
        for sp in sps:
            assert e.advance_p(sp) == 0
            assert e.species_order(sp) == "tile"                # the bookkeeping still says tile order: the checking pass finds out
    return e, sps


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def by_tag(p, tags):
    """the records of p in the order of `tags`"""
    order = np.argsort(p["tag"], kind="stable")
    at = np.searchsorted(p["tag"][order], tags)
    assert np.array_equal(p["tag"][order][at], tags)
    return p[order][at]


def draws_table(n, seed=4):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0, 2 * np.pi, n)
    return np.stack([rng.standard_normal(n), np.cos(phi), np.sin(phi), rng.uniform(0, 1, n)], 1).astype(F)


def collide_and_compare(e, sps, kind, before, expect_sorted, expect_instance):
    """one recorded-draws call on the species as they are; `before`: their particles before it (any order, by tag)"""
    V = package()
    same = kind == "one"
    table = draws_table(max(e.capacity(sp)[0] for sp in sps) + 16)
    e.set_collide_draws(table)
    e.collide(sps[0], None if same else sps[1], **KINDS[kind], **COMMON)
    st = e.collide_stats()
    after = [e.get_particles(sp) for sp in sps]
    print(kind, st)
    assert st["sorted_first"] == (1 if expect_sorted else 0) and st["instance"] == expect_instance
    lying = []
    for b, a in zip(before, after):
        assert len(a) == len(b)
        if not expect_sorted:
            assert np.array_equal(a["tag"], b["tag"]), "the array order changed"
        b = by_tag(b, a["tag"])                                  # as the particles lay when the kernel ran
        for c in ("dx", "dy", "dz", "i", "q", "tag", "tag2"):
            assert np.array_equal(b[c], a[c]), c
        lying.append(b)
    vol = (F(e.grid.dx) * F(e.grid.dy)) * F(e.grid.dz)
    ua, ub, ref = R.collide(lying[0], None if same else lying[1], sp_a=sps[0], sp_b=None if same else sps[1], volume=vol, draws=table,
                            **KINDS[kind], **COMMON)
    for u, a, name in ((ua, after[0], "a"),) + (() if same else ((ub, after[1], "b"),)):
        got = np.stack([a["ux"], a["uy"], a["uz"]], 1)
        wrong = np.flatnonzero((bits(got) != bits(u)).any(1))
        assert len(wrong) == 0, (name, len(wrong), wrong[:5], got[wrong[:3]], u[wrong[:3]])
    for key in ("cells", "pairs", "skipped", "one_sided", "fullest_cell"):
        assert st[key] == ref[key], (key, st, ref)
    assert ref["pairs"] > 100 and ref["one_sided"] > 10
    changed = sum(int((bits(np.stack([a[c] for c in ("ux", "uy", "uz")], 1)) != bits(np.stack([b[c] for c in ("ux", "uy", "uz")], 1))).any(1).sum())
                  for a, b in zip(after, lying))
    assert changed > ref["pairs"] // 2                           # (the comparison is of momenta that moved)
    return st


def run_state(state, kind, limit=CAP):
    arrays = deck(kind, limit)
    e, sps = build(state, arrays)
    if state == "tile_tail_holes":
        # a download would drop the dead slots and sort: the particles before the call are a twin engine's
        twin, tsps = build(state, arrays)
        before = [twin.get_particles(sp) for sp in tsps]
        twin.close()
    else:
        before = [e.get_particles(sp) for sp in sps]
    fullest = max(int(c.max()) for c in cell_counts(kind, limit))
    group = fullest > 64 or os.environ.get("VPIC_HIP_COLLIDE_INSTANCE", "") == "group"
    order = [e.species_order(sp) for sp in sps]
    st = collide_and_compare(e, sps, kind, before, state not in IN_PLACE, "group" if group else "wave")
    assert st["fullest_cell"] == fullest or state == "tile_pushed"      # (the push moved particles between the cells)
    if state in IN_PLACE or state in TILE_STATES:
        assert [e.species_order(sp) for sp in sps] == order     # a sort the call made is in the order the species was in
        assert all(e.species_stats(sp)["by_tile_only"] == 0 for sp in sps) or state in IN_PLACE
    if state != "unsorted":
        # exact now: a second call collides where the particles lie
        again = [e.get_particles(sp) for sp in sps]
        collide_and_compare(e, sps, kind, again, False, "group" if group else "wave")
    e.close()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("state", [s for s in STATES if s != "tile_only"])
def test_bit_for_bit(state, kind):
    run_state(state, kind)


@pytest.mark.parametrize("kind", ["one", "two_1836"])
def test_bit_for_bit_sorted_by_tile_only(kind):
    run_child(__file__, ["tile_only", kind], 300)


@pytest.mark.parametrize("kind", ["one", "two_1"])
@pytest.mark.parametrize("instance", ["wave", "group"])
@pytest.mark.parametrize("state", IN_PLACE)
def test_both_instances_at_64(state, instance, kind):
    """the deck without its cells above 64: the wavefront instance by choice, the workgroup instance by the knob -- and
    test_bit_for_bit's full deck, whose fullest listed cell below the cap is 65 and up, runs the workgroup instance"""
    with environment(**(dict(VPIC_HIP_COLLIDE_INSTANCE="group") if instance == "group" else {})):
        run_state(state, kind, limit=64)


@pytest.mark.parametrize("kind", ["one", "two_1"])
def test_a_cell_over_the_cap_is_refused_before_anything_is_written(kind):
    V = package()
    arrays = deck(kind, CAP, True)
    e, sps = build("unsorted", arrays)
    e.set_collide_draws(draws_table(max(len(a) for a in arrays)))
    with pytest.raises(V.VpicHipError, match="VPIC_HIP_COLLIDE_MAX_CELL"):
        e.collide(sps[0], None if kind == "one" else sps[1], **KINDS[kind], **COMMON)
    st = e.collide_stats()
    assert st["fullest_cell"] == CAP + 1 and st["pairs"] == 0 and st["instance"] is None and st["sorted_first"] == 1
    for sp, a in zip(sps, arrays):
        got = e.get_particles(sp)
        assert e.species_order(sp) == "voxel"
        assert got.tobytes() == by_tag(np.array(a), got["tag"]).tobytes()
    e.close()


# ---- 2: conservation with the device's own draws ----------------------------------------------------------------------------
def sums(p, m):
    u = np.stack([p["ux"], p["uy"], p["uz"]], 1).astype(np.float64)
    return m * u.sum(0), m * (u * u).sum(), m * np.sqrt((u * u).sum(1).max()), m * (u * u).sum(1).max()


@pytest.mark.parametrize("ratio", [1, 100])
def test_conservation(ratio):
    """equal weights, 32^3 x 64 per cell, drifting Maxwellians: sum of m u per component and of m u^2 in double, before and
    after one call, within K N 2^-24 max|m u| (resp. max m u^2), N the particles, K = 4 x the worst per-pair figure
    recorded in tests/test_collide_ref.py's docstring (WORST_P for the momentum, WORST_E for the energy)."""
    V = package()
    n = 32
    e = V.Engine(V.make_grid(n, n, n, float(n), float(n), float(n), F(0.1)))
    e.set_vacuum()
    masses = [1.0] if ratio == 1 else [1.0, float(ratio)]
    sps = []
    for k, m in enumerate(masses):
        sp = e.new_species(-1.0 / m, n ** 3 * 64 + 4096, 4096)
        e.load_maxwellian(sp, 64, 100 + k, -0.01, u=(0.02, 0.0, 0.01) if k == 0 else (-0.01, 0.01, 0.0), vth=0.05 / np.sqrt(m))
        sps.append(sp)
    before = [e.get_particles(sp) for sp in sps]
    kw = dict(m_a=1.0, wq_a=100.0, cvar=1e-7, dt=1.0, seed=8, call=1)
    if ratio != 1:
        kw.update(m_b=float(ratio), wq_b=100.0, cvar=4e-7)
    e.collide(sps[0], sps[-1], **kw)
    st = e.collide_stats()
    after = [e.get_particles(sp) for sp in sps]
    e.close()
    assert st["pairs"] == (n ** 3 * 32 if ratio == 1 else n ** 3 * 64) and st["skipped"] == 0 and st["one_sided"] == 0 and st["instance"] == "wave"
    N = sum(len(b) for b in before)
    p0 = sum(sums(b, m)[0] for b, m in zip(before, masses)); p1 = sum(sums(a, m)[0] for a, m in zip(after, masses))
    e0 = sum(sums(b, m)[1] for b, m in zip(before, masses)); e1 = sum(sums(a, m)[1] for a, m in zip(after, masses))
    top_p = max(sums(b, m)[2] for b, m in zip(before, masses)); top_e = max(sums(b, m)[3] for b, m in zip(before, masses))
    bound_p, bound_e = 4 * WORST_P * N * 2.0 ** -24 * top_p, 4 * WORST_E * N * 2.0 ** -24 * top_e
    print(f"ratio {ratio}: N {N}, d(sum m u) {p1 - p0} (bound {bound_p:.3e}), d(sum m u^2) {e1 - e0:.3e} (bound {bound_e:.3e}), of {e0:.6e}")
    assert np.abs(p1 - p0).max() <= bound_p and abs(e1 - e0) <= bound_e
    moved = np.mean([(bits(a["ux"]) != bits(by_tag(b, a["tag"])["ux"])).mean() for a, b in zip(after, before)])
    assert moved > 0.99                                          # (something happened)
    da = after[0]; db = by_tag(before[0], da["tag"])
    turn = np.sqrt(((da["ux"] - db["ux"]).astype(np.float64) ** 2 + (da["uy"] - db["uy"]) ** 2 + (da["uz"] - db["uz"]) ** 2).mean())
    assert turn > 1e-3                                           # ... far above rounding: the rms change is a few per cent of vth


# ---- 3: the distribution of the draws ----------------------------------------------------------------------------------------
def beam_statistics(delta2, phi):
    return delta2.mean(), (delta2 ** 2).mean(), np.cos(phi).mean(), np.sin(phi).mean(), (np.cos(phi) * np.sin(phi)).mean()


def assert_draw_statistics(stat, s2, M, what):
    d2, d4, c, s, cs = stat
    print(f"{what}: mean d^2 / s2 - 1 = {d2 / s2 - 1:+.4f} (bound {5 * np.sqrt(2 / M):.4f}), mean d^4 / 3 s2^2 - 1 = {d4 / (3 * s2 * s2) - 1:+.4f} "
          f"(bound {5 * np.sqrt(96 / M) / 3:.4f}), mean cos {c:+.5f}, sin {s:+.5f} (bound {5 / np.sqrt(2 * M):.5f}), cos sin {cs:+.5f} (bound {5 / np.sqrt(8 * M):.5f})")
    assert abs(d2 / s2 - 1) <= 5 * np.sqrt(2 / M)
    assert abs(d4 / (3 * s2 * s2) - 1) <= 5 * np.sqrt(96 / M) / 3
    assert abs(c) <= 5 / np.sqrt(2 * M) and abs(s) <= 5 / np.sqrt(2 * M) and abs(cs) <= 5 / np.sqrt(8 * M)


def test_distribution_of_the_draws():
    """two cold beams +-u0 z of 64 + 64 particles in each of 1024 cells, equal weights and masses: every pair has g = 2 u0
    along z and s2 = 0.01; from every a-particle delta^2 = (1 - cos) / (1 + cos), cos = uz' / u0, and phi from (ux', uy').
    The bounds are five standard errors of the stated distributions at M = 65 536 (sampling bounds, not tolerances of the
    kernel); numpy's own normals at the same M are held to them first."""
    V = package()
    L = V.layout
    M, s2, u0 = 65536, 0.01, 0.05
    rng = np.random.default_rng(2026)
    assert_draw_statistics(beam_statistics(s2 * rng.standard_normal(M) ** 2, rng.uniform(0, 2 * np.pi, M)), s2, M, "numpy")
    nx, ny, nz = 16, 8, 8
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), F(0.1)))
    e.set_vacuum()
    x, y, z = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1), indexing="ij")
    vox = np.repeat(np.sort(L.voxel(x.ravel(), y.ravel(), z.ravel(), nx, ny, nz)), 64)
    sps = []
    for sign in (1.0, -1.0):
        p = np.zeros(M, L.particle_t)
        p["i"], p["uz"], p["q"], p["tag"] = vox, sign * u0, -0.01, np.arange(M) + 1
        sp = e.new_species(-1.0, M + 4096, 4096)
        e.set_particles(sp, p)
        e.sort_p(sp)
        sps.append(sp)
    g = float(F(u0) - F(-u0))
    cvar = s2 * 1.0 * 0.25 * g ** 3 / (1.0 * 64 * 1.0)           # s2 V m_ab^2 g^3 / (w N dt), w = 0.01 x 100
    e.collide(sps[0], sps[1], m_a=1.0, m_b=1.0, wq_a=100.0, wq_b=100.0, cvar=cvar, dt=1.0, seed=31, call=0)
    st = e.collide_stats()
    assert st["pairs"] == M and st["cells"] == 1024 and st["sorted_first"] == 0 and st["instance"] == "wave"
    a = e.get_particles(sps[0])
    b = e.get_particles(sps[1])
    e.close()
    cos_t = a["uz"].astype(np.float64) / float(F(u0))
    assert_draw_statistics(beam_statistics((1 - cos_t) / (1 + cos_t), np.arctan2(a["uy"].astype(np.float64), a["ux"].astype(np.float64))), s2, M, "device")
    for c in ("ux", "uy", "uz"):                                 # equal masses and weights: the pair's momentum stays zero
        assert abs(a[c].astype(np.float64).sum() + b[c].astype(np.float64).sum()) <= 4 * WORST_P * 2 * M * 2.0 ** -24 * u0


# ---- 4: seeds ---------------------------------------------------------------------------------------------------------------
def set_momenta(e, sp, p):
    """the library's test hook: ux, uy, uz of the array as it lies, nothing else (the order and the partition stay)"""
    import ctypes as C
    f = package().lib().vpic_hip_debug_set_momenta              # (a test hook that no header declares: the arguments say their types)
    u = [np.ascontiguousarray(p[c], F) for c in ("ux", "uy", "uz")]
    assert f(e._h, C.c_int(sp), *[x.ctypes.data_as(C.c_void_p) for x in u], C.c_int64(len(p))) == 0


def test_seeds():
    """on ONE array (a sort places the particles of a cell in no fixed order, so the momenta are put back between the calls
    instead of uploading again): the same seed and call twice give the same bits, another call other momenta for at least
    99 % of the paired particles, and set_collide_draws(None) really switches back to the counter stream"""
    kind = "two_1"
    arrays = deck(kind, 64)
    e, sps = build("voxel", arrays)
    start = [e.get_particles(sp) for sp in sps]
    kw = dict(KINDS[kind], **COMMON)
    mom = lambda ps: np.concatenate([bits(np.stack([p[c] for c in ("ux", "uy", "uz")], 1)) for p in ps])   # noqa: E731

    def run(call, table=None):
        for sp, p in zip(sps, start):
            set_momenta(e, sp, p)
        assert np.array_equal(mom([e.get_particles(sp) for sp in sps]), mom(start))
        if table is not None:
            e.set_collide_draws(table)
        e.collide(sps[0], sps[1], **dict(kw, call=call))
        st = e.collide_stats()
        assert st["sorted_first"] == 0 and st["instance"] == "wave"
        return mom([e.get_particles(sp) for sp in sps]), st["pairs"]

    first, paired = run(5)
    again, _ = run(5)
    other, _ = run(6)
    with_table, _ = run(5, draws_table(max(len(a) for a in arrays)))
    e.set_collide_draws(None)
    back, _ = run(5)
    e.close()
    assert np.array_equal(first, again)
    assert np.array_equal(first, back) and not np.array_equal(first, with_table)
    was_paired = (first != mom(start)).any(1)
    assert was_paired.sum() >= paired
    assert ((first != other).any(1))[was_paired].mean() >= 0.99


# ---- 5: arguments -----------------------------------------------------------------------------------------------------------
def test_arguments():
    V = package()
    arrays = deck("two_1", 64)
    e, sps = build("voxel", arrays)
    before = [e.get_particles(sp) for sp in sps]
    good = dict(KINDS["two_1"], **COMMON)

    def refused(name, sp_a=sps[0], sp_b=sps[1], **change):
        with pytest.raises(V.VpicHipError, match=name):
            e.collide(sp_a, sp_b, **dict(good, **change))

    refused("sp_a", sp_a=7)
    refused("sp_b", sp_b=-1)
    refused("m_a", m_a=0.0)
    refused("m_b", m_b=-1.0)
    refused("wq_a", wq_a=0.0)
    refused("wq_b", wq_b=float("nan"))
    refused("cvar", cvar=-1e-9)
    refused("dt", dt=-0.1)
    e.set_collide_draws(draws_table(max(len(a) for a in arrays) - 1))
    refused("draws")
    e.set_collide_draws(None)
    for sp, b in zip(sps, before):
        assert e.get_particles(sp).tobytes() == b.tobytes() and e.species_order(sp) == "voxel"
    e.collide(sps[0], sps[1], **good)                            # ... and the good call goes through
    assert e.collide_stats()["pairs"] > 0
    e.close()


if __name__ == "__main__":
    with environment(VPIC_HIP_WINDOW="tile"):
        run_state(sys.argv[1], sys.argv[2])
    print("child OK")
