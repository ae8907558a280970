"""vpic_hip_species_load_profile on the device against tests/load_ref.py, the numpy restatement of THE RULE in
include/vpic_hip.h.

1  PARITY with recorded draws (vpic_hip_set_load_draws): every word of every particle, partition[], counts and order, over
   the grids, totals, broadcast shapes, NULL tables, flags and empty cells of the issue.
2  GENERATOR mode: positions, voxels, q, tags and order == the reference (Philox and float arithmetic only); cold cells
   give the drift exactly; the normals' moments within 6 standard errors; no two particles at one position; the same call
   twice the same bits, another stream other particles in every cell.
3  ANY DECOMPOSITION: the union of the pieces == the whole, momenta included.
4  APPEND, 5 BOOKKEEPING (twin engines stepped side by side), 6 REFUSALS (nothing touched)."""
import contextlib
import ctypes as C
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

import load_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
WORDS = ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q", "tag", "tag2")


def package():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


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


def engine(dims, tile=False, dt=0.02):
    V = package()
    nx, ny, nz = dims
    with environment(**(dict(VPIC_HIP_WINDOW="tile") if tile else {})):
        e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), F(dt)))
    e.set_vacuum()
    e.load_interpolator()
    if tile:
        e.set_sort_order("engine")
    return e


def same_bits(a, b, names=WORDS):
    return [n for n in names if not np.array_equal(a[n].view("u%d" % a[n].dtype.itemsize), b[n].view("u%d" % b[n].dtype.itemsize))]


def draw_table(n, seed=5):
    """float32[n, 7]: positions from every 24-bit draw's range, standard normals, U small half of the time (so that cold and
    slow cells flip too)"""
    rng = np.random.default_rng(seed)
    d = np.empty((n, 7), F)
    d[:, :3] = R.unit_open(rng.integers(0, 1 << 32, (n, 3)).astype(np.uint32))
    d[:, 3:6] = rng.standard_normal((n, 3)).astype(F)
    d[:, 6] = R.unit_open(rng.integers(0, 1 << 32, n).astype(np.uint32)) * np.where(rng.random(n) < 0.5, F(1e-3), F(1))
    return d


def tables(dims, shape, seed, total=None, nulls=()):
    """count, q, ud, uth of the given [tz, ty, tx] shape: counts 0 .. 5 (or adding up to `total`), the first and the last
    entry 0, q of two signs and 0, drifts of both signs with cells at rest, spreads with cold cells"""
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    if total is None:
        count = rng.integers(0, 6, size)
    else:
        count = rng.multinomial(total, np.full(size, 1.0 / size)) if size > 2 else np.array([total] + [0] * (size - 1))
    if size > 2 and total is None:
        count[0] = count[-1] = 0
    q = rng.choice(np.array([-0.5, 0.25, 0.0, -0.125], F), size)
    ud = [np.where(rng.random(size) < 0.2, 0, rng.standard_normal(size) * 0.8).astype(F).reshape(shape) for _ in range(3)]
    uth = [np.where(rng.random(size) < 0.2, 0, rng.uniform(0, 0.7, size)).astype(F).reshape(shape) for _ in range(3)]
    for k in nulls:
        (ud if k < 3 else uth)[k % 3] = None
    return count.astype(np.int32).reshape(shape), q.reshape(shape), (None if all(t is None for t in ud) else ud), (None if all(t is None for t in uth) else uth)


def check_parity(dims, count, q, ud, uth, flip=False, tags=None):
    n = int(R.table(count, dims).sum())
    draws = draw_table(n + 3)
    e = engine(dims)
    sp = e.new_species(-1.0, n + 100, 64)
    e.set_load_draws(draws)
    loaded = e.load_profile(sp, count, q, ud, uth, seed=1, flip=flip, tags=tags)
    ref, part, _, _ = R.load(dims, count, q, ud, uth, flip=flip, tag0=tags, draws=draws)
    assert loaded == n == e.np(sp) == len(ref) and e.capacity(sp)[0] == n
    assert e.species_order(sp) == "voxel"
    assert np.array_equal(e.get_partition(sp), part)
    got = e.get_particles(sp)
    assert same_bits(got, ref) == []
    return got


# ---- 1 parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [0, 1, 255, 256, 257, 70000])
def test_parity_totals(total):
    """8 x 6 x 5 cells, every table of the grid's shape, FLIP and TAGS on"""
    dims = (8, 6, 5)
    got = check_parity(dims, *tables(dims, (5, 6, 8), 10 + total % 7, total=total), flip=True, tags=1000)
    assert len(got) == total


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 3, 2), (8, 6, 5)])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("tags", [None, 1 << 40])
def test_parity_grids_and_flags(dims, flip, tags):
    got = check_parity(dims, *tables(dims, dims[::-1], 3), flip=flip, tags=tags)
    if flip and dims == (8, 6, 5):                                # the flag matters: the unflipped load differs
        plain = check_parity(dims, *tables(dims, dims[::-1], 3), flip=False, tags=tags)
        assert same_bits(got, plain) != [] and same_bits(got, plain, ("dx", "dy", "dz", "i", "q")) == []


def test_parity_long_empty_run_and_one_cell_over_four_workgroups():
    """300 x 1 x 1: 299 empty cells, then one cell of 1000 particles"""
    dims = (300, 1, 1)
    count = np.zeros((1, 1, 300), np.int32)
    count[0, 0, 299] = 1000
    rng = np.random.default_rng(8)
    ud = [rng.standard_normal((1, 1, 300)).astype(F) for _ in range(3)]
    got = check_parity(dims, count, -0.25, ud, (F(0.3), F(0.1), F(0.2)), flip=True, tags=7)
    assert len(got) == 1000 and np.all(got["i"] == 300 + 302 * (1 + 3))
    count[0, 0, 0] = 3                                            # ... and a cell at the other end of the run
    assert len(check_parity(dims, count, -0.25, ud, (F(0.3), F(0.1), F(0.2)))) == 1003


@pytest.mark.parametrize("shape", [(tz, ty, tx) for tz in (1, 5) for ty in (1, 6) for tx in (1, 8)])
def test_parity_every_broadcast_shape(shape):
    dims = (8, 6, 5)
    check_parity(dims, *tables(dims, shape, 40 + sum(shape)), flip=True, tags=5)


@pytest.mark.parametrize("nulls", [(0, 1, 2, 3, 4, 5), (0, 1, 2), (3, 4, 5), (1, 5), (0, 2, 3)])
def test_parity_null_tables(nulls):
    dims = (5, 3, 2)
    count, q, ud, uth = tables(dims, (2, 3, 5), 77, nulls=nulls)
    got = check_parity(dims, count, q, ud, uth, flip=True)
    if len(nulls) == 6:
        assert not got["ux"].any() and not got["uy"].any() and not got["uz"].any()


def test_parity_scalars_and_mixed_shapes():
    """scalars, and tables that broadcast against each other to one tdim (a Harris profile is (nz, 1, 1))"""
    dims = (8, 6, 5)
    z = np.arange(5).reshape(5, 1, 1)
    got = check_parity(dims, 3, F(-0.5), (np.cos(z).astype(F), np.sin(z).astype(F), None), (F(0.2), F(0.2), F(0.2)), tags=1)
    assert len(got) == 3 * 240
    check_parity(dims, (z % 3).astype(np.int32), np.where(np.arange(8) % 2, F(1), F(-1)).reshape(1, 1, 8), None, None)


# ---- 2 generator mode ----------------------------------------------------------------------------------------------------------
EXACT = ("dx", "dy", "dz", "i", "q", "tag", "tag2")


def test_generator_positions_voxels_charges_tags_and_order():
    dims = (8, 6, 5)
    count, q, ud, uth = tables(dims, (5, 6, 8), 21)
    count[2, 3, 4] = 700                                          # j beyond one workgroup
    e = engine(dims)
    sp = e.new_species(-1.0, 4096, 64)
    n = e.load_profile(sp, count, q, ud, uth, seed=0xdeadbeef, stream=3, global_dims=(100000, 70000, 9), offset=(99992, 5, 4), tags=11)
    ref, part, cell, _ = R.load(dims, count, q, ud, uth, seed=0xdeadbeef, stream=3, global_dims=(100000, 70000, 9), offset=(99992, 5, 4), tag0=11)
    assert int(cell.max()) > 1 << 32
    got = e.get_particles(sp)
    assert n == len(ref) == len(got) and same_bits(got, ref, EXACT) == []
    assert np.array_equal(e.get_partition(sp), part)
    # the momenta: the reference's normals are numpy's, the device's its own -- close, not equal.  Two float libraries agree
    # on log, sin and cos to a few 2^-24 of a radius of at most 6, times uth <= 0.7 and the boost's factor (|D| <= 4 here):
    # below 1e-4 absolute with room to spare; no flip in this call, so no decision can fall the other way
    for c in ("ux", "uy", "uz"):
        assert np.allclose(got[c], ref[c], rtol=1e-3, atol=1e-4)


def test_generator_cold_cells_carry_the_drift_exactly():
    dims = (5, 3, 2)
    count, q, ud, _ = tables(dims, (2, 3, 5), 31)
    for flip in (False, True):
        e = engine(dims)
        sp = e.new_species(-1.0, 4096, 64)
        e.load_profile(sp, count + 20, q, ud, (F(0), F(0), F(0)), seed=4, flip=flip)
        got = e.get_particles(sp)
        cells = np.repeat(np.arange(30), (count + 20).ravel())
        for k, c in enumerate(("ux", "uy", "uz")):
            assert np.array_equal(got[c], ud[k].ravel()[cells])


@pytest.fixture(scope="module")
def hot():
    """8 x 6 x 5 cells at 512 particles each, at rest, uth = (0.3, 0.5, 0.2): twice with one stream, once with another"""
    dims, uth = (8, 6, 5), (F(0.3), F(0.5), F(0.2))
    e = engine(dims)
    sp = e.new_species(-1.0, 240 * 512, 64)
    out = []
    for stream in (0, 0, 1):
        assert e.load_profile(sp, 512, F(-1.0 / 512), None, uth, seed=2026, stream=stream) == 240 * 512
        out.append(e.get_particles(sp))
    return uth, out


def test_generator_moments_of_the_normals(hot):
    """mean 0 within 6 sigma / sqrt(N); variance sigma^2 within 6 sigma^2 sqrt(2 / N) (the variance of a normal's square is 2)"""
    uth, (p, _, _) = hot
    n = len(p)
    for k, c in enumerate(("ux", "uy", "uz")):
        x = p[c].astype(np.float64) / float(uth[k])
        print("%s: mean %.5f (bound %.5f), variance - 1 %.5f (bound %.5f)" % (c, x.mean(), 6 / np.sqrt(n), (x * x).mean() - 1, 6 * np.sqrt(2.0 / n)))
        assert abs(x.mean()) <= 6 / np.sqrt(n)
        assert abs((x * x).mean() - 1) <= 6 * np.sqrt(2.0 / n)
    assert abs(np.mean(p["ux"].astype(np.float64) * p["uy"]) / float(uth[0] * uth[1])) <= 6 / np.sqrt(n)     # n0 and n1 share a radius


def test_generator_no_two_particles_at_one_position(hot):
    p = hot[1][0]
    pos = np.stack([p["dx"], p["dy"], p["dz"]], axis=1).view(np.uint32)
    assert len(np.unique(pos, axis=0)) == len(p)


def test_generator_same_call_same_bits_other_stream_other_particles(hot):
    first, again, other = hot[1]
    assert same_bits(first, again) == []
    for c in ("dx", "ux"):
        a, b = first[c].reshape(240, 512), other[c].reshape(240, 512)
        assert (a != b).mean(axis=1).min() > 0.99                 # every cell


# ---- 3 any decomposition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [(2, 1, 1), (1, 1, 2), (2, 2, 1)])
def test_any_decomposition(cut):
    whole = (8, 6, 4)
    count, q, ud, uth = tables(whole, (4, 6, 8), 91)
    count[1, 2, 3] = 300
    kw = dict(seed=77, stream=2, flip=True)
    e = engine(whole)
    sp = e.new_species(-1.0, 8192, 64)
    e.load_profile(sp, count, q, ud, uth, **kw)
    ref = e.get_particles(sp)
    _, _, ref_cell, ref_j = R.load(whole, count, q, seed=0)
    order = np.lexsort((ref_j, ref_cell))
    dims = tuple(w // c for w, c in zip(whole, cut))
    pieces, cells, js = [], [], []
    for kz in range(cut[2]):
        for ky in range(cut[1]):
            for kx in range(cut[0]):
                off = (kx * dims[0], ky * dims[1], kz * dims[2])
                sl = (slice(off[2], off[2] + dims[2]), slice(off[1], off[1] + dims[1]), slice(off[0], off[0] + dims[0]))
                cut_ = lambda t: None if t is None else [a[sl] for a in t]
                ed = engine(dims)
                spd = ed.new_species(-1.0, 8192, 64)
                ed.load_profile(spd, count[sl], q[sl], cut_(ud), cut_(uth), global_dims=whole, offset=off, **kw)
                p = ed.get_particles(spd)
                _, _, cell, j = R.load(dims, count[sl], q[sl], seed=0, global_dims=whole, offset=off)
                # the voxel is the piece's own: as a global cell it is the key
                x, y, z = p["i"] % (dims[0] + 2) - 1, p["i"] // (dims[0] + 2) % (dims[1] + 2) - 1, p["i"] // ((dims[0] + 2) * (dims[1] + 2)) - 1
                assert np.array_equal(cell, ((off[0] + x) + whole[0] * ((off[1] + y) + whole[1] * (off[2] + z))).astype(np.uint64))
                pieces.append(p); cells.append(cell); js.append(j)
    union, cell, j = np.concatenate(pieces), np.concatenate(cells), np.concatenate(js)
    uorder = np.lexsort((j, cell))
    assert np.array_equal(cell[uorder], ref_cell[order]) and np.array_equal(j[uorder], ref_j[order])
    assert same_bits(union[uorder], ref[order], ("dx", "dy", "dz", "ux", "uy", "uz", "q")) == []


# ---- 4 append ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [False, True])
def test_append_a_sheet_behind_a_background(tile):
    dims = (8, 6, 5)
    z = np.arange(5).reshape(5, 1, 1)
    bg = dict(count=4, q=F(-0.25), ud=None, uth=(F(0.1), F(0.1), F(0.1)))
    sheet = dict(count=np.array([0, 3, 9, 3, 0], np.int32).reshape(5, 1, 1), q=F(-0.5),
                 ud=(np.cos(z).astype(F), np.sin(z).astype(F), None), uth=(F(0.3), F(0.3), F(0.3)))
    n0, n1 = 4 * 240, 15 * 48
    draws = draw_table(n0)
    e, twin = engine(dims, tile), engine(dims, tile)
    sp, spt = e.new_species(-1.0, 4096, 4096), twin.new_species(-1.0, 4096, 4096)
    for eng, s in ((e, sp), (twin, spt)):
        eng.set_load_draws(draws)
        assert eng.load_profile(s, bg["count"], bg["q"], bg["ud"], bg["uth"], seed=1, tags=1) == n0
        if tile:
            eng.sort_p(s)
            assert eng.species_order(s) == "tile"
    before = e.get_particles(sp)
    assert e.load_profile(sp, sheet["count"], sheet["q"], sheet["ud"], sheet["uth"], seed=2, flip=True, tags=10 ** 6, append=True) == n1
    ref = R.load(dims, sheet["count"], sheet["q"], sheet["ud"], sheet["uth"], flip=True, tag0=10 ** 6, draws=draws)[0]
    got = e.get_particles(sp)
    assert len(got) == n0 + n1 == e.np(sp)
    assert same_bits(got[:n0], before) == []                      # the first population: untouched
    assert same_bits(got[n0:], ref) == []                         # the second: behind the extent, in the call's order
    # orders and counts as append_particles leaves them
    twin.append_particles(spt, ref)
    assert e.species_order(sp) == twin.species_order(spt) == ("tile" if tile else "none")
    assert e.capacity(sp) == twin.capacity(spt) and same_bits(twin.get_particles(spt), got) == []
    if tile:
        assert np.array_equal(e.get_tile_partition(sp), twin.get_tile_partition(spt))
    for eng, s in ((e, sp), (twin, spt)):
        eng.set_accumulation("deterministic")
        eng.sort_p(s)
        for step in range(3):
            eng.step(step, 0)
        eng.sync()
    a, b = e.get_particles(sp), twin.get_particles(spt)
    assert len(a) == n0 + n1 and np.array_equal(np.sort(a["tag"]), np.sort(got["tag"]))
    ka, kb = np.argsort(a["tag"]), np.argsort(b["tag"])
    assert same_bits(a[ka], b[kb]) == [] and np.all(np.isfinite(a["ux"]))
    # an append without tags into a species that has them: the new particles' tags read 0
    assert e.load_profile(sp, 1, F(-0.25), seed=3, append=True) == 240
    assert not e.get_particles(sp)["tag"][n0 + n1:].any() and e.np(sp) == n0 + n1 + 240


# ---- 5 bookkeeping -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("charged", [True, False])
def test_bookkeeping_is_that_of_an_uploaded_species(charged):
    """engine A after load_profile, engine B after set_particles of A's particles: three steps in deterministic accumulation
    with a non-zero field leave the same particles and fields"""
    dims = (8, 6, 5)
    count, q, ud, uth = tables(dims, (5, 6, 8), 55)
    q = np.where(q == 0, F(0.25), q) * F(0.01) if charged else F(0)
    L = package().layout
    rng = np.random.default_rng(9)
    f = np.zeros(L.nv(*dims), L.field_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        f[c] = (rng.standard_normal(len(f)) * 0.05).astype(F)
    out = []
    for k in range(2):
        e = engine(dims, dt=0.3)
        e.set_accumulation("deterministic", 0.01)
        sp = e.new_species(-1.0, 4096, 4096)
        if k == 0:
            e.load_profile(sp, count + 1, q, ud, uth, seed=5)
            loaded = e.get_particles(sp)
            assert (loaded["q"] == 0).all() == (not charged)
        else:
            e.set_particles(sp, loaded)
        e.set_fields(f)
        e.load_interpolator()
        for step in range(3):
            e.step(step, 0)
        e.sync()
        out.append((e.get_particles(sp), e.get_fields()))
    assert len(out[0][0]) == len(out[1][0]) == len(loaded)
    assert same_bits(out[0][0], out[1][0]) == []
    assert same_bits(out[0][1], out[1][1], [n for n in L.field_t.names]) == []
    assert np.any(out[0][1]["jfx"] != 0) == charged                # the chargeless path deposits nothing


def test_collide_finds_exact_ranges_without_sorting():
    dims = (8, 6, 5)
    e = engine(dims)
    sp = e.new_species(-1.0, 8192, 64)
    e.load_profile(sp, 16, F(-0.01), None, (F(0.3), F(0.3), F(0.3)), seed=1)
    before = e.get_particles(sp)
    e.collide(sp, m_a=1.0, wq_a=100.0, cvar=3e-4, dt=0.7, seed=1, call=0)
    stats = e.collide_stats()
    assert stats["sorted_first"] == 0 and stats["pairs"] == 8 * 240
    after = e.get_particles(sp)
    assert same_bits(after, before, ("dx", "dy", "dz", "i", "q")) == [] and same_bits(after, before, ("ux",)) != []


# ---- 6 refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    V = package()
    L = V.layout
    dims = (5, 3, 2)
    e = engine(dims)
    sp = e.new_species(-1.0, 1000, 64)
    count, q, ud, uth = tables(dims, (2, 3, 5), 13)
    assert e.load_profile(sp, count, q, ud, uth, seed=1, tags=9) > 0
    before, part = e.get_particles(sp), e.get_partition(sp)

    def untouched():
        assert e.species_order(sp) == "voxel" and e.np(sp) == len(before) and e.capacity(sp)[0] == len(before)
        assert same_bits(e.get_particles(sp), before) == [] and np.array_equal(e.get_partition(sp), part)

    def refused(match, *args, **kw):
        with pytest.raises(V.VpicHipError, match=match):
            e.load_profile(*args, **dict(dict(seed=1), **kw))
        untouched()

    bad = lambda t, v: np.where(np.arange(30).reshape(2, 3, 5) == 17, v, t).astype(t.dtype)
    refused("sp = 7", 7, count, q, ud, uth)
    refused("sp = -1", -1, count, q, ud, uth)
    refused(r"tdim\[0\] = 4", sp, count[:, :, :4], q[:, :, :4])
    refused(r"tdim\[1\] = 2", sp, count[:, :2], q[:, :2])
    refused(r"tdim\[2\] = 3", sp, np.zeros((3, 1, 1), np.int32), F(1))
    refused(r"goff\[0\]", sp, count, q, global_dims=(9, 3, 2), offset=(5, 0, 0))
    refused(r"goff\[2\]", sp, count, q, global_dims=(9, 3, 2), offset=(0, 0, 1))
    refused(r"goff\[1\] = -1 is negative", sp, count, q, global_dims=(9, 9, 9), offset=(0, -1, 0))
    refused(r"count\[17\] = -2 is negative", sp, bad(count, -2), q)
    refused(r"q\[17\] is not finite", sp, count, bad(q, np.inf))
    refused(r"ud\[1\]\[17\] is not finite", sp, count, q, (ud[0], bad(ud[1], np.nan), ud[2]), uth)
    refused(r"uth\[2\]\[17\] is not finite", sp, count, q, ud, (uth[0], uth[1], bad(uth[2], np.inf)))
    refused(r"uth\[0\]\[17\] = -0.5 is negative", sp, count, q, ud, (bad(uth[0], -0.5), uth[1], uth[2]))
    refused("more than 2\\^31 - 1", sp, 1 << 30, F(1))
    refused("exceed max_np", sp, 34, F(1))                        # 1020 particles into 1000 slots
    assert len(before) > 40
    refused("exceed max_np", sp, 32, F(1), append=True)           # 960 more behind them
    e.set_load_draws(draw_table(int(count.sum()) - 1))
    refused("draws table holds", sp, count, q, ud, uth)
    e.set_load_draws(None)
    pm = np.zeros(1, L.particle_mover_t)
    pm["i"] = 3
    e.set_movers(sp, pm)
    refused("pending movers", sp, count, q, ud, uth)
    e.set_movers(sp, pm[:0])

    # what Engine.load_profile cannot express: NULL arguments and unknown flag bits, through the C ABI itself
    lib = V.lib()
    cnt, qq = np.ascontiguousarray(count), np.ascontiguousarray(q)

    def raw(match, null_d=False, **fields):
        d = np.zeros(1, L.load_t)
        d["count"], d["q"], d["tdim"], d["gdim"], d["seed"] = cnt.ctypes.data, qq.ctypes.data, (5, 3, 2), (5, 3, 2), 1
        for k, v in fields.items():
            d[k] = v
        n = C.c_int64(-5)
        assert lib.vpic_hip_species_load_profile(e._h, sp, None if null_d else d.ctypes.data_as(C.c_void_p), C.byref(n)) != 0
        assert match in lib.vpic_hip_last_error().decode() and n.value == -5
        untouched()

    raw("d is NULL", null_d=True)
    raw("count is NULL", count=0)
    raw("q is NULL", q=0)
    raw("flags = 8 has unknown bits", flags=8)
    raw("flags = 65 has unknown bits", flags=65)
    # ... and the call still works afterwards
    assert e.load_profile(sp, count, q, ud, uth, seed=1, tags=9) == len(before)
    untouched()
