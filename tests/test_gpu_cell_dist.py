"""vpic_hip_cell_distribution on the GPU against the numpy restatement of test_cell_dist_ref.py: EXACT equality of every
count, every int64 sum, every refusal count and the statistics.  The sums are integers of values that both sides round
identically (test_cell_dist_ref.py says why), so there is no tolerance and no excluded cell -- a difference is a bug.

Inputs: the field chain's fields (oracle.field_chain.inputs: random in every component, ghosts included, so that a wrong
neighbour offset shows) and a seeded random hydro array, on six of its grids -- (1,1,6) and (3,1,1) with axes one cell
thick, (6,5,4), (67,3,2) whose x extent crosses a wavefront, (33,17,9) and (130,9,65): 76 050 cells over many workgroups
with a ragged last one.  Descriptors: test_cell_dist_ref.cases."""
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

from oracle import field_chain as FC  # noqa: E402
from species_states import package  # noqa: E402
from test_cell_dist_ref import (GLOBAL, GRIDS, HAND_CASES, HAND_DIMS, REFUSING, cases, cell_distribution_ref, generated_fields,  # noqa: E402
                                generated_hydro, handmade_grid, interior, reference_of_the_inputs)

pytestmark = pytest.mark.gpu
L = importlib.import_module("old-vpic_amd.layout")


def engine(V, dims, f=None, h=None):
    e = V.Engine(V.make_grid(*dims, *FC.box(dims), FC.DT))
    if f is not None:
        e.set_fields(f)
    if h is not None:
        e.set_hydro(h)
    return e


def call(e, desc, values):
    r = e.cell_distribution(desc["axes"], values, desc.get("select", ()))
    return r, e.cell_distribution_stats()


def check(name, r, stats, want, values, in_lds):
    want_counts, want_isums, want_refused, want_stats = want
    print(f"({name}): seen {stats[0]} kept {stats[1]} counted {stats[2]} through global memory {stats[3]} refused {stats[4:]}; "
          f"expected {want_stats} refused {list(want_refused)}, differing sums "
          f"{int((r.isums != want_isums).sum()) if r.isums.shape == want_isums.shape else 'shape'}, differing counts {int((r.counts != want_counts).sum())}")
    assert r.isums.dtype == np.int64 and r.isums.shape == want_isums.shape and r.counts.dtype == np.uint64
    assert np.array_equal(r.counts, want_counts), name
    assert np.array_equal(r.isums, want_isums), name
    assert np.array_equal(r.refused, want_refused) and r.refused.dtype == np.int64, name
    assert stats[:3] == want_stats and int(r.counts.sum()) == stats[2], name
    assert list(stats[4:4 + len(values)]) == list(want_refused) and not any(stats[4 + len(values):]), name
    assert stats[3] == (0 if in_lds else stats[2]), name
    quanta = np.array([q for _, q in values]).reshape((-1,) + (1,) * (r.isums.ndim - 1))
    assert r.sums.dtype == np.float64 and np.array_equal(r.sums, r.isums * quanta), name


@pytest.mark.parametrize("dims", GRIDS, ids=FC.grid_name)
def test_cells_equal_the_restatement_exactly(dims):
    V = package()
    f, h = generated_fields(dims), generated_hydro(dims)
    e = engine(V, dims, f, h)
    e.load_interpolator()
    before = (e.get_fields().tobytes(), e.get_hydro().tobytes(), e.get_interpolator().tobytes())
    want = reference_of_the_inputs(dims)
    got = {}
    for name, (desc, values) in cases(dims).items():
        r, stats = call(e, desc, values)
        again, stats_again = call(e, desc, values)
        for a, b in zip(r, again):
            assert a.tobytes() == b.tobytes(), name                           # two calls: identical bytes
        assert stats == stats_again, name
        got[name] = (r, stats)
    # fields, hydro and interpolator are left exactly as they were
    assert (e.get_fields().tobytes(), e.get_hydro().tobytes(), e.get_interpolator().tobytes()) == before
    assert before[0] == f.tobytes()
    e.close()
    for name, (desc, values) in cases(dims).items():
        r, stats = got[name]
        check(name, r, stats, want[name], values, name not in GLOBAL)
        assert (stats[4] > 0) == (name == REFUSING and int(want[name][2][0]) > 0), name
    for a, b in (("edge_lds", "edge_global"), ("edge_lds1", "edge_global1")):     # identical totals on either side of the budget
        assert np.array_equal(got[a][0].isums.sum(axis=-1), got[b][0].isums.sum(axis=-1)) and got[a][1][2] == got[b][1][2] == int(np.prod(dims))
        assert got[a][1][3] == 0 and got[b][1][3] == got[b][1][2]
    if "map2d" in got:
        assert got["map2d"][1][3] == got["map2d"][1][2] == int(np.prod(dims))
    # the refusals of one value leave the other alone: "one" counts every cell of its row
    r = got[REFUSING][0]
    assert np.array_equal(r.isums[1].astype(np.uint64), r.counts)


def test_handmade_grid_uploaded():
    """the 2 x 2 x 2 grid of test_cell_dist_ref.py: ties both ways, t at 2^32 and just below, negative values, the NaN of a
    cell without B, coordinates on a bin edge and on hi; in LDS and -- the same values over more bins -- through global memory"""
    V = package()
    f, h = handmade_grid()
    e = engine(V, HAND_DIMS, f, h)
    wide = [(dict(axes=[("rhob", -1.0, 2.0, 1), ("rhof", -0.5, 0.001, 2000)]), HAND_CASES[0][1]),   # 2000 bins x 9 words: global adds
            (dict(axes=[("b_c", 0.0, 0.001, 8500)], select=[("e_par_c", -1.0, 1.0)]), [])]
    for desc, values in HAND_CASES + wide:
        r, stats = call(e, desc, values)
        check(str(desc), r, stats, cell_distribution_ref(f, h, HAND_DIMS, desc, values), values, (desc, values) not in wide)
    r, stats = call(e, *HAND_CASES[0])
    assert int(r.isums[0, 0]) == 2 - 2 + (2 ** 32 - 256) + 3 + 4 and list(r.refused) == [1, 1, 0, 0] and stats == (8, 8, 8, 0, 1, 1, 0, 0)
    assert int(r.isums[1, 0]) == 5 and int(r.isums[2, 0]) == 25 and int(r.isums[3, 0]) == -1152
    e.close()


def test_centred_fields_reproduce_the_loaded_interpolator():
    """One bin per cell (x by z, row by row in y) and a quantum of which every centred field is a whole multiple: the sums
    ARE the fields at the cells' centres, and equal the interpolator the engine has just loaded from the same fields."""
    V = package()
    dims = (6, 5, 4)
    nx, ny, nz = dims
    rng = np.random.default_rng(20261019)
    f = np.zeros(L.nv(*dims), L.field_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz", "jfx", "jfy", "jfz"):
        f[c] = (rng.integers(-1024, 1025, len(f)) / 64.0).astype(np.float32)  # multiples of 2^-6: their means of four are multiples of 2^-8
    e = engine(V, dims, f)
    e.load_interpolator()
    fi = e.get_interpolator()
    v = interior(dims)[3].reshape(nz, ny, nx)
    names = ("ex_c", "ey_c", "ez_c", "bx_c", "by_c", "bz_c")
    members = ("ex", "ey", "ez", "cbx", "cby", "cbz")
    quantum = 2.0 ** -8
    for half in (names[:3], names[3:]):
        for j in range(ny):
            r = e.cell_distribution([("x", 0.0, 1.0, nx), ("z", 0.0, 1.0, nz)], [((n,), quantum) for n in half], [("y", float(j), float(j + 1))])
            assert np.all(r.counts == 1) and not r.refused.any() and e.cell_distribution_stats()[:3] == (nx * ny * nz, nx * nz, nx * nz)
            for k, n in enumerate(half):
                want = fi[members[names.index(n)]][v[:, j, :]]
                assert np.array_equal(r.sums[k], want.astype(np.float64)) and np.any(want != 0), (n, j)
    e.close()


def test_two_boxes_that_partition_the_domain_add_to_the_whole():
    V = package()
    dims = (33, 17, 9)
    e = engine(V, dims, generated_fields(dims), generated_hydro(dims))
    axes = [("b_c", 0.0, 0.05, 60), ("y", 0.0, 1.0, dims[1])]
    values = [(("jdote_c",), 2.0 ** -24), (("hydro.rho", "e_c"), 2.0 ** -24), (("one",), 1.0)]
    whole = e.cell_distribution(axes, values)
    n_whole = e.cell_distribution_stats()
    low = e.cell_distribution(axes, values, [("x", 0.0, 13.0)])
    n_low = e.cell_distribution_stats()
    high = e.cell_distribution(axes, values, [("x", 13.0, 33.0)])
    n_high = e.cell_distribution_stats()
    e.close()
    assert np.array_equal(low.counts + high.counts, whole.counts) and np.array_equal(low.isums + high.isums, whole.isums)
    assert low.counts.any() and high.counts.any() and whole.isums[0].any() and whole.isums[1].any()
    assert n_low[1] == 13 * 17 * 9 and n_high[1] == 20 * 17 * 9 and n_whole[1] == 33 * 17 * 9
    assert n_low[2] + n_high[2] == n_whole[2] and not whole.refused.any()


def test_argument_errors():
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    dims = (4, 4, 4)
    e = engine(V, dims, FC.inputs(dims)["f"])
    SENTINEL_C, SENTINEL_S = np.uint64(0xabcdef), np.int64(-77)
    counts, sums = np.full(1 << 16, SENTINEL_C, np.uint64), np.full(4 << 16, SENTINEL_S, np.int64)
    cp, sp_ = counts.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)
    ok_axes, ok_values = [("ex", -4.0, 2.0, 4)], [(("jdote_c", "rhof"), 1e-6)]

    def run(axes=ok_axes, select=(), values=ok_values, counts_ptr=cp, sums_ptr=sp_, patch=None, patch_v=None, n_val=None, null_d=False, null_v=False):
        d = eng.cell_dist_desc(axes, select)
        v, n = eng.cell_dist_values(values)
        if patch:
            patch(d)
        if patch_v:
            patch_v(v)
        return l.vpic_hip_cell_distribution(e._h, None if null_d else C.byref(d), None if null_v else v, n if n_val is None else n_val, counts_ptr, sums_ptr)

    def fails(rc, word):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert word in msg, msg
        assert np.all(counts == SENTINEL_C) and np.all(sums == SENTINEL_S), "a refused call wrote output: " + msg

    fails(run(null_d=True), "descriptor")
    fails(run(counts_ptr=None, sums_ptr=None), "output")
    fails(run(values=[], counts_ptr=None), "counts")
    fails(run(patch=lambda d: setattr(d, "n_axes", 0)), "axes")
    fails(run(patch=lambda d: setattr(d, "n_axes", 3)), "axes")
    fails(run(patch=lambda d: setattr(d, "n_sel", -1)), "ranges")
    fails(run(patch=lambda d: setattr(d, "n_sel", 5)), "ranges")
    # an unknown code: the gaps of the numbering, ONE as a coordinate, and every particle code
    for code in (63, 67, 71, 102, 103, 118, 126, 127, 128, -1) + tuple(range(0, 8)) + tuple(range(16, 22)) + tuple(range(32, 36)):
        fails(run(patch=lambda d: setattr(d.axis[0], "coord", code)), "coordinate")
        fails(run(select=[("x", 0.0, 1.0)], patch=lambda d: setattr(d.sel[0], "coord", code)), "coordinate")
        if code != 127:
            for place in range(3):
                fails(run(patch_v=lambda v: v[0].factor.__setitem__(place, code)), "factor")
    fails(run(axes=[("ex", -1.0, 0.5, 0)]), "bins")
    for width in (0.0, -0.5, np.inf, np.nan):
        fails(run(axes=[("ex", -1.0, width, 4)]), "width")
    fails(run(axes=[("ex", -1.0, 0.5, 2048), ("ey", -1.0, 0.5, 2049)]), "cap")
    for n_val in (-1, 5):
        fails(run(n_val=n_val), "values")
    fails(run(null_v=True), "values array")
    fails(run(sums_ptr=None), "sums")
    for quantum in (0.0, -1e-9, np.inf, -np.inf, np.nan):
        fails(run(values=[(("ex",), 1e-9), (("ex",), quantum)]), "quantum")
    fails(l.vpic_hip_cell_distribution_stats(e._h, None), "output")
    # a hydro code on a fresh engine fails -- as an axis, a range or a factor -- and succeeds once the array exists
    fails(run(axes=[("hydro.rho", -1.0, 0.5, 4)]), "hydro")
    fails(run(select=[("hydro.txy", -1.0, 1.0)]), "hydro")
    fails(run(values=[(("ex", "one", "hydro.jx"), 1e-6)]), "hydro")
    with pytest.raises(V.VpicHipError):
        e.cell_distribution([("hydro.ke", 0.0, 1.0, 4)])
    for name in ("ux", "hydro.ex", "one"):
        with pytest.raises(KeyError):
            e.cell_distribution([(name, 0.0, 1.0, 4)])
    with pytest.raises(KeyError):
        e.cell_distribution(ok_axes, [(("q",), 1.0)])
    e.clear_hydro()
    assert run(axes=[("hydro.rho", -1.0, 0.5, 4)], values=[(("ex", "one", "hydro.jx"), 1e-6)]) == 0
    assert list(counts[:4]) == [0, 0, 64, 0] and not sums[:4].any()              # a cleared array: rho == 0 in every cell
    # what is allowed: no values (v and sums NULL), no counts beside values, every known code in every place
    counts[:] = SENTINEL_C
    sums[:] = SENTINEL_S
    assert run(values=[], sums_ptr=None, null_v=True) == 0 and int(counts[:4].sum()) == e.cell_distribution_stats()[2] and np.all(sums == SENTINEL_S)
    counts[:] = SENTINEL_C
    assert run(counts_ptr=None) == 0 and np.all(counts == SENTINEL_C) and np.all(sums[4:] == SENTINEL_S)
    for code in sorted(set(eng.CELL_COORDS.values())):
        assert run(patch=lambda d: setattr(d.axis[0], "coord", code)) == 0, code
        assert run(select=[("x", 0.0, 1.0)], patch=lambda d: setattr(d.sel[0], "coord", code)) == 0, code
        assert run(patch_v=lambda v: v[0].factor.__setitem__(1, code)) == 0, code
    r = e.cell_distribution([("z", 0.0, 1.0, 4)], [(("one",), 0.5), (("x", "y"), 0.25)])
    assert list(r.counts) == [16] * 4 and r.isums.tolist() == [[32] * 4, [256] * 4] and e.cell_distribution_stats() == (64, 64, 64, 0, 0, 0, 0, 0)
    e.close()
