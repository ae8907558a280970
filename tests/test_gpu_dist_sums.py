"""vpic_hip_species_distribution_sums on the GPU against the float64 restatement of test_dist_sums_ref.py: EXACT equality
of every int64 sum, every count, every refusal count and the statistics, in every order a species' array can be in.
The sums are integers of values that both sides round identically (test_dist_sums_ref.py says why), so there is no
tolerance and no excluded particle -- a difference is a bug.

The inputs are those of test_gpu_distribution.py (560 000 particles on 96 x 8 x 6, its five array states through
species_states.build_state; "tile_only" in a fresh child process) with the seeded two-population q of
test_dist_sums_ref.seeded_q.  build_state steps with zero fields, so the seeded interpolator is set AFTER the state is built.
The four states that hold the inputs return the same sums, those of the one reference computed once; "tile_tail_holes"
holds 5 000 appended particles more, has lost 300 and has pushed every particle once, so its reference is the restatement
of the particles downloaded after the calls.

Descriptors (test_dist_sums_ref.cases): lds4 (1-D ke, four values, LDS), global2d and par_perp (2-D above the LDS budget,
without and with field factors), mixed (a selection over ke, z and cos_pitch, three values, one of three factors),
refusing (a quantum that refuses a good share), edge_lds / edge_global (the last bin count in LDS and the first beyond)."""
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

import species_states  # noqa: E402
from species_states import N_DOOMED, N_TAIL, STATES, package  # noqa: E402
from test_dist_sums_ref import (GLOBAL, HAND_CASES, HAND_UPLOADABLE, IN_LDS, REFUSING, cases, distribution_sums_ref,  # noqa: E402
                                generated_inputs, handmade_sums, reference_of_the_inputs)
from test_distribution_ref import GRID, HAND_GRID, N, SEED  # noqa: E402
from test_fieldcoord_ref import generated_interpolator, hand_interpolator  # noqa: E402
from test_select_ref import INF  # noqa: E402

pytestmark = pytest.mark.gpu


def build_state(V, state):
    """(engine, species) with the weighted particles in the array state asked for (as test_gpu_distribution.build_state)"""
    holes = state == "tile_tail_holes"
    p = generated_inputs(spread=0.95 if holes else 1.0)
    tail = generated_inputs(SEED + 1, N_TAIL, spread=0.95, first_tag=2 * 10 ** 7) if holes else None
    return species_states.build_state(V, state, p, GRID, tail, dt=0.02 if holes else 0.4, doomed_dx=0.99)


def call(e, sp, desc, values):
    r = e.distribution_sums(sp, desc["axes"], values, desc.get("select", ()))
    return r, e.distribution_sums_stats()


def check_state(state):
    V = package()
    holes = state == "tile_tail_holes"
    e, sp = build_state(V, state)
    fi = generated_interpolator()
    e.set_interpolator(fi)                                    # (after the state is built: its one step ran with zero fields)
    live = e.np(sp)
    assert live == N + (N_TAIL if holes else 0)
    got = {}
    for name, (desc, values) in cases().items():
        r, stats = call(e, sp, desc, values)
        again, stats_again = call(e, sp, desc, values)
        for a, b in zip(r, again):
            assert a.tobytes() == b.tobytes(), name                                               # two calls: identical bytes
        assert stats == stats_again, name
        counts = e.distribution(sp, desc["axes"], desc.get("select", ()))
        assert r.counts.tobytes() == counts.tobytes() and r.counts.shape == counts.shape, name   # the histogram's own counts
        assert e.distribution_stats()[:3] == stats[:3], name
        got[name] = (r, stats)
    back = e.get_particles(sp)                                # (after the calls: a download drops the dead slots)
    e.close()
    assert len(back) == live
    want = {name: distribution_sums_ref(back, GRID, fi, desc, values) for name, (desc, values) in cases().items()} if holes \
        else reference_of_the_inputs()
    for name, (desc, values) in cases().items():
        r, stats = got[name]
        want_counts, want_isums, want_refused, want_stats = want[name]
        print(f"{state} ({name}): seen {stats[0]} kept {stats[1]} counted {stats[2]} through global memory {stats[3]} refused {stats[4:]}; "
              f"expected {want_stats} refused {list(want_refused)}, differing sums "
              f"{int((r.isums != want_isums).sum()) if r.isums.shape == want_isums.shape else 'shape'}, differing counts {int((r.counts != want_counts).sum())}")
        assert r.isums.dtype == np.int64 and r.isums.shape == want_isums.shape and r.counts.dtype == np.uint64
        assert np.array_equal(r.isums, want_isums), name
        assert np.array_equal(r.counts, want_counts), name
        assert np.array_equal(r.refused, want_refused) and r.refused.dtype == np.int64, name
        assert stats[:3] == want_stats and int(r.counts.sum()) == stats[2], name
        assert list(stats[4:4 + len(values)]) == list(want_refused) and not any(stats[4 + len(values):]), name
        assert stats[3] == (0 if name in IN_LDS else stats[2]) and (name in IN_LDS) != (name in GLOBAL), name
        assert (stats[4] > 0) == (name == REFUSING), name
        quanta = np.array([q for _, q in values]).reshape((-1,) + (1,) * (r.isums.ndim - 1))
        assert r.sums.dtype == np.float64 and np.array_equal(r.sums, r.isums * quanta), name


def run_child(args, timeout):
    species_states.run_child(__file__, args, timeout)


@pytest.mark.parametrize("state", STATES)
def test_sums_equal_the_restatement_exactly(state):
    if state == "tile_only":
        run_child([state], timeout=600)                      # the knob is read when the engine is created: a fresh process
    else:
        check_state(state)


@pytest.mark.parametrize("state", ["tile", "tile_tail_holes"])
def test_the_species_is_left_alone(state):
    """the order, the tile partition and the bookkeeping are the same before and after, through both paths, and so are the
    bytes get_particles returns -- looked at before the calls only on the species without dead slots: a download drops them
    from the array, and with appended particles and dead slots in it the array must be left as it is too"""
    V = package()
    holes = state == "tile_tail_holes"
    e, sp = build_state(V, state)
    e.set_interpolator(generated_interpolator())

    def snapshot():
        return (e.species_stats(sp), e.species_order(sp), e.np(sp), e.nm(sp), e.get_tile_partition(sp).tobytes(), e.capacity(sp),
                b"" if holes else e.get_particles(sp).tobytes())

    before = snapshot()
    assert before[0]["dead_slots"] == (N_DOOMED if holes else 0) and before[1] == "tile"
    for name in ("lds4", "par_perp", "mixed"):
        desc, values = cases()[name]
        r, stats = call(e, sp, desc, values)
        assert r.counts.any() and r.isums.any() and stats[0] == N + (N_TAIL if holes else 0)
        assert snapshot() == before, name
    e.close()


def test_small_and_empty_species():
    """Fewer particles than one wavefront, on every branch an upload accepts (ties both ways, t at 2^32 and just below, negative
    values, a NaN through a zeroed interpolator record, q of two magnitudes, one to three factors), in LDS and -- the same
    values over more bins -- through global memory; and an empty species."""
    V = package()
    nx, ny, nz = HAND_GRID
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
    fi = hand_interpolator()
    e.set_interpolator(fi)
    sp = e.new_species(-1.0, 64, 8)
    for desc, values in HAND_CASES:
        r, stats = call(e, sp, desc, values)
        assert not r.counts.any() and not r.isums.any() and not r.refused.any() and stats == (0,) * 8
    p = handmade_sums()[HAND_UPLOADABLE]
    e.set_particles(sp, p)
    wide = [(dict(axes=[("ux", -0.5, 0.001, 3000), ("uy", -1.0, 2.0, 1)]), HAND_CASES[0][1]),                 # 3000 bins x 9 words: global adds
            (dict(axes=[("ux", -0.5, 0.5, 3), ("b", 0.0, 0.002, 2600)], select=[("ke", 0.005, INF)]), HAND_CASES[1][1])]
    for desc, values in HAND_CASES + wide:
        r, stats = call(e, sp, desc, values)
        want_counts, want_isums, want_refused, want_stats = distribution_sums_ref(p, HAND_GRID, fi, desc, values)
        assert np.array_equal(r.counts, want_counts), (desc, r.counts, want_counts)
        assert np.array_equal(r.isums, want_isums), (desc, r.isums[r.isums != want_isums], want_isums[r.isums != want_isums])
        assert np.array_equal(r.refused, want_refused), (desc, r.refused, want_refused)
        assert stats[:3] == want_stats and stats[3] == (stats[2] if (desc, values) in wide else 0), desc
    # the first case in words: ties to even both ways, 2^32 refused, the float below it taken
    r, stats = call(e, sp, *HAND_CASES[0])
    assert int(r.isums[0, 0]) == 2 - 2 + (2 ** 32 - 256) + 3 and list(r.refused) == [1, 2, 2, 3] and stats[4:] == (1, 2, 2, 3)
    e.close()


def test_argument_errors():
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    e = V.Engine(V.make_grid(4, 4, 4, 4.0, 4.0, 4.0, np.float32(0.4)))
    sp = e.new_species(-1.0, 64, 8)
    counts, sums = np.zeros(1 << 16, np.uint64), np.zeros(4 << 16, np.int64)
    cp, sp_ = counts.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)
    ok_axes, ok_values = [("ux", -1.0, 0.5, 4)], [(("q", "ke"), 1e-9)]

    def run(axes=ok_axes, select=(), values=ok_values, species=sp, counts_ptr=cp, sums_ptr=sp_, patch=None, patch_v=None, n_val=None,
            null_d=False, null_v=False):
        d, v = eng.dist_desc(axes, select), eng.dist_values(values)
        if patch:
            patch(d)
        if patch_v:
            patch_v(v)
        return l.vpic_hip_species_distribution_sums(e._h, species, None if null_d else C.byref(d), None if null_v else v,
                                                    len(v) if n_val is None else n_val, counts_ptr, sums_ptr)

    def fails(rc, word):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert word in msg, msg

    assert run() == 0
    assert run(counts_ptr=None) == 0                                                      # counts may be NULL
    # everything vpic_hip_species_distribution fails on
    fails(run(species=sp + 1), "species")
    fails(run(species=-1), "species")
    fails(run(null_d=True), "descriptor")
    fails(run(patch=lambda d: setattr(d, "n_axes", 0)), "axes")
    fails(run(patch=lambda d: setattr(d, "n_axes", 3)), "axes")
    fails(run(patch=lambda d: setattr(d, "n_sel", -1)), "ranges")
    fails(run(patch=lambda d: setattr(d, "n_sel", 5)), "ranges")
    fails(run(patch=lambda d: setattr(d.axis[0], "coord", 8)), "coordinate")
    fails(run(patch=lambda d: setattr(d.axis[0], "coord", 32)), "coordinate")             # a factor code is no coordinate
    fails(run(select=[("ke", 0.0, 1.0)], patch=lambda d: setattr(d.sel[0], "coord", 33)), "coordinate")
    fails(run(axes=[("ux", -1.0, 0.5, 0)]), "bins")
    for width in (0.0, -0.5, np.inf, np.nan):
        fails(run(axes=[("ux", -1.0, width, 4)]), "width")
    fails(run(axes=[("ux", -1.0, 0.5, 2048), ("uy", -1.0, 0.5, 2049)]), "cap")
    # n_val outside 1..4
    for n_val in (0, -1, 5):
        fails(run(n_val=n_val), "values")
    # a NULL v or sums
    fails(run(null_v=True), "values array")
    fails(run(sums_ptr=None), "sums")
    # an unknown factor, LOG10_KE as a factor
    for code in (7, 8, 15, 22, 31, 36, -1):
        for place in range(3):
            fails(run(patch_v=lambda v: v[0].factor.__setitem__(place, code)), "factor")
    fails(run(values=[(("q",), 1e-9), (("ke", "one", "ux"), 1e-9)], patch_v=lambda v: v[1].factor.__setitem__(2, 7)), "factor")
    with pytest.raises(V.VpicHipError):
        e.distribution_sums(sp, ok_axes, [(("q", "log10_ke"), 1e-9)])
    # a quantum that is not positive and finite
    for quantum in (0.0, -1e-9, np.inf, -np.inf, np.nan):
        fails(run(values=[(("q",), 1e-9), (("q",), quantum)]), "quantum")
    fails(l.vpic_hip_species_distribution_sums_stats(e._h, None), "output")
    with pytest.raises(KeyError):
        e.distribution_sums(sp, ok_axes, [(("weight",), 1e-9)])
    with pytest.raises(KeyError):
        e.distribution_sums(sp, [("pitch", -1.0, 0.5, 4)], ok_values)
    # every factor that is one is accepted, and the engine is still usable
    for code in list(range(0, 7)) + list(range(16, 22)) + list(range(32, 36)):
        assert run(patch_v=lambda v: v[0].factor.__setitem__(1, code)) == 0, code
    one = np.zeros(1, V.layout.particle_t)
    one["i"], one["ux"], one["q"] = 1 + 6 * (1 + 6 * 1), 0.25, -0.5
    e.set_particles(sp, one)
    r = e.distribution_sums(sp, ok_axes, [(("q",), 0.125), (("q", "ux"), 2.0 ** -10)])
    assert list(r.counts) == [0, 0, 1, 0] and r.isums.tolist() == [[0, 0, -4, 0], [0, 0, -128, 0]] and list(r.refused) == [0, 0]
    assert r.sums.tolist() == [[0, 0, -0.5, 0], [0, 0, -0.125, 0]] and e.distribution_sums_stats() == (1, 1, 1, 0, 0, 0, 0, 0)
    e.close()


if __name__ == "__main__":
    check_state(sys.argv[1])
    print("child OK")
