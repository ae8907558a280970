"""The coordinates in the frame of the local magnetic field (u_par, u_perp, pitch, mu, b, e_par) on the GPU, as axes and
ranges of vpic_hip_species_distribution and as ranges of vpic_hip_species_select / _select_count, against the float64
restatement of test_fieldcoord_ref.py: EXACT equality of every count, of the three statistics, and of the bytes of the
selected records, indices and fields.  Every operation behind the coordinates is correctly rounded on both sides
(float +, x for the fields at the particle; double +, -, x, /, sqrt after the promotion), so there is no margin and no
excluded particle -- a difference is a bug.  No descriptor here uses LOG10_KE.

The inputs and the five array states are those of test_gpu_distribution.py (560 000 particles on 96 x 8 x 6; "tile_only"
in a fresh child process; in "tile_tail_holes" the reference is computed from the particles downloaded after the calls).
species_states.build_state steps with zero fields, so the seeded interpolator (test_select_ref.random_interpolator(4))
is set AFTER the state is built: the coordinates use the interpolator as it is loaded at the call.

Paths: par_perp through global adds (out[3] == out[2]); cos_pitch, ke_mu, b, e_par in LDS (out[3] == 0); x_pitch through the
sliding window (out[3] == 0 in voxel, tile and tile-only order)."""
import ctypes as C
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

import species_states  # noqa: E402
from species_states import N_DOOMED, N_TAIL, STATES, package  # noqa: E402
from test_distribution_ref import GRID, HAND_GRID, N  # noqa: E402
from test_fieldcoord_ref import (B_RANGE, GLOBAL, IN_LDS, UPLOADABLE, WINDOW, descriptors, distribution_ref, generated_inputs,  # noqa: E402
                                 generated_interpolator, hand_interpolator, handmade_field, keep_mask, select_ref, selections)
from test_gpu_distribution import build_state  # noqa: E402
from test_select_ref import INF, fields_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference_of_the_inputs():
    """{name: (counts, (seen, kept, counted))} of the inputs, computed once: the same in every state that holds them"""
    p, fi = generated_inputs(), generated_interpolator()
    return {name: distribution_ref(p, GRID, fi, desc, stats=True) for name, desc in descriptors().items()}


def check_state(state):
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    holes = state == "tile_tail_holes"
    descs, sels = descriptors(lds_bins=eng.DIST_LDS_BINS), selections()
    e, sp = build_state(V, V.layout, state)
    fi = generated_interpolator()
    e.set_interpolator(fi)                                    # (after the state is built: its one step ran with zero fields)
    live = e.np(sp)
    assert live == N + (N_TAIL if holes else 0)
    hist, sel = {}, {}
    for name, desc in descs.items():
        counts = e.distribution(sp, desc["axes"], desc.get("select", ()))
        stats = e.distribution_stats()
        again = e.distribution(sp, desc["axes"], desc.get("select", ()))
        assert counts.tobytes() == again.tobytes() and stats == e.distribution_stats(), name
        if "select" in desc:
            assert e.select_count(sp, select=desc["select"]) == stats[1], name        # what a histogram keeps is what a selection counts
        hist[name] = (counts, stats)
    for name, (desc, _) in sels.items():
        r = e.select(sp, fields=True, index=True, **desc)
        again = e.select(sp, fields=True, index=True, **desc)
        for a, b in zip(r[1:], again[1:]):
            assert a.tobytes() == b.tobytes(), name
        assert r.count == again.count == e.select_count(sp, **desc), name
        sel[name] = r
    back = e.get_particles(sp)                                # (after the calls: a download drops the dead slots)
    e.close()
    assert len(back) == live
    want_hist = {name: distribution_ref(back, GRID, fi, desc, stats=True) for name, desc in descs.items()} if holes else reference_of_the_inputs()
    for name in descs:
        counts, stats = hist[name]
        want_counts, want_stats = want_hist[name]
        print(f"{state} ({name}): seen {stats[0]} kept {stats[1]} counted {stats[2]} through global memory {stats[3]}; "
              f"expected {want_stats}, differing bins {int((counts != want_counts).sum()) if counts.shape == want_counts.shape else 'shape'}")
        assert counts.dtype == np.uint64 and counts.shape == want_counts.shape
        assert np.array_equal(counts, want_counts), name
        assert stats[:3] == want_stats and int(counts.sum()) == stats[2], name
        if name in IN_LDS:
            assert stats[3] == 0, name
        if name in GLOBAL:
            assert stats[3] == stats[2], name
        if name in WINDOW and state in ("voxel", "tile", "tile_only"):
            assert stats[3] == 0, name
    for name, (desc, want_count) in sels.items():
        r = sel[name]
        mask = keep_mask(back, GRID, fi, desc)
        want = back[mask]
        print(f"{state} ({name}): kept {r.count}, expected {int(mask.sum())}")
        assert r.count == len(want) == len(r.particles) == len(r.index) and r.fields.shape == (r.count, 6), name
        assert 0 < r.count < live, name
        if not holes:
            assert r.count == want_count, name
            assert r.particles.tobytes() == want.tobytes(), name
            assert np.array_equal(r.index, np.flatnonzero(mask)), name
            assert r.fields.tobytes() == fields_ref(want, fi).tobytes(), name
        else:
            assert np.all(np.diff(r.index) > 0) and r.index[0] >= 0 and r.index[-1] < live + N_DOOMED, name
            mine, theirs = np.argsort(r.particles["tag"], kind="stable"), np.argsort(want["tag"], kind="stable")
            assert len(np.unique(want["tag"])) == len(want)
            assert r.particles[mine].tobytes() == want[theirs].tobytes(), name
            assert r.fields[mine].tobytes() == fields_ref(want[theirs], fi).tobytes(), name
    # the b range, seen from the fields that came back: their double norm lies in it
    bx, by, bz = (sel["b"].fields[:, k].astype(np.float64) for k in (3, 4, 5))
    norm = np.sqrt((bx * bx + by * by) + bz * bz)
    assert np.all((norm >= B_RANGE[0]) & (norm < B_RANGE[1]))


def run_child(args, timeout):
    species_states.run_child(__file__, args, timeout)


@pytest.mark.parametrize("state", STATES)
def test_field_coordinates_equal_the_restatement_exactly(state):
    if state == "tile_only":
        run_child([state], timeout=600)                      # the knob is read when the engine is created: a fresh process
    else:
        check_state(state)


def test_handmade_and_empty_species():
    """Fewer particles than one wavefront, on every branch an upload accepts (B == 0 through a zeroed interpolator record,
    u == 0, u along B with perp2 < 0 before the clamp, u opposite to B, a value on a bin edge and on a range's hi),
    through all three paths and through the selection; and an empty species."""
    V = package()
    nx, ny, nz = HAND_GRID
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
    fi = hand_interpolator()
    e.set_interpolator(fi)
    sp = e.new_species(-1.0, 64, 8)
    assert not e.distribution(sp, [("cos_pitch", -1.0, 0.5, 4)]).any() and e.distribution_stats() == (0, 0, 0, 0)
    assert not e.distribution(sp, [("u_par", -1.0, 0.001, 2000), ("e_par", 0.0, 0.25, 20)]).any() and e.distribution_stats() == (0, 0, 0, 0)
    assert e.select_count(sp, select=[("b", 0.0, INF)]) == 0 and e.select(sp, select=[("mu", 0.0, INF)], fields=True).count == 0
    p = handmade_field()[UPLOADABLE]
    e.set_particles(sp, p)
    names = ("u_par", "u_perp", "cos_pitch", "mu", "b", "e_par")
    descs = [dict(axes=[("b", 0.0, 1.0, 5)]), dict(axes=[("u_perp", 0.0, 0.25, 4)]), dict(axes=[("cos_pitch", -1.0, 0.5, 4)]),
             dict(axes=[("u_par", -1.5, 0.75, 4), ("b", 0.5, 2.0, 3)]), dict(axes=[("mu", 0.0, 0.046875, 4)], select=[("e_par", 0.5, 0.6)]),
             dict(axes=[("e_par", 0.0, 0.1, 8)], select=[("u_par", 0.0, 0.5)]),
             dict(axes=[("x", -1.0, 0.125, 100), ("u_perp", 0.0, 0.0125, 90)]),                 # the window, 9 000 bins
             dict(axes=[("cos_pitch", -1.0, 0.1, 20), ("x", -1.0, 0.001, 5000)]),                   # bins too fine for a window: global adds
             dict(axes=[("u_par", -1.5, 0.006, 500), ("mu", 0.0, 0.01, 20)])]                   # no position axis: global adds
    descs += [dict(axes=[("ux", -2.0, 4.0, 1)], select=[(name, -INF, INF)]) for name in names]  # a NaN is in no range
    for desc in descs:
        counts = e.distribution(sp, desc["axes"], desc.get("select", ()))
        want, want_stats = distribution_ref(p, HAND_GRID, fi, desc, stats=True)
        assert np.array_equal(counts, want), (desc, counts, want)
        assert e.distribution_stats()[:3] == want_stats, desc
    for desc in [dict(select=[(name, -INF, INF)]) for name in names] + [
            dict(select=[("u_par", 0.0, 0.5)]), dict(select=[("u_par", 0.5, 1.0)]), dict(select=[("mu", 0.140625, INF)]),
            dict(select=[("e_par", 0.5, 0.7), ("ux", -1.0, 0.5)], tag_every=(2, 0)), dict(select=[("b", 0.0, 2.0)])]:
        index, want, want_fields = select_ref(p, HAND_GRID, fi, desc)
        r = e.select(sp, fields=True, index=True, **desc)
        assert r.count == len(index) == e.select_count(sp, **desc), desc
        assert r.particles.tobytes() == want.tobytes() and np.array_equal(r.index, index), desc
        assert r.fields.tobytes() == want_fields.tobytes(), desc
    assert list(e.select(sp, select=[("b", 0.0, 2.0)], index=True).index) == [0]                # the zeroed record: B == 0, kept by a B range alone
    e.close()


def test_the_species_is_left_alone():
    V = package()
    e, sp = build_state(V, V.layout, "tile_tail_holes")
    e.set_interpolator(generated_interpolator())

    def state():
        return e.species_stats(sp), e.species_order(sp), e.np(sp), e.get_tile_partition(sp).tobytes(), e.capacity(sp)

    before = state()
    assert before[0]["dead_slots"] == N_DOOMED and before[1] == "tile"
    d = descriptors()
    for name in ("x_pitch", "ke_mu"):
        assert e.distribution(sp, d[name]["axes"], d[name].get("select", ())).any()
        assert state() == before
    desc = selections()["pitch_every"][0]
    r = e.select(sp, fields=True, index=True, **desc)
    assert 0 < r.count < e.np(sp)
    assert state() == before
    assert e.select_count(sp, **desc) == r.count
    assert state() == before
    e.close()


def test_unknown_coordinates_fail():
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    e = V.Engine(V.make_grid(4, 4, 4, 4.0, 4.0, 4.0, np.float32(0.4)))
    sp = e.new_species(-1.0, 64, 8)
    counts = np.zeros(16, np.uint64)
    n = C.c_int64(-1)

    def fails(rc):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert "coordinate" in msg, msg

    for code in (8, 15, 22, -1):
        d = eng.dist_desc([("cos_pitch", -1.0, 0.5, 4)])
        d.axis[0].coord = code
        fails(l.vpic_hip_species_distribution(e._h, sp, C.byref(d), counts.ctypes.data_as(C.c_void_p)))
        d = eng.dist_desc([("cos_pitch", -1.0, 0.5, 4)], [("mu", 0.0, 1.0)])
        d.sel[0].coord = code
        fails(l.vpic_hip_species_distribution(e._h, sp, C.byref(d), counts.ctypes.data_as(C.c_void_p)))
        s = eng.select_desc([("ke", 0.0, 1.0), ("b", 0.0, 1.0)])
        s.sel[1].coord = code
        fails(l.vpic_hip_species_select_count(e._h, sp, C.byref(s), C.byref(n)))
        fails(l.vpic_hip_species_select(e._h, sp, C.byref(s), 0, None, None, None, C.byref(n)))
    for code in range(16, 22):                               # and the six are known, as axis and as range
        d = eng.dist_desc([("cos_pitch", -1.0, 0.5, 4)], [("mu", -INF, INF)])
        d.axis[0].coord, d.sel[0].coord = code, code
        assert l.vpic_hip_species_distribution(e._h, sp, C.byref(d), counts.ctypes.data_as(C.c_void_p)) == 0
        s = eng.select_desc([("b", 0.0, 1.0)])
        s.sel[0].coord = code
        assert l.vpic_hip_species_select_count(e._h, sp, C.byref(s), C.byref(n)) == 0 and n.value == 0
    e.close()


if __name__ == "__main__":
    check_state(sys.argv[1])
    print("child OK")
