"""vpic_hip_species_select on the GPU against the numpy restatement of test_select_ref.py: EXACT equality of the
records, the indices and the fields at the particles (integers, copied floats, and float arithmetic rounded once per
operation on both sides: no tolerance to choose), in every order a species' array can be in, for the seven selections
of test_select_ref.selections -- the energetic tail, a box, every 100th tag, a tag range, all three kinds at once,
everything, nothing.

The inputs and the array states are those of test_gpu_distribution.py (build_state: 560 000 particles on a 96 x 8 x 6
grid, tags 1..N; "unsorted", "voxel", "tile", "tile_only" in a fresh child process, "tile_tail_holes" with 5 000
appended particles and 300 dead slots).  In the four states without holes the species holds the inputs, so the counts
are the ones test_select_ref.py asserts on the CPU, and a download leaves the order alone: the selection must equal
the downloaded array under the restatement's mask, byte for byte.  A download of the last state drops the dead slots,
so there the two sides are compared after sorting by tag (unique), and the indices are checked for what they promise.

The interpolator is set to seeded non-zero values in every voxel and component before the calls."""
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
from test_distribution_ref import GRID, N, SEED, VTH, coordinate, dist_inputs  # noqa: E402
from test_gpu_distribution import build_state  # noqa: E402
from test_select_ref import INF, fields_ref, keep_mask, random_interpolator, select_ref, selections  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = 2048                                                   # particles per chunk (include/vpic_hip.h: select_stats)


@functools.lru_cache(maxsize=None)
def ke_max_of_the_inputs():
    return float(coordinate(dist_inputs(SEED, N, VTH, GRID), GRID, "ke").max())


def check_state(state):
    V = package()
    holes = state == "tile_tail_holes"
    e, sp = build_state(V, V.layout, state)
    fi = random_interpolator(4, GRID)
    e.set_interpolator(fi)
    live = e.np(sp)
    extent = live + e.species_stats(sp)["dead_slots"]
    assert live == N + (N_TAIL if holes else 0) and extent == live + (N_DOOMED if holes else 0)
    sels = selections(ke_max_of_the_inputs())
    got = {}
    for name, (desc, _) in sels.items():
        r = e.select(sp, fields=True, index=True, **desc)
        stats = e.select_stats()
        again = e.select(sp, fields=True, index=True, **desc)
        for a, b in zip(r[1:], again[1:]):
            assert a.tobytes() == b.tobytes(), name                                   # two calls: identical bytes
        assert r.count == again.count == e.select_count(sp, **desc), name
        got[name] = (r, stats)
    back = e.get_particles(sp)                                 # (after the calls: a download drops the dead slots)
    e.close()
    assert len(back) == live
    for name, (desc, want_count) in sels.items():
        r, stats = got[name]
        mask = keep_mask(back, GRID, desc)
        want = back[mask]
        print(f"{state} ({name}): kept {r.count}, expected {int(mask.sum())}; stats {stats}")
        assert r.particles.dtype == V.layout.particle_t and r.fields.dtype == np.float32 and r.index.dtype == np.int64
        assert r.count == len(want) == len(r.particles) == len(r.index) and r.fields.shape == (r.count, 6), name
        assert stats == (live, r.count, r.count, -(-extent // CHUNK)), name
        if not holes:
            assert r.count == want_count, name
            assert r.particles.tobytes() == want.tobytes(), name
            assert np.array_equal(r.index, np.flatnonzero(mask)), name
            assert r.fields.tobytes() == fields_ref(want, fi).tobytes(), name
        else:
            assert np.all(np.diff(r.index) > 0) and (r.count == 0 or (r.index[0] >= 0 and r.index[-1] < extent)), name
            assert not np.any((r.particles["tag"] >= 10 ** 7) & (r.particles["tag"] < 10 ** 7 + N_DOOMED)), name
            mine, theirs = np.argsort(r.particles["tag"], kind="stable"), np.argsort(want["tag"], kind="stable")
            assert len(np.unique(want["tag"])) == len(want)
            assert r.particles[mine].tobytes() == want[theirs].tobytes(), name
            assert r.fields[mine].tobytes() == fields_ref(want[theirs], fi).tobytes(), name
    if holes:
        assert 0 < got["tail"][0].count < live and got["all"][0].count == live and got["none"][0].count == 0


def run_child(args, timeout):
    species_states.run_child(__file__, args, timeout)


@pytest.mark.parametrize("state", STATES)
def test_selection_equals_the_restatement_exactly(state):
    if state == "tile_only":
        run_child([state], timeout=600)                      # the knob is read when the engine is created: a fresh process
    else:
        check_state(state)


def test_cap():
    """count is the number kept whatever the cap; exactly the first cap records are written; the record behind them
    in every host array keeps its pattern"""
    V = package()
    l = V.lib()
    eng = importlib.import_module("old-vpic_amd.engine")
    e, sp = build_state(V, V.layout, "tile")
    fi = random_interpolator(4, GRID)
    e.set_interpolator(fi)
    desc, want_count = selections(ke_max_of_the_inputs())["tail"]
    full = e.select(sp, fields=True, index=True, **desc)
    assert full.count == want_count == 23247
    d = eng.select_desc(**desc)
    for cap in (want_count, want_count - 1, 1, 0):
        p = np.frombuffer(bytearray(b"\xa5" * (48 * (cap + 1))), V.layout.particle_t)
        f = np.frombuffer(bytearray(b"\xa5" * (24 * (cap + 1))), np.float32).reshape(cap + 1, 6)
        i = np.frombuffer(bytearray(b"\xa5" * (8 * (cap + 1))), np.int64)
        n = C.c_int64(-1)
        rc = l.vpic_hip_species_select(e._h, sp, C.byref(d), cap, p.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p),
                                       i.ctypes.data_as(C.c_void_p), C.byref(n))
        assert rc == 0, l.vpic_hip_last_error().decode()
        assert n.value == want_count, cap
        assert e.select_stats()[1:3] == (want_count, cap), cap
        assert p[:cap].tobytes() == full.particles[:cap].tobytes(), cap
        assert f[:cap].tobytes() == full.fields[:cap].tobytes(), cap
        assert i[:cap].tobytes() == full.index[:cap].tobytes(), cap
        for guard in (p[cap:], f[cap:], i[cap:]):
            assert set(guard.tobytes()) == {0xa5}, cap
        r = e.select(sp, cap=cap, fields=True, index=True, **desc)                    # the same through the method
        assert r.count == want_count and len(r.particles) == len(r.fields) == len(r.index) == cap
        assert r.particles.tobytes() == full.particles[:cap].tobytes()
    # parts that are not asked for are not written, and do not change the rest
    only_index = e.select(sp, index=True, **desc)
    assert only_index.fields is None and only_index.index.tobytes() == full.index.tobytes()
    n = C.c_int64(-1)
    assert l.vpic_hip_species_select(e._h, sp, C.byref(d), want_count, None, None, None, C.byref(n)) == 0
    assert n.value == want_count and e.select_stats()[1:3] == (want_count, 0)
    e.close()


SMALL_GRID = (4, 4, 4)


@pytest.mark.parametrize("tagged", [False, True])
def test_small_and_empty_species(tagged):
    """0, 1, 63, 64, 65, 257 and one chunk - 1, one chunk, one chunk + 1 particles, everything kept and nothing kept;
    tagged: tags 1..n; not tagged: no tag was ever uploaded, every tag reads 0"""
    V = package()
    nx, ny, nz = SMALL_GRID
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
    fi = random_interpolator(6, SMALL_GRID)
    e.set_interpolator(fi)
    for n in (0, 1, 63, 64, 65, 257, CHUNK - 1, CHUNK, CHUNK + 1):
        sp = e.new_species(-1.0, max(n, 1), 8)
        p = dist_inputs(SEED + n, n, VTH, SMALL_GRID) if n else np.zeros(0, V.layout.particle_t)
        if tagged:
            p["tag"] = np.arange(n) + 1
            p["tag2"] = -np.arange(n)
        if n:
            e.set_particles(sp, p)
        everything = [dict(), dict(select=[("ke", 0.0, INF), ("x", 0.0, float(nx))])]
        nothing = [dict(select=[("ke", 1e6, INF)]), dict(select=[("x", -3.0, 0.0)])]
        if tagged:
            everything += [dict(tag_range=(1, n + 1)), dict(tag_every=(1, 0))]
            nothing += [dict(tag_range=(n + 1, n + 2)), dict(tag_range=(-5, 1))]
        else:
            everything += [dict(tag_range=(0, 1)), dict(tag_every=(3, 0))]
            nothing += [dict(tag_range=(1, 2)), dict(tag_every=(3, 1))]
        for desc in everything + nothing + [dict(tag_every=(2, 1)), dict(select=[("ux", 0.0, INF)])]:
            index, want, want_fields = select_ref(p, SMALL_GRID, fi, desc)
            if any(desc is d for d in everything):
                assert len(index) == n
            if any(desc is d for d in nothing):
                assert len(index) == 0
            r = e.select(sp, fields=True, index=True, **desc)
            assert r.count == len(index) == e.select_count(sp, **desc), (n, desc)
            assert r.particles.tobytes() == want.tobytes() and np.array_equal(r.index, index), (n, desc)
            assert r.fields.tobytes() == want_fields.tobytes(), (n, desc)
            assert e.select_stats() == (n, len(index), 0, -(-n // CHUNK)), (n, desc)  # (select_count came last: nothing written)
        assert e.species_stats(sp)["dead_slots"] == 0 and e.np(sp) == n
    e.close()


def test_the_species_is_left_alone():
    V = package()
    e, sp = build_state(V, V.layout, "tile_tail_holes")

    def state():
        return e.species_stats(sp), e.species_order(sp), e.np(sp), e.get_tile_partition(sp).tobytes()

    before = state()
    assert before[0]["dead_slots"] == N_DOOMED and before[1] == "tile"
    desc = selections(ke_max_of_the_inputs())["mixed"][0]
    r = e.select(sp, fields=True, index=True, **desc)
    assert 0 < r.count < e.np(sp)
    assert state() == before
    assert e.select_count(sp, **desc) == r.count
    assert state() == before
    e.clear_accumulators()
    e.advance_p(sp)                                            # the push that follows finds the species as it left it
    assert e.np(sp) == before[2] and e.species_order(sp) == "tile"
    e.close()


def test_argument_errors():
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    e = V.Engine(V.make_grid(4, 4, 4, 4.0, 4.0, 4.0, np.float32(0.4)))
    sp = e.new_species(-1.0, 64, 8)
    p = np.zeros(4, V.layout.particle_t)
    n = C.c_int64(-1)
    pp, np_ = p.ctypes.data_as(C.c_void_p), C.byref(n)

    def call(species=sp, cap=4, patch=None, desc=True, count=np_, **kw):
        d = eng.select_desc(**kw)
        if patch:
            patch(d)
        return l.vpic_hip_species_select(e._h, species, C.byref(d) if desc else None, cap, pp, None, None, count)

    def count(species=sp, patch=None, desc=True, count=np_, **kw):
        d = eng.select_desc(**kw)
        if patch:
            patch(d)
        return l.vpic_hip_species_select_count(e._h, species, C.byref(d) if desc else None, count)

    def fails(rc, word):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert word in msg, msg

    assert call() == 0 and n.value == 0 and count() == 0
    for fn in (call, count):
        fails(fn(species=sp + 1), "species")
        fails(fn(species=-1), "species")
        fails(fn(desc=False), "descriptor")
        fails(fn(count=None), "count")
        fails(fn(patch=lambda d: setattr(d, "n_sel", -1)), "ranges")
        fails(fn(patch=lambda d: setattr(d, "n_sel", 5)), "ranges")
        fails(fn(select=[("ke", 0.0, 1.0)], patch=lambda d: setattr(d.sel[0], "coord", 8)), "coordinate")
        fails(fn(select=[("ke", 0.0, 1.0), ("x", 0.0, 1.0)], patch=lambda d: setattr(d.sel[1], "coord", -1)), "coordinate")
        fails(fn(patch=lambda d: setattr(d, "flags", 4)), "flag")
        fails(fn(tag_range=(0, 1), patch=lambda d: setattr(d, "flags", 1 | 8)), "flag")
        fails(fn(tag_every=(0, 0)), "tag_every")
        fails(fn(tag_every=(-3, 0)), "tag_every")
        fails(fn(tag_every=(5, 5)), "tag_phase")
        fails(fn(tag_every=(5, -1)), "tag_phase")
    fails(call(cap=-1), "cap")
    fails(l.vpic_hip_species_select_stats(e._h, None), "output")
    with pytest.raises(V.VpicHipError):
        e.select(sp, tag_every=(0, 0))
    with pytest.raises(V.VpicHipError):
        e.select_count(sp, tag_every=(4, 4))
    with pytest.raises(V.VpicHipError):
        e.select(sp, cap=-2)
    with pytest.raises(KeyError):
        e.select(sp, select=[("pitch", 0.0, 1.0)])
    # a tag_every that is not enabled is not looked at, and the engine still answers
    assert call(patch=lambda d: setattr(d, "tag_every", -1)) == 0
    one = np.zeros(1, V.layout.particle_t)
    one["i"], one["ux"], one["q"], one["tag"] = 1 + 6 * (1 + 6 * 1), 0.25, -0.01, 12
    e.set_particles(sp, one)
    r = e.select(sp, select=[("ux", 0.0, 1.0)], tag_every=(4, 0), index=True)
    assert r.count == 1 and r.particles.tobytes() == one.tobytes() and list(r.index) == [0] and r.fields is None
    assert e.select_stats() == (1, 1, 1, 1)
    e.close()


if __name__ == "__main__":
    check_state(sys.argv[1])
    print("child OK")
