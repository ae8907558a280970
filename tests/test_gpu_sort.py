"""Every kernel path of the sorts (particles.hip: k_sort_p, k_tail_sort; push.hip: the launch that sorts as it pushes) held
to tests/sort_ref.py: order, content bit for bit, partition[] / tpart[] entry by entry and the fullest-tile word -- all with
`==`, no tolerance anywhere but the accumulator sums of P8 (ACC_TOL of test_gpu_tiles.py).  GPU box only.

Paths (knobs are read when the engine is created: set before V.Engine):
  P1  voxel order, default plan                       wg_count_kernel<false> + wg_scatter_kernel<false>
  P2  voxel order, VPIC_HIP_OLD_SORT=1                sort_count_kernel<false> + sort_scatter_kernel<false>
  P3  voxel order after three pushes of a hot species sort_count_kernel<false> + wg_scatter_kernel<false> (policy.h: plan_sort,
      (> 15 % of the particles change cell per step)  count_by_wave)
  P4  tile order by cell (VPIC_HIP_WINDOW=tile)       wg_count_kernel<true> + wg_scatter_kernel<true>
  P5  tile order by cell, VPIC_HIP_OLD_SORT=1         sort_count_kernel<true> + sort_scatter_kernel<true> (what k_tail_sort runs)
  P6  by tile only (VPIC_HIP_TILE_COARSE=1)           coarse_count_kernel + wg_scatter_kernel<true, true>
  P7  tile order by cell, counted by the push before  the scan of Species::hist + wg_scatter_kernel<true>
  P8  the sort inside the push                        advance_p_kernel<.., SORT> (vpic_hip_sort_advance_p)
  P9  the tail regrouping, P9h with dead slots in it  k_tail_sort, tail_copy_back_kernel's n_live branch
Grids, particle counts and arrangements: sort_ref.GRIDS, NP_EDGES, ARRANGEMENTS, each with its reason;
tests/test_sort_ref.py asserts on the CPU that the seeded inputs reach the table overflows, the scan's carry loop and the
group_info fallback they are there for.  test_the_matrix_covers_every_path checks the parameter lists themselves.

`ghosts` (2 % of the particles in ghost voxels, which vpic_hip_species_set_particles refuses) goes in through the
library's test hook vpic_hip_debug_set_particles_any_voxel; such a species is sorted and read back, never pushed.
Dead slots: species_states.build_state("tile_tail_holes").  A download compacts a species with dead slots (a sort in the
order it is in), so the live reference there is e.select(sp, index=True), which reads the array as it is."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sort_ref as S
from conftest import bits_equal
from species_states import N_DOOMED, N_TAIL, build_state
from test_gpu_tiles import ACC_TOL, acc_close, hot_particles, random_interpolator

pytestmark = pytest.mark.gpu

KNOBS = ("VPIC_HIP_WINDOW", "VPIC_HIP_TILE_COARSE", "VPIC_HIP_OLD_SORT", "VPIC_HIP_SORT_IN_PUSH", "VPIC_HIP_TAIL_SORT_MIN",
         "VPIC_HIP_NO_TAIL_SORT", "VPIC_HIP_STAGE", "VPIC_HIP_FOLLOW", "VPIC_HIP_ITERS")
TILE_ENV = {"VPIC_HIP_WINDOW": "tile", "VPIC_HIP_TILE_COARSE": "0"}
PATHS = {                                                   # path: (order of the array afterwards, knobs)
    "P1": ("voxel", {}),
    "P2": ("voxel", {"VPIC_HIP_OLD_SORT": "1"}),
    "P3": ("voxel", {}),
    "P4": ("tile", TILE_ENV),
    "P5": ("tile", dict(TILE_ENV, VPIC_HIP_OLD_SORT="1")),
    "P6": ("tile_only", {"VPIC_HIP_WINDOW": "tile", "VPIC_HIP_TILE_COARSE": "1"}),
}
PURE = ("P1", "P2", "P4", "P5", "P6")
OTHER_GRIDS = tuple(g for g in S.GRIDS if g not in S.MAIN_GRIDS)
# (path, grid, arrangement, particles): the np edges on (7,9,6); every arrangement on the two main grids; random and nearly
# on the other grids
PURE_CASES = [(path, (7, 9, 6), "random", n) for path in ("P1", "P4", "P6") for n in S.NP_EDGES] + \
             [(path, grid, name, S.default_n(grid)) for path in PURE for grid in S.MAIN_GRIDS for name in S.ARRANGEMENTS] + \
             [(path, grid, name, S.default_n(grid)) for path in PURE for grid in OTHER_GRIDS for name in ("random", "nearly")]
P3_CASES = [(grid, name) for grid in S.MAIN_GRIDS for name in S.ARRANGEMENTS if name != "ghosts"]      # (ghosts are never pushed)
HOLES_CASES = [(path, grid) for path in ("P1", "P4", "P6") for grid in S.MAIN_GRIDS]
PUSH_CASES = [((7, 9, 6), "periodic"), ((5, 4, 4), "periodic"), ((16, 8, 12), "periodic"), ((7, 9, 6), "reflecting_z")]
TAIL_CASES = [((7, 9, 6), "random", 1), ((7, 9, 6), "random", 300), ((7, 9, 6), "round_robin_20", 2049), ((7, 9, 6), "random", 5000),
              ((16, 8, 12), "random", 5000)]
TAGS = [True, False]
TAG_IDS = ["tagged", "tagless"]


def case_id(c):
    return " ".join(S.grid_id(x) if isinstance(x, tuple) else str(x) for x in c)


@pytest.fixture(scope="module")
def V():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def engine_for(V, grid, dt=0.3, **kw):
    nx, ny, nz = grid
    return V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt), **kw))


def upload(V, e, sp, p, any_voxel=False):
    if not any_voxel:
        e.set_particles(sp, p)
        return
    f = V.lib().vpic_hip_debug_set_particles_any_voxel          # (a test hook that no header declares: the arguments say their types)
    p = np.ascontiguousarray(p, V.layout.particle_t)
    if f(e._h, C.c_int(sp), p.ctypes.data_as(C.c_void_p), C.c_int64(len(p))):
        raise V.VpicHipError(V.lib().vpic_hip_last_error().decode())


def after_a_sort(V, e, sp, live, grid, order):
    """everything a sort of `live` into `order` must have left behind; returns partition[] / tpart[]"""
    got = e.get_particles(sp)
    stats = e.species_stats(sp)
    assert e.np(sp) == len(live) == len(got)
    assert e.capacity(sp)[0] == len(live)                   # the extent: no slot beyond the live particles
    assert stats["dead_slots"] == 0
    assert stats["by_tile_only"] == (1 if order == "tile_only" else 0)
    if order == "voxel":
        starts = e.get_partition(sp)
        S.check(got, live, grid, "voxel", partition=starts)
        assert e.species_order(sp) == "voxel"
        assert e.measure_disorder(sp) == 0.0
    else:
        starts = e.get_tile_partition(sp)
        S.check(got, live, grid, order, tpart=starts)
        assert e.species_order(sp) == "tile"
        with pytest.raises(V.VpicHipError):
            e.get_partition(sp)                             # partition[] is the reference's order's
        e.sync()
        assert e.species_stats(sp)["fullest_tile"] == S.fullest_tile(live["i"], grid)
    return starts


def sort_twice(V, e, sp, live, grid, order):
    """sort_p, everything checked; sort_p again: checked again, with identical partition[] / tpart[]"""
    e.sort_p(sp)
    first = after_a_sort(V, e, sp, live, grid, order)
    e.sort_p(sp)
    again = after_a_sort(V, e, sp, live, grid, order)
    assert np.array_equal(first, again)


@pytest.mark.parametrize("tagged", TAGS, ids=TAG_IDS)
@pytest.mark.parametrize("case", PURE_CASES, ids=case_id)
def test_sort_p(V, monkeypatch, case, tagged):
    """set particles, sort_p, download, check; and a second sort_p"""
    path, grid, name, n = case
    order, env = PATHS[path]
    set_knobs(monkeypatch, env)
    p = S.case_particles(grid, name, n, order, tagged)
    e = engine_for(V, grid)
    sp = e.new_species(-1.0, n + 8, 64)
    upload(V, e, sp, p, any_voxel=name == "ghosts")
    if n == 0:
        e.sort_p(sp)
        assert e.np(sp) == 0
    else:
        sort_twice(V, e, sp, p, grid, order)
    e.close()


def pushable(grid, name, n, tagged, vth, spread=1.0, seed=0):
    """particles in the case's voxels that a push can take: offsets inside the cell, momenta of thermal spread vth"""
    rng = np.random.default_rng([seed, n, int(tagged)] + list(grid))
    p = np.zeros(n, S.particle_dtype())
    p["i"] = S.case_voxels(grid, name, n, "voxel")
    for c in ("dx", "dy", "dz"):
        p[c] = (rng.uniform(-1, 1, n) * spread).astype(np.float32)
    for c in ("ux", "uy", "uz"):
        p[c] = (rng.standard_normal(n) * vth).astype(np.float32)
    p["q"] = (-0.01 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    if tagged:
        p["tag"] = rng.permutation(n) + 1
    return p


@pytest.mark.parametrize("tagged", TAGS, ids=TAG_IDS)
@pytest.mark.parametrize("case", P3_CASES, ids=case_id)
def test_sort_p_of_a_hot_species_in_voxel_order(V, monkeypatch, case, tagged):
    """P3: zero fields, |u| of order 1, half a cell per step at most: well over 15 % of the particles change cell per step,
    which makes plan_sort count a wavefront at a time and scatter by workgroup.  The array starts in the arrangement's order
    and is not sorted before the pushes; the reference is the download taken just before the sort."""
    grid, name = case
    set_knobs(monkeypatch, PATHS["P3"][1])
    n = S.default_n(grid)
    p = pushable(grid, name, n, tagged, vth=1.0)
    e = engine_for(V, grid, dt=0.5)
    e.set_vacuum()
    e.load_interpolator()
    sp = e.new_species(-1.0, n + 8, 4096)
    e.set_particles(sp, p)
    for push in range(3):
        e.clear_accumulators()
        assert e.advance_p(sp) == 0
        e.sync()
        assert e.species_stats(sp)["crossed"] / n > 0.15, push      # (the sort reads the fraction of the push before the last: both hold)
    before = e.get_particles(sp)
    sort_twice(V, e, sp, before, grid, "voxel")
    e.close()


@pytest.mark.parametrize("case", HOLES_CASES, ids=case_id)
def test_a_sort_drops_the_dead_slots(V, monkeypatch, case):
    """Dead slots (i = -1: N_DOOMED particles that one step of the resident exchange removed at an absorbing wall) inside a
    sort by P1, P4 and P6: the live particles as e.select reads them from the array before the sort, sorted; the extent is
    the live count afterwards and no dead slot is left.  (Tagged: build_state tags the doomed particles.)"""
    path, grid = case
    order, env = PATHS[path]
    set_knobs(monkeypatch, env if path == "P6" else {})
    n = 6000
    p = pushable(grid, "random", n, True, vth=0.05, spread=0.9)
    tail = pushable(grid, "nearly", N_TAIL, True, vth=0.05, spread=0.9, seed=1)
    tail["tag"] += 10 ** 6
    e, sp = build_state(V, "tile_tail_holes", p, grid, tail, dt=0.02, doomed_dx=0.99, coarse=path == "P6")
    assert e.species_stats(sp)["dead_slots"] == N_DOOMED and e.capacity(sp)[0] == n + N_TAIL + N_DOOMED
    r = e.select(sp, index=True)
    live = r.particles
    assert r.count == len(live) == n + N_TAIL == e.np(sp) and np.all(live["i"] >= 0)
    assert r.index.max() >= n + N_TAIL - 1 and len(np.unique(live["tag"])) == len(live)
    assert e.species_stats(sp)["dead_slots"] == N_DOOMED                      # (reading them did not compact the array)
    if path == "P1":
        e.set_sort_order("reference")
    sort_twice(V, e, sp, live, grid, order)
    e.close()


def push_setup(V, orc, L, grid, walls, seed):
    nx, ny, nz = grid
    kw = dict(pbc=[0, 0, L.REFLECT_PARTICLES, 0, 0, L.REFLECT_PARTICLES]) if walls == "reflecting_z" else {}
    rng = np.random.default_rng(seed)
    g = V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.5), **kw)
    og = orc.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.5), **kw)
    fi = random_interpolator(orc, L, og, rng)
    p = hot_particles(L, rng, nx, ny, nz, 40 if nx * ny * nz < 100 else 24, vth=0.5)
    p["tag"] = 0                                            # (tags ride outside the push: a tagged species sorts the ordinary way)
    e = V.Engine(g)
    e.set_sort_order("engine")
    e.set_interpolator(fi)
    sp = e.new_species(-1.0, 2 * len(p), 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == "tile" and e.species_stats(sp)["by_tile_only"] == 0
    return e, sp, og, fi, p


def push(e, sp, hint=False):
    if hint:
        e._l.vpic_hip_species_sort_hint(e._h, sp)
    e.clear_accumulators()
    assert e.advance_p(sp) == 0


@pytest.mark.parametrize("case", PUSH_CASES, ids=case_id)
def test_a_sort_counted_by_the_push_before(V, orc, L, monkeypatch, case):
    """P7: vpic_hip_species_sort_hint, advance_p, sort_p -- the sort starts at the scan of the counts that push took.  Hot
    tag-less species, a random interpolator; checked against the download taken between the push and the sort."""
    grid, walls = case
    set_knobs(monkeypatch, {})
    e, sp, og, fi, p = push_setup(V, orc, L, grid, walls, 43)
    push(e, sp)
    push(e, sp)
    push(e, sp, hint=True)
    before = e.get_particles(sp)
    assert len(before) == len(p)
    sort_twice(V, e, sp, before, grid, "tile")
    e.close()


@pytest.mark.parametrize("case", PUSH_CASES, ids=case_id)
def test_the_sort_inside_the_push(V, orc, L, monkeypatch, case):
    """P8 (VPIC_HIP_SORT_IN_PUSH=1): sort, two plain pushes, a hinted push, sort_advance_p -- one launch over np particles
    that sorted as it pushed, or the case has not tested what it claims.  The array is then ordered by the tile-and-cell key
    of where every particle was BEFORE that push: for EVERY occupied key, the key's range holds exactly the oracle's push
    (advance_p in place on the stably key-sorted download) of the particles that were in that key, as a multiset of
    records; tpart[] is the starts of the keys before the push; the accumulator is the oracle's within ACC_TOL.  Then a
    hinted push and a second sort_advance_p, checked the same way."""
    grid, walls = case
    set_knobs(monkeypatch, {"VPIC_HIP_SORT_IN_PUSH": "1"})
    e, sp, og, fi, p = push_setup(V, orc, L, grid, walls, 47)
    push(e, sp)
    push(e, sp)
    push(e, sp, hint=True)
    e.profile_enable(True)
    pm = np.zeros(4096, L.particle_mover_t)
    for round_ in (1, 2):
        before = e.get_particles(sp)
        assert len(before) == len(p)
        e.clear_accumulators()
        assert e.sort_advance_p(sp) == 0
        ms, launches, parts = e.profile_read_sorting()
        assert launches == round_ and parts == round_ * len(p)
        got = e.get_particles(sp)
        kb = S.keys(before["i"], grid, "tile")
        by_key = np.argsort(kb, kind="stable")
        ref, k_sorted = before[by_key].copy(), kb[by_key]
        ref_a = np.zeros(og.nv, L.accumulator_t)
        assert orc.advance_p(ref, len(ref), -1.0, pm, ref_a, fi, og) == 0   # in place: range k of ref = the particles that were in key k
        S.same_per_key(got, k_sorted, ref, k_sorted, what="the sort inside the push")
        assert np.array_equal(e.get_tile_partition(sp), S.starts(before["i"], grid, "tile"))
        acc_close(e.get_accumulator(), ref_a, ACC_TOL)
        assert e.species_order(sp) == "tile" and e.np(sp) == len(p) and e.species_stats(sp)["dead_slots"] == 0
        if round_ == 1:
            push(e, sp, hint=True)
    e.close()


def still_particles(grid, name, n, tagged, seed):
    """particles a push with zero fields leaves as they are, bit for bit: u = +0"""
    p = pushable(grid, name, n, tagged, vth=0.0, seed=seed)
    for c in ("ux", "uy", "uz"):
        p[c] = 0.0
    return p


@pytest.mark.parametrize("tagged", TAGS, ids=TAG_IDS)
@pytest.mark.parametrize("case", TAIL_CASES, ids=case_id)
def test_the_tail_is_regrouped_by_tile(V, monkeypatch, case, tagged):
    """P9 (VPIC_HIP_TAIL_SORT_MIN=1): tile-sort, append a tail, push with zero fields and u = 0 -- the identity on every
    word.  The sorted part is the input bit for bit in its places, the tail is the appended particles grouped by tile."""
    grid, name, n_tail = case
    set_knobs(monkeypatch, dict(TILE_ENV, VPIC_HIP_TAIL_SORT_MIN="1"))
    n = 6000
    p = still_particles(grid, "random", n, tagged, 2)
    tail = still_particles(grid, name, n_tail, tagged, 3)
    tail["tag"] += 10 ** 6 if tagged else 0
    e = engine_for(V, grid, dt=0.5)
    e.set_vacuum()
    e.load_interpolator()
    sp = e.new_species(-1.0, n + n_tail + 64, 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    sorted_in = e.get_particles(sp)
    S.check(sorted_in, p, grid, "tile")
    e.append_particles(sp, tail)
    e.clear_accumulators()
    assert e.advance_p(sp) == 0
    got = e.get_particles(sp)
    assert len(got) == n + n_tail
    assert bits_equal(got[:n], sorted_in)
    S.check(got[n:], tail, grid, "tile_only")
    e.close()


@pytest.mark.parametrize("tagged", TAGS, ids=TAG_IDS)
@pytest.mark.parametrize("grid", S.MAIN_GRIDS, ids=S.grid_id)
def test_the_tail_is_regrouped_with_dead_slots_in_it(V, L, monkeypatch, grid, tagged):
    """P9h: doomed particles (ux = 3, on their way through the absorbing +x wall) appended IN THE TAIL; one step of the
    resident exchange removes them and leaves their slots dead.  The next identity push regroups the tail again: the live
    tail is the appended survivors grouped by tile, and the dead slots are the last slots of the extent
    (tail_copy_back_kernel, `k >= *n_live`)."""
    set_knobs(monkeypatch, dict(TILE_ENV, VPIC_HIP_TAIL_SORT_MIN="1"))
    nx, ny, nz = grid
    n, n_tail, n_doomed = 6000, 3000, 40
    p = still_particles(grid, "random", n, tagged, 4)
    tail = still_particles(grid, "random", n_tail + n_doomed, tagged, 5)
    tail["tag"] += 10 ** 6 if tagged else 0
    rng = np.random.default_rng(6)
    doomed = np.sort(rng.choice(n_tail + n_doomed, n_doomed, replace=False))     # all over the tail
    tail["i"][doomed] = L.voxel(nx, rng.integers(1, ny + 1, n_doomed), rng.integers(1, nz + 1, n_doomed), nx, ny, nz)
    tail["dx"][doomed], tail["ux"][doomed] = 0.99, 3.0
    survivors = np.delete(tail, doomed)
    e = engine_for(V, grid, dt=0.02, pbc=[L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0])
    e.set_vacuum()
    e.load_interpolator()
    sp = e.new_species(-1.0, n + len(tail) + 64, 8192)
    e.set_particles(sp, p)
    e.sort_p(sp)
    sorted_in = e.get_particles(sp)
    e.append_particles(sp, tail)
    e.clear_accumulators()
    e.exchange_begin()
    e.advance_p_async(sp)
    e.exchange_pack([0] * 6, [0] * 6, 8192)
    e.exchange_finish([])
    assert e.exchange_flags == 0
    assert e.species_stats(sp)["dead_slots"] == n_doomed and e.np(sp) == n + n_tail
    e.clear_accumulators()
    assert e.advance_p(sp) == 0                             # the identity on the survivors; regroups the tail, dead slots and all
    assert e.species_stats(sp)["dead_slots"] == n_doomed and e.capacity(sp)[0] == n + n_tail + n_doomed
    r = e.select(sp, index=True)
    assert r.count == n + n_tail
    assert np.array_equal(r.index, np.arange(n + n_tail))   # the live particles first: the dead slots are the last of the extent
    assert bits_equal(r.particles[:n], sorted_in)
    S.check(r.particles[n:], survivors, grid, "tile_only")
    e.close()


def test_the_matrix_covers_every_path():
    """The parameter lists themselves: every path P1-P9, every grid in both key orders, every np edge on (7,9,6) under P1,
    P4 and P6, every arrangement under P1-P6 (P3: every one that may be pushed)."""
    assert set(S.GRIDS) == {(1, 1, 1), (3, 5, 2), (4, 4, 4), (5, 4, 4), (7, 9, 6), (62, 3, 2), (63, 2, 3), (16, 8, 12), (40, 40, 40), (66, 64, 64)}
    assert S.NP_EDGES == (0, 1, 63, 64, 65, 257, 2047, 2048, 2049, 14341, 16384, 16385, 18435, 81937)
    assert S.ARRANGEMENTS == ("random", "sorted", "reversed", "one_cell", "round_robin_20", "nearly", "ghosts")
    assert {c[0] for c in PURE_CASES} == set(PURE) and set(PURE) | {"P3"} == set(PATHS)
    assert {PATHS[path][0] for path in PURE} == set(S.ORDERS)
    for grid in S.GRIDS:                                    # every grid in both key orders (and by tile only, and the old kernels)
        for path in PURE:
            for name in ("random", "nearly"):
                assert (path, grid, name, S.default_n(grid)) in PURE_CASES, (path, grid, name)
    for path in ("P1", "P4", "P6"):
        for n in S.NP_EDGES:
            assert (path, (7, 9, 6), "random", n) in PURE_CASES, (path, n)
    for grid in S.MAIN_GRIDS:
        for name in S.ARRANGEMENTS:
            for path in PURE:
                assert (path, grid, name, S.default_n(grid)) in PURE_CASES, (path, grid, name)
            assert name == "ghosts" or (grid, name) in P3_CASES
    assert len(PURE_CASES) == len(set(PURE_CASES)) == 3 * 14 + 5 * 2 * 7 + 5 * 8 * 2
    assert TAGS == [True, False]
    assert set(HOLES_CASES) == {(path, grid) for path in ("P1", "P4", "P6") for grid in S.MAIN_GRIDS}       # dead slots
    assert {g for g, _ in PUSH_CASES} == {(7, 9, 6), (5, 4, 4), (16, 8, 12)} and ((7, 9, 6), "reflecting_z") in PUSH_CASES   # P7, P8
    assert {g for g, _, _ in TAIL_CASES} == set(S.MAIN_GRIDS) and min(t for _, _, t in TAIL_CASES) == 1     # P9 (P9h: both main grids)
    for fn in (test_sort_p, test_sort_p_of_a_hot_species_in_voxel_order, test_a_sort_drops_the_dead_slots, test_a_sort_counted_by_the_push_before,
               test_the_sort_inside_the_push, test_the_tail_is_regrouped_by_tile, test_the_tail_is_regrouped_with_dead_slots_in_it):
        assert not any(m.name in ("skip", "skipif", "xfail") for m in getattr(fn, "pytestmark", []))
