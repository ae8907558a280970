"""The hydro moments of a selection of a species, summed on the device (vpic_hip_accumulate_hydro_p_select,
csrc/moments.hip), against tests/test_moments_select_ref.py: the oracle's accumulate_hydro_p on the rows that keep_mask
keeps.  The deck is that file's (the 10 x 7 x 3 grid of test_gpu_moments.py with q drawn from four values); the array
states are those of species_states.py -- "unsorted", "voxel", "tile", "tile_only" (a fresh child process), "tile_tail_holes"
-- built as test_gpu_moments.py builds them: the grid has an axis thinner than a tile, so the states in tile order are
made under VPIC_HIP_WINDOW=tile.  "tile_tail_holes" holds other particles than the inputs (600 appended, 60 absorbed, all
pushed once), so every state is compared with the oracle on what get_particles returns for it.

One engine per (state, mode) serves all selections: measure() makes every call once and the parametrised cases look at
their part of what it returned.

Float mode: within ACC_TOL = 2e-6 of each moment's largest entry in the reference.  Deterministic mode: BIT FOR BIT equal
to accumulate_hydro_p of a second species of the same q_m that holds exactly the particles select() returns for the
descriptor -- both calls use the fixed-point scale of |q| = 0.015, which every kept subset contains (asserted here on the
returned particles, and on the inputs by the CPU test) -- and equal across the states that hold the same particles.

The selected moments against an exact reference, word for word (deterministic) and within a derived per-node bound (float),
at the whole species' scale: tests/test_gpu_moments_exact.py::test_the_moments_of_a_selection."""
import ctypes as C
import functools
import importlib
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_moments as M  # noqa: E402
import test_moments_select_ref as R  # noqa: E402
from species_states import STATES, package, run_child  # noqa: E402
from test_fieldcoord_ref import keep_mask  # noqa: E402

pytestmark = pytest.mark.gpu
ACC_TOL = 2e-6
GRID, N, SEED = R.GRID, R.N, R.SEED
N_TAIL, N_DOOMED = M.N_TAIL, M.N_DOOMED
IN_TILE_ORDER = ("tile", "tile_only", "tile_tail_holes")
SAME_PARTICLES = ("unsorted", "voxel", "tile", "tile_only")              # the inputs, in another order
SELECTIONS = list(R.selections())
MODES = ["float", "deterministic"]


def build_state(state, mode, perm_seed=1):
    """(engine, species) holding the deck's particles, uploaded in the order of a permutation, in the array state asked for
    (test_gpu_moments.build_state with the charges of test_moments_select_ref)"""
    V = package()
    L = V.layout
    f, fi, p = R.inputs()
    holes = state == "tile_tail_holes"
    g, _ = M.grids(V, L, state)
    e = M.new_engine(V, g, state in IN_TILE_ORDER)
    e.set_fields(np.array(f)); e.set_interpolator(np.array(fi))
    e.set_accumulation(mode)
    sp = e.new_species(-1.0, N + N_TAIL + N_DOOMED + 4096, 4096)
    p = np.array(p)
    if holes:
        p = R.discrete_charges(M.make_particles(SEED + 1, spread=0.95), SEED + 7)
        rng = np.random.default_rng(5)
        d = R.discrete_charges(M.make_particles(SEED + 2, N_DOOMED, first_tag=10 ** 7), SEED + 8)
        d["i"] = L.voxel(GRID[0], rng.integers(1, GRID[1] + 1, N_DOOMED), rng.integers(1, GRID[2] + 1, N_DOOMED), *GRID)
        d["dx"], d["ux"] = 0.99, 3.0                     # on their way through the absorbing +x wall
        p = np.concatenate([p, d])
    p = p[np.random.default_rng(perm_seed).permutation(len(p))]
    e.set_particles(sp, p)
    if state == "voxel":
        e.sort_p(sp)
        assert e.species_order(sp) == "voxel"
    if state in IN_TILE_ORDER:
        e.sort_p(sp)
        assert e.species_order(sp) == "tile"
        assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0)
    if holes:
        t = R.discrete_charges(M.make_particles(SEED + 3, N_TAIL, spread=0.95, first_tag=2 * 10 ** 7), SEED + 9)
        e.append_particles(sp, t[np.random.default_rng(perm_seed + 1).permutation(N_TAIL)])
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(sp)
        e.exchange_pack([0] * 6, [0] * 6, 4096)
        e.exchange_finish([])
        assert e.exchange_flags == 0
        assert e.species_stats(sp)["dead_slots"] == N_DOOMED
        assert e.np(sp) == N + N_TAIL
    return e, sp


def selected_hydro(e, sp, desc):
    """clear_hydro, the selected call, get_hydro.  (Engine.accumulate_hydro_p without a selection argument makes the
    whole-species call, so the descriptor that names nothing goes to the entry point itself.)"""
    e.clear_hydro()
    if desc:
        e.accumulate_hydro_p(sp, **desc)
    else:
        d = importlib.import_module("old-vpic_amd.engine").select_desc()
        e._ck(e._l.vpic_hip_accumulate_hydro_p_select(e._h, sp, C.byref(d)))
    return e.get_hydro()


def measure_on_device(state, mode):
    """every call of one (state, mode), once: per selection the selected moments, their statistics and select_count; in
    deterministic mode also the moments of a second species made of what select() returns, and the largest |q| of those
    particles; at the end the whole species' plain moments and its particles.  A dict of arrays (it travels through an
    .npz file from the child process of "tile_only")."""
    e, sp = build_state(state, mode)
    order = e.species_order(sp)
    out = {}
    other = e.new_species(-1.0, N + N_TAIL + 4096, 4096) if mode == "deterministic" else None
    for name, desc in R.selections().items():
        out[f"h:{name}"] = selected_hydro(e, sp, desc)
        out[f"stats:{name}"] = np.array(e.moments_stats(), np.int64)
        out[f"count:{name}"] = np.array(e.select_count(sp, **desc), np.int64)
        if mode == "deterministic":
            r = e.select(sp, **desc)
            assert r.count == len(r.particles)
            e.clear_hydro()
            if r.count:
                e.set_particles(other, r.particles)
                e.accumulate_hydro_p(other)
            out[f"ref:{name}"] = e.get_hydro()
            out[f"qtop:{name}"] = np.array(np.abs(r.particles["q"]).max() if r.count else 0.0, np.float32)
        assert e.species_order(sp) == order, name
    e.clear_hydro(); e.accumulate_hydro_p(sp)                 # (last: a deterministic whole-species call may sort)
    out["h:plain"] = e.get_hydro()
    out["particles"] = e.get_particles(sp)
    e.close()
    return out


@functools.lru_cache(maxsize=None)
def measure(state, mode):
    if state != "tile_only":
        return measure_on_device(state, mode)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        with M.environment(VPIC_HIP_WINDOW="tile"):
            run_child(__file__, ["tile_only", mode, path], 300)          # (sets VPIC_HIP_TILE_COARSE=1)
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def oracle_of(state, mode, name):
    """(oracle hydro of the kept rows of the state's particles, how many are kept)"""
    back = measure(state, mode)["particles"]
    assert len(back) == (N + N_TAIL if state == "tile_tail_holes" else N)
    ref, keep = R.selected_hydro_ref(back, R.inputs()[1], R.selections()[name])
    return ref, int(keep.sum())


def assert_close(got, ref, what):
    for c in M.moments(ref):
        err, top = float(np.abs(got[c].astype(np.float64) - ref[c]).max()), float(np.abs(ref[c]).max())
        print(f"{what} {c}: max error {err:.3e}, largest entry {top:.3e}, ratio {err / top if top else 0.0:.2e}")
        assert err <= ACC_TOL * top, (what, c)


def check_stats(state, name, stats, count, kept):
    """out[0] is select_count's number (and the reference's), out[1] + out[2] == out[0]; a species in tile order goes
    through its tiles' LDS windows, any other through global memory alone"""
    print(f"{state} {name}: statistics {tuple(stats)}, select_count {count}, the reference keeps {kept}")
    assert stats[0] == count == kept and stats[1] + stats[2] == stats[0] and stats[3] == 0
    if state in IN_TILE_ORDER:
        assert (stats[1] > 0) == (kept > 0)
        if state != "tile_tail_holes":
            assert stats[2] == 0
    else:
        assert stats[1] == 0


@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("state", STATES)
def test_float_mode(state, name):
    """clear_hydro, the selected call, get_hydro: the oracle on the kept rows within ACC_TOL; the empty selection leaves
    the array all zero; moments_stats()[0] is select_count's number."""
    got = measure(state, "float")
    ref, kept = oracle_of(state, "float", name)
    h = got[f"h:{name}"]
    assert_close(h, ref, f"{state} {name}")
    check_stats(state, name, got[f"stats:{name}"], int(got[f"count:{name}"]), kept)
    if name == "empty":
        assert kept == 0 and not h.view(np.uint8).any()
    elif name != "all":
        assert 100 <= kept <= len(got["particles"]) - 100
    if name == "all":
        assert_close(got["h:plain"], ref, f"{state} whole species")


@pytest.mark.parametrize("name", SELECTIONS)
@pytest.mark.parametrize("state", STATES)
def test_deterministic_mode(state, name):
    """bit for bit the moments of a species made of what select() returns; "all" bit for bit the plain call's; the same
    bytes in every state that holds the same particles; and within ACC_TOL of the oracle."""
    got = measure(state, "deterministic")
    ref, kept = oracle_of(state, "deterministic", name)
    h_sel, h_ref = got[f"h:{name}"], got[f"ref:{name}"]
    if kept:
        assert float(got[f"qtop:{name}"]) == float(np.abs(R.Q_TOP))       # the two species share their fixed-point scale
    print(f"{state} {name}: words that differ from the moments of the selected particles as a species "
          f"{int((M.hydro_bits(h_sel) != M.hydro_bits(h_ref)).sum())}")
    assert h_sel.tobytes() == h_ref.tobytes()
    assert_close(h_sel, ref, f"{state} {name}")
    check_stats(state, name, got[f"stats:{name}"], int(got[f"count:{name}"]), kept)
    if name == "all":
        assert h_sel.tobytes() == got["h:plain"].tobytes()
    if name == "empty":
        assert not h_sel.view(np.uint8).any()
    if state in SAME_PARTICLES:
        base = measure("tile", "deterministic")[f"h:{name}"]
        print(f"{state} {name}: words that differ from state tile {int((M.hydro_bits(h_sel) != M.hydro_bits(base)).sum())}")
        assert h_sel.tobytes() == base.tobytes()


@pytest.mark.parametrize("state", ["unsorted", "tile"])
@pytest.mark.parametrize("mode", MODES)
def test_the_species_is_left_alone(mode, state):
    """particles, sort order, tile partition and species_stats are identical before and after selected calls -- also in
    deterministic mode on an unsorted species, which the whole-species call would sort under VPIC_HIP_WINDOW=tile."""
    V = package()
    f, fi, p = R.inputs()
    e = M.new_engine(V, M.grids(V, V.layout)[0], True)      # (an engine that WOULD push the species in tile order)
    e.set_fields(np.array(f)); e.set_interpolator(np.array(fi)); e.set_accumulation(mode)
    sp = e.new_species(-1.0, N + 4096, 4096)
    e.set_particles(sp, np.array(p)[np.random.default_rng(7).permutation(N)])
    if state == "tile":
        e.sort_p(sp)

    def snapshot():
        return (e.get_particles(sp).tobytes(), e.species_order(sp), e.get_tile_partition(sp).tobytes() if state == "tile" else b"",
                e.species_stats(sp), e.np(sp), e.nm(sp))
    before = snapshot()
    assert before[1] == ("tile" if state == "tile" else "none")
    for name in ("box", "ke_pitch", "every", "all"):
        selected_hydro(e, sp, R.selections()[name])
        stats = e.moments_stats()
        assert (stats[1] > 0) == (state == "tile") and stats[1] + stats[2] == stats[0] > 0
        assert snapshot() == before, name
    if mode == "deterministic" and state == "unsorted":
        e.clear_hydro(); e.accumulate_hydro_p(sp)             # the whole-species call does sort here: the check above can fail
        assert e.species_order(sp) == "tile"
    e.close()


def test_argument_errors_leave_the_array_unchanged():
    """every failure the header lists returns non-zero with a message, and the hydro array keeps its bytes"""
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    e, sp = build_state("tile", "float")
    e.clear_hydro(); e.accumulate_hydro_p(sp)
    h0 = e.get_hydro().tobytes()
    call = e._l.vpic_hip_accumulate_hydro_p_select

    def desc(**kw):
        d = eng.select_desc([("ke", 0.0, 1.0)])
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def bad_coord(c):
        d = desc()
        d.sel[0].coord = c
        return d

    cases = {
        "bad sp": (sp + 7, desc()), "negative sp": (-1, desc()), "NULL s": (sp, None),
        "n_sel -1": (sp, desc(n_sel=-1)), "n_sel 5": (sp, desc(n_sel=5)),
        "coordinate 8": (sp, bad_coord(8)), "coordinate 22": (sp, bad_coord(22)), "coordinate -1": (sp, bad_coord(-1)),
        "flag bit 4": (sp, desc(flags=4)), "flag bits 3 | 8": (sp, desc(flags=11, tag_every=2)),
        "tag_every 0": (sp, desc(flags=eng.SELECT_TAG_EVERY, tag_every=0)),
        "tag_phase == every": (sp, desc(flags=eng.SELECT_TAG_EVERY, tag_every=16, tag_phase=16)),
        "tag_phase -1": (sp, desc(flags=eng.SELECT_TAG_EVERY, tag_every=16, tag_phase=-1)),
    }
    for what, (species, d) in cases.items():
        rc = call(e._h, species, C.byref(d) if d is not None else None)
        msg = e._l.vpic_hip_last_error().decode()
        print(f"{what}: rc {rc}, {msg!r}")
        assert rc != 0 and msg, what
        assert e.get_hydro().tobytes() == h0, what
    with pytest.raises(KeyError):
        e.accumulate_hydro_p(sp, select=[("pitch", 0.0, 1.0)])
    with pytest.raises(V.VpicHipError):
        e.accumulate_hydro_p(sp, tag_every=(0, 0))
    assert e.get_hydro().tobytes() == h0
    # a good call still adds: twice the moments of the whole species
    e.accumulate_hydro_p(sp, select=[("ke", 0.0, R.INF)])
    assert_close(e.get_hydro(), M.reference(np.concatenate([R.inputs()[2]] * 2), -1.0, R.inputs()[1])[0], "added to what was there")
    e.close()


def test_out_of_range_refusal_and_small_species():
    """deterministic mode: a kept particle at |u| = 2^40 makes the call fail with the error that names the range and adds
    nothing; a selection that leaves it out is summed.  A chargeless species adds nothing, an empty one neither."""
    V = package()
    fi = R.inputs()[1]
    e, sp = build_state("tile", "deterministic")
    one = np.array(R.inputs()[2][:1])
    one["ux"], one["tag"] = 2.0 ** 40, 10 ** 8
    e.append_particles(sp, one)
    e.clear_hydro()
    with pytest.raises(V.VpicHipError, match="range"):
        e.accumulate_hydro_p(sp, select=[("ux", -10.0, R.INF)])
    stats = e.moments_stats()
    assert stats[0] == N + 1 and stats[3] >= 1
    assert not e.get_hydro().view(np.uint8).any()
    e.accumulate_hydro_p(sp, select=[("ux", -10.0, 10.0)])
    assert e.moments_stats() == (N, N, 0, 0)
    assert e.get_hydro().tobytes() == measure("tile", "deterministic")["h:all"].tobytes()
    for mode in MODES:
        e.set_accumulation(mode, 0.01)
        ghost, empty = e.new_species(-1.0, 4096, 64), e.new_species(-1.0, 4096, 64)
        z = np.array(R.inputs()[2][::10])
        z["q"] = 0
        e.set_particles(ghost, z)
        h = selected_hydro(e, ghost, R.selections()["box"])
        assert e.moments_stats()[0] == int(keep_mask(z, GRID, fi, R.selections()["box"]).sum()) > 0
        assert not (M.hydro_bits(h) & 0x7fffffff).any()                   # (every contribution is +-0)
        h = selected_hydro(e, empty, R.selections()["every"])
        assert e.moments_stats() == (0, 0, 0, 0) and not h.view(np.uint8).any()
    e.close()


if __name__ == "__main__":
    assert sys.argv[1] == "tile_only"
    np.savez(sys.argv[3], **measure_on_device(sys.argv[1], sys.argv[2]))
    print("child OK")
