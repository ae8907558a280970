"""The reference world of tests/exchange_ref.py, pinned on the CPU: two slabs stepped by the helper against ONE advance_p on
the whole periodic box, and the properties that keep the cases of tests/test_gpu_exchange.py from passing vacuously -- each
asserted on the reference alone, from the same seeded inputs the GPU file uploads."""
import numpy as np
import pytest

import det_exact as X
import exchange_ref as R

L = R.L


def global_cell(p, rank, dims):
    """(x, y, z) of every particle in the whole box of two slabs cut in x"""
    nx, ny, nz = dims
    v = p["i"].astype(np.int64)
    x, y, z = v % (nx + 2), (v // (nx + 2)) % (ny + 2), v // ((nx + 2) * (ny + 2))
    return x + rank * nx, y, z


@pytest.mark.parametrize("dims", R.GRIDS)
def test_two_slabs_step_like_one_domain(orc, dims):
    """Two slabs cut in x, periodic in y and z, one step of the helper with as many rounds as it takes, against one
    orc.advance_p on the whole box (2 nx, ny, nz) with the same interpolator cell for cell: every particle's global
    cell, momentum, charge AND position equal bit for bit, as multisets.  Positions too: both runs walk the same move_p
    segments (a crossing into the neighbour mirrors the coordinate and carries the displacement left, in move_p as in
    boundary_p's injector).  Measured largest position difference on these inputs: 0."""
    nx, ny, nz = dims
    whole = (2 * nx, ny, nz)
    og = orc.make_grid(2 * nx, ny, nz, float(2 * nx), float(ny), float(nz), np.float32(R.DT))
    fi = X.interpolator(og, seed=11)
    n = 2 * R.N_HOT
    p = X.particles(5, n, whole, X.HOT)
    assert R.all_different(p, R.P_WORDS)
    # the slabs
    w = R.World("slabs", dims, fi_seed=None)
    gx = p["i"] % (2 * nx + 2)
    gy, gz = (p["i"] // (2 * nx + 2)) % (ny + 2), p["i"] // ((2 * nx + 2) * (ny + 2))
    X_, Y_, Z_ = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1), indexing="ij")
    for d in w.domains:
        mine = p[(gx - 1) // nx == d.rank].copy()
        mx = gx[(gx - 1) // nx == d.rank] - d.rank * nx
        mine["i"] = L.voxel(mx, gy[(gx - 1) // nx == d.rank], gz[(gx - 1) // nx == d.rank], nx, ny, nz)
        d.add_species(X.Q_M, mine, n)
        d.fi[L.voxel(X_, Y_, Z_, nx, ny, nz)] = fi[L.voxel(X_ + d.rank * nx, Y_, Z_, 2 * nx, ny, nz)]
    for d in w.domains:
        w.push(d.rank, 0)
    assert sum(d.species[0]["nm"] for d in w.domains) > 0
    rounds = w.exchange()
    assert len(rounds) >= 1
    # one domain
    ref = p.copy()
    pm = np.zeros(n, L.particle_mover_t)
    a = np.zeros(og.nv, L.accumulator_t)
    assert orc.advance_p(ref, n, X.Q_M, pm, a, fi, og) == 0
    want = np.zeros(n, [("x", "i8"), ("y", "i8"), ("z", "i8")] + [(c, "f4") for c in ("dx", "dy", "dz", "ux", "uy", "uz", "q")])
    want["x"], want["y"], want["z"] = global_cell(ref, 0, whole)
    got = []
    for d in w.domains:
        live = d.live(0)
        g = np.zeros(len(live), want.dtype)
        g["x"], g["y"], g["z"] = global_cell(live, d.rank, dims)
        for c in ("dx", "dy", "dz", "ux", "uy", "uz", "q"):
            g[c] = live[c]
        got.append(g)
    got = np.concatenate(got)
    for c in ("dx", "dy", "dz", "ux", "uy", "uz", "q"):
        want[c] = ref[c]
    assert len(got) == n
    assert R.same_multiset(got, want, ("x", "y", "z", "ux", "uy", "uz", "q"))
    worst = 0.0
    if not R.same_multiset(got, want, want.dtype.names):          # (measure before failing: momenta are unique keys)
        go, wo = np.argsort(got, order=("ux", "uy", "uz", "q")), np.argsort(want, order=("ux", "uy", "uz", "q"))
        worst = max(float(np.abs(got[c][go].astype(np.float64) - want[c][wo]).max()) for c in ("dx", "dy", "dz"))
    print("largest position difference %.3e" % worst)
    assert worst == 0.0


@pytest.mark.parametrize("dims", R.GRIDS)
@pytest.mark.parametrize("n", R.PATTERN_COUNTS)
def test_pattern_cases_send_exactly_n_through_one_face(dims, n):
    """through_face: each of the n particles is one mover for face +x and nothing else moves; at n = 300 that is the face
    of one species with more than 256 movers (more than one workgroup of the classify kernel)"""
    w = R.pattern_world(dims, n)
    assert w.push(0, 0) == n and w.push(1, 0) == 0
    assert np.all(R.faces_of_movers(w.domains[0], 0) == 3)
    sent = w.round()
    assert list(sent) == [(0, 3)] and len(sent[(0, 3)]) == n
    assert R.all_different(sent[(0, 3)], R.INJ_WORDS)
    assert max(R.PATTERN_COUNTS) > 256


@pytest.mark.parametrize("dims", R.GRIDS)
def test_hot_case_mixes_faces_species_and_rounds(dims):
    """four hot species in a world whose six faces are shared: a wavefront-sized run of 64 consecutive movers leaves through
    at least three different faces; the messages of a later round, species mixed by `interleaved`, hold at least three
    species within 64 consecutive records; at least one arrival stops on a face of the receiver; every record of every
    message has its own bits."""
    w = R.four_species_world("all_shared", dims)
    for d in w.domains:
        for k in range(4):
            assert w.push(d.rank, k) > 64
    face = R.faces_of_movers(w.domains[0], 0)
    assert np.all(face >= 0)
    assert max(len(np.unique(face[k:k + 64])) for k in range(len(face) - 63)) >= 3
    first = w.round()
    assert all(R.all_different(r, R.INJ_WORDS) for r in first.values())
    assert R.all_different(np.concatenate(list(first.values())), R.INJ_WORDS)
    stopped = sum(s["nm"] for d in w.domains for s in d.species)
    assert stopped >= 1
    later = w.round()
    assert later and max(R.species_in_windows(R.interleaved(r)) for r in later.values()) >= 3
    w.exchange()
    for d in w.domains:
        assert R.all_different(np.concatenate([d.live(k) for k in range(4)]), R.P_WORDS)


@pytest.mark.parametrize("dims", R.GRIDS)
def test_corner_particle_needs_three_rounds(dims):
    """x face, then y, then z: the corner particle (known by its charge, which no other particle has) is in a message of
    each of three rounds, through faces +x, +y, +z"""
    w = R.corner_world(dims)
    q = R.corner_particle(dims)["q"][0]
    for d in w.domains:
        w.push(d.rank, 0)
    rounds = w.exchange()
    assert len(rounds) >= 3
    where = [[key for key, rec in r.items() if np.any(rec["q"] == q)] for r in rounds[:3]]
    assert where == [[(0, 3)], [(1, 4)], [(0, 5)]]
    assert sum(int(np.sum(d.live(0)["q"] == q)) for d in w.domains) == 1


@pytest.mark.parametrize("dims", R.GRIDS)
def test_absorbing_case_shares_nodes(dims):
    """at least 64 particles are absorbed onto nodes that another absorbed particle adds to as well; the addends the helper
    takes from the reference one particle at a time sum to the reference's rhob within the bound of a float sum in
    another order"""
    w = R.absorbing_world(dims)
    d = w.domains[0]
    assert w.push(0, 0) > 0
    nodes, addends = R.absorbed_addends(d, 0)
    hits = np.bincount(nodes.reshape(-1), minlength=d.og.nv)
    assert int(np.sum((hits[nodes] >= 2).any(axis=1))) >= 64
    nm = d.species[0]["nm"]
    per_face = w.pack(0)
    assert len(nodes) == nm - sum(len(r) for r in per_face)
    assert [len(r) > 0 for r in per_face] == [False, False, False, True, False, False]
    exact, bound = R.rhob_bound(d.og.nv, nodes, addends)
    assert np.all(np.abs(d.f["rhob"].astype(np.float64) - exact) <= bound)
    assert np.abs(exact).max() > 0


def test_multiset_helpers():
    a = np.zeros(3, L.particle_t)
    a["dx"] = [0.0, -0.0, 1.0]
    assert R.all_different(a, R.P_WORDS)                           # +0 and -0 are different bits
    b = a[[2, 0, 1]]
    assert R.same_multiset(a, b, R.P_WORDS) and R.sub_multiset(a[:2], b, R.P_WORDS)
    assert not R.sub_multiset(a[[0, 0]], b, R.P_WORDS) and not R.same_multiset(a[:2], b, R.P_WORDS)
    assert not R.all_different(a[[0, 1, 0]], R.P_WORDS)
