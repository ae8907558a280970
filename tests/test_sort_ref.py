"""tests/sort_ref.py, the numpy reference and checker of the sorts, on the CPU: pinned on the oracle's sort_p (itself pinned
on the compiled reference by K7, test_oracle_golden.py), its tile keys a bijection, its checker shown to notice every kind of
damage, and the properties of the seeded inputs that the GPU cases (test_gpu_sort.py) rely on to reach the kernels' edges
asserted, not assumed."""
import numpy as np
import pytest

import sort_ref as S

ORACLE_GRIDS = [g for g in S.GRIDS if g not in ((40, 40, 40), (66, 64, 64))]


def sorted_copy(p, grid, order):
    return p[np.argsort(S.keys(p["i"], grid, order), kind="stable")]


@pytest.mark.parametrize("name", ["random", "nearly", "ghosts"])
@pytest.mark.parametrize("grid", ORACLE_GRIDS, ids=S.grid_id)
def test_against_the_oracle(orc, grid, name):
    """starts(.., "voxel") is the partition of the oracle's sort_p, and check accepts the oracle's output"""
    n = S.default_n(grid)
    for tagged in (True, False):
        p = S.case_particles(grid, name, n, "voxel", tagged)
        g = orc.make_grid(*grid, *[float(d) for d in grid], np.float32(0.3))
        out, part = p.copy(), np.zeros(g.nv + 1, np.int32)
        orc.sort_p(out, n, part, g)
        assert g.nv == S.nv_of(grid)
        assert np.array_equal(S.starts(p["i"], grid, "voxel"), part)
        S.check(out, p, grid, "voxel", partition=part)
    if name == "ghosts":
        assert p["i"].min() == 0 and p["i"].max() == S.nv_of(grid) - 1


@pytest.mark.parametrize("grid", list(S.GRIDS), ids=S.grid_id)
def test_tile_keys_are_a_bijection(grid):
    """from the interior cells onto {64 t + c} restricted to the cells that exist; and the tile of a key is key // 64"""
    nx, ny, nz = grid
    ntx, nty, ntz = S.tiles_of(grid)
    inside = S.interior(grid)
    k = S.keys(inside, grid, "tile")
    assert len(np.unique(k)) == len(inside) == nx * ny * nz
    t, c = np.divmod(np.arange(ntx * nty * ntz * 64), 64)
    tx, ty, tz = t % ntx, t // ntx % nty, t // (ntx * nty)
    exists = (4 * tx + (c & 3) < nx) & (4 * ty + (c >> 2 & 3) < ny) & (4 * tz + (c >> 4) < nz)
    assert np.array_equal(np.sort(k), np.flatnonzero(exists))
    assert np.array_equal(S.keys(inside, grid, "tile_only"), k // 64)
    # a ghost voxel has the key of the interior voxel that clamping each of its cell indices into the interior gives
    gh = S.ghosts_of(grid)
    cx, cy, cz = S.cells(gh, grid)
    near = np.clip(cx, 1, nx) + (nx + 2) * (np.clip(cy, 1, ny) + (ny + 2) * np.clip(cz, 1, nz))
    assert np.array_equal(S.keys(gh, grid, "tile"), S.keys(near, grid, "tile"))
    assert len(gh) + len(inside) == S.nv_of(grid) and gh[0] == 0 and gh[-1] == S.nv_of(grid) - 1


def test_the_arrangements_are_what_they_say():
    rng = np.random.default_rng(1)
    for grid in S.MAIN_GRIDS:
        inside = set(S.interior(grid).tolist())
        for order in S.ORDERS:
            n = 4321
            i = S.arrangement("sorted", rng, grid, n, order)
            assert np.all(np.diff(S.keys(i, grid, order)) >= 0)
            i = S.arrangement("reversed", rng, grid, n, order)
            assert np.all(np.diff(S.keys(i, grid, order)) <= 0) and len(set(i.tolist())) > 1
            i = S.arrangement("nearly", rng, grid, n, order)
            descents = int((np.diff(S.keys(i, grid, order)) < 0).sum())
            assert 0 < descents <= 2 * (n // 20)
        assert len(set(S.arrangement("one_cell", rng, grid, 500).tolist())) == 1
        i = S.arrangement("round_robin_20", rng, grid, 640)
        for w in range(10):                                            # every wavefront: 20 distinct voxels, more than MAX_GROUPS = 16
            assert len(set(i[64 * w:64 * w + 64].tolist())) == 20
        assert len(set(S.keys(i, grid, "tile_only").tolist())) == min(20, S.ntiles_of(grid))
        for name in S.ARRANGEMENTS:
            i = S.arrangement(name, rng, grid, 3000)
            assert i.dtype == np.int32 and len(i) == 3000 and i.min() >= 0 and i.max() < S.nv_of(grid)
            assert (name == "ghosts") == (not set(i.tolist()) <= inside)
        i = S.arrangement("ghosts", rng, grid, 3000)
        assert i.min() == 0 and i.max() == S.nv_of(grid) - 1 and sum(v not in inside for v in i.tolist()) == 60
    p = S.particles(rng, S.arrangement("random", rng, (7, 9, 6), 100000), True)
    for name in S.WORDS[1:]:
        assert np.all(np.isfinite(p[name]))
    assert len(np.unique(p["tag"])) == len(p) and p["tag"].min() == 1


CORRUPTIONS = ["duplicated", "swapped", "last_bit", "partition_off_by_one", "tpart_end", "dead_slot"]


@pytest.mark.parametrize("tagged", [True, False], ids=["tagged", "tagless"])
@pytest.mark.parametrize("damage,order", [(d, o) for d in CORRUPTIONS for o in S.ORDERS
                                          if not (d == "partition_off_by_one" and o != "voxel") and not (d == "tpart_end" and o == "voxel")])
def test_the_checker_notices(damage, order, tagged):
    """a correct output passes; each corruption of it makes check raise"""
    grid, n = (7, 9, 6), 5000
    p = S.case_particles(grid, "random", n, order, tagged)
    good = sorted_copy(p, grid, order)
    part = S.starts(p["i"], grid, "voxel").astype(np.int32) if order == "voxel" else None
    tpart = S.starts(p["i"], grid, order).astype(np.int32) if order != "voxel" else None
    S.check(good, p, grid, order, partition=part, tpart=tpart)
    S.check(good[::-1][np.argsort(S.keys(good[::-1]["i"], grid, order), kind="stable")], p, grid, order, partition=part, tpart=tpart)   # the order inside a key is free
    k = S.keys(good["i"], grid, order)
    bad, bad_part, bad_tpart = good.copy(), part, tpart
    if damage == "duplicated":
        j = int(np.flatnonzero(np.diff(k) == 0)[7])                    # over its neighbour of the same key: the order still holds
        bad[j + 1] = bad[j]
    elif damage == "swapped":
        j = int(np.flatnonzero(np.diff(k) > 0)[5])
        bad[[j, j + 1]] = bad[[j + 1, j]]
    elif damage == "last_bit":
        w = bad["uy"].view(np.uint32)
        w[1234] ^= 1
    elif damage == "partition_off_by_one":
        bad_part = part.copy()
        bad_part[len(part) // 2] += 1
    elif damage == "tpart_end":
        bad_tpart = tpart.copy()
        bad_tpart[-1] -= 1
    elif damage == "dead_slot":
        bad["i"][n // 3] = -1
    with pytest.raises(AssertionError):
        S.check(bad, p, grid, order, partition=bad_part, tpart=bad_tpart)
    if damage == "dead_slot":                                          # ... and one kept beside all the live ones
        with pytest.raises(AssertionError):
            S.check(np.concatenate([good, bad[n // 3:n // 3 + 1]]), p, grid, order)
    if damage == "tpart_end" and order == "tile":                      # one entry in the middle off by one as well
        bad_tpart = tpart.copy()
        bad_tpart[len(tpart) // 2] += 1
        with pytest.raises(AssertionError):
            S.check(good, p, grid, order, tpart=bad_tpart)


def full_chunks(i):
    return [i[c:c + S.CHUNK] for c in range(0, len(i) - S.CHUNK + 1, S.CHUNK)]


def test_the_conditions_the_gpu_cases_rely_on():
    """The seeded inputs do reach the branches their grids are there for (thresholds: particles.hip)."""
    # (16,8,12): every 2048-particle chunk of `random` holds more distinct cells than the workgroup's table has slots, in
    # either order (the keys are a bijection of the cells): wg_count_kernel / wg_scatter_kernel take `slot == -1`
    grid = (16, 8, 12)
    for order in S.ORDERS:
        chunks = full_chunks(S.case_voxels(grid, "random", S.default_n(grid), order))
        assert len(chunks) >= 5
        assert min(len(np.unique(c)) for c in chunks) > S.WG_TABLE
    # (40,40,40): ... more distinct TILES than the table of wg_scatter_kernel<true, true>, and so than coarse_count_kernel's
    grid = (40, 40, 40)
    for order in S.ORDERS:
        chunks = full_chunks(S.case_voxels(grid, "random", S.default_n(grid), order))
        assert len(chunks) >= 5
        fewest = min(len(np.unique(S.keys(c, grid, "tile_only"))) for c in chunks)
        assert fewest > S.WG_TABLE > S.COARSE_TABLE
    # (66,64,64): the scan takes more blocks than scan_blocks_kernel handles in one round, in both orders
    grid = (66, 64, 64)
    for order in ("voxel", "tile"):
        assert (S.n_keys(grid, order) + 1 + S.SCAN_BLOCK - 1) // S.SCAN_BLOCK > S.SCAN_BLOCKS_PER_ROUND
    # round_robin_20: more distinct keys in every wavefront than group_info follows (MAX_GROUPS = 16), in voxel and tile
    # order on both main grids, by tile only where the grid has 20 tiles
    for grid in S.MAIN_GRIDS:
        i = S.case_voxels(grid, "round_robin_20", S.default_n(grid))
        for order in ("voxel", "tile") + (("tile_only",) if S.ntiles_of(grid) >= 20 else ()):
            assert min(len(np.unique(S.keys(i[w:w + 64], grid, order))) for w in range(0, len(i) - 63, 64)) > 16
    # one_cell, sorted: runs of equal keys cross wavefront and chunk boundaries
    for grid in S.MAIN_GRIDS:
        i = S.case_voxels(grid, "sorted", S.default_n(grid), "voxel")
        assert any(i[c - 1] == i[c] for c in range(S.CHUNK, len(i), S.CHUNK)) and any(i[c - 1] == i[c] for c in range(64, len(i), 64))
    # the np edges: 7, 8, 9 and 40 chunks, and a remainder for all but 16384
    assert [(-(-n // S.CHUNK), n % S.CHUNK != 0) for n in (14341, 16384, 18435, 81937)] == [(8, True), (8, False), (10, True), (41, True)]
    assert [n // S.CHUNK for n in (14341, 16384, 18435, 81937)] == [7, 8, 9, 40]
    # ghosts: voxel 0 and voxel nv - 1 are there
    for grid in S.MAIN_GRIDS:
        i = S.case_voxels(grid, "ghosts", S.default_n(grid))
        assert i.min() == 0 and i.max() == S.nv_of(grid) - 1
