"""The sorts' reference and checker, in plain numpy (no GPU): what tests/test_sort_ref.py pins on the oracle and
tests/test_gpu_sort.py holds every path of k_sort_p, the tail regrouping and the sort inside the push to.  Everything
here is exact: integer keys, integer starts, particle records compared as bit patterns.

Orders.  "voxel": the reference's, key = voxel index (sort_p.c:48-58), nv keys.  "tile": the engine's own (engine.h,
sort_key<true>): 4x4x4-cell tiles over the interior, tile-major, cell within the tile; key = 64 tile + cell, 64 ntiles keys
-- a partial tile counts as a whole one, its cells beyond the grid are keys that nothing has.  "tile_only": key = tile
(the tile key // 64).  A voxel of a ghost layer (the reference's sort_p takes any voxel of the grid) has the tile key of
the nearest interior cell: each of its cell indices clamped into the interior."""
import importlib

import numpy as np

TILE_EDGE, TILE_CELLS = 4, 64
ORDERS = ("voxel", "tile", "tile_only")
ARRANGEMENTS = ("random", "sorted", "reversed", "one_cell", "round_robin_20", "nearly", "ghosts")
WORDS = ("i", "dx", "dy", "dz", "ux", "uy", "uz", "q")


def particle_dtype():
    return importlib.import_module("old-vpic_amd.layout").particle_t


def nv_of(grid):
    nx, ny, nz = grid
    return (nx + 2) * (ny + 2) * (nz + 2)


def tiles_of(grid):
    """(ntx, nty, ntz): tiles along every axis, the last one of an axis may be partial"""
    return tuple((n + TILE_EDGE - 1) // TILE_EDGE for n in grid)


def ntiles_of(grid):
    ntx, nty, ntz = tiles_of(grid)
    return ntx * nty * ntz


def n_keys(grid, order):
    """keys the starts of an order have an entry for: nv, or 64 per tile (by tile only too: tpart[] keeps its shape)"""
    return nv_of(grid) if order == "voxel" else ntiles_of(grid) * TILE_CELLS


def cells(i, grid):
    """(cx, cy, cz) of voxel indices, ghost layers included (interior cells from 1): the integer divisions written out"""
    nx, ny, nz = grid
    i = np.asarray(i).astype(np.int64)
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    cz = i // sz
    rem = i - cz * sz
    cy = rem // sy
    cx = rem - cy * sy
    return cx, cy, cz


def keys(i, grid, order):
    """int64 sort keys of voxel indices i in `order` (the module's docstring states the orders)"""
    assert order in ORDERS, order
    i = np.asarray(i).astype(np.int64)
    if order == "voxel":
        return i
    nx, ny, nz = grid
    ntx, nty, ntz = tiles_of(grid)
    cx, cy, cz = cells(i, grid)
    x = np.minimum(np.maximum(cx - 1, 0), nx - 1)          # a ghost index: the nearest interior cell's
    y = np.minimum(np.maximum(cy - 1, 0), ny - 1)
    z = np.minimum(np.maximum(cz - 1, 0), nz - 1)
    tile = ((z // TILE_EDGE) * nty + (y // TILE_EDGE)) * ntx + (x // TILE_EDGE)
    if order == "tile_only":
        return tile
    return tile * TILE_CELLS + ((z % TILE_EDGE) * 16 + (y % TILE_EDGE) * 4 + (x % TILE_EDGE))


def starts(i_live, grid, order):
    """int64[n_keys + 1]: where every key's particles begin in an array sorted in `order`, and the particle count at the
    end -- partition[] for "voxel", tpart[] for "tile".  For "tile_only" every tile's particles are counted at the
    tile's FIRST key, 64 tile (the kernels count them there, particles.hip: coarse_count_kernel): entry 64 t is where tile t
    begins, the entries 64 t + 1 .. 64 t + 63 where tile t + 1 does."""
    k = keys(i_live, grid, order)
    if order == "tile_only":
        k = k * TILE_CELLS
    n = n_keys(grid, order)
    return np.concatenate([[0], np.cumsum(np.bincount(k, minlength=n))]).astype(np.int64)


def fullest_tile(i_live, grid):
    """particles of the fullest tile (the word tile_max_kernel publishes after a tile sort)"""
    if len(i_live) == 0:
        return 0
    return int(np.bincount(keys(i_live, grid, "tile_only"), minlength=ntiles_of(grid)).max())


def words(p):
    """uint32[n, 8]: the eight 32-bit words of every particle record (without tags), as bit patterns"""
    return np.stack([p[n].view(np.uint32) for n in WORDS], axis=1)


def _records(p):
    """particle records without tags, in one canonical order (bit patterns, every field a sort key)"""
    a = words(p)
    return a[np.lexsort(a.T[::-1])]


def _all_words(p):
    """uint32[n, 12]: the record's words and those of the two tags"""
    t = np.stack([p["tag"], p["tag2"]], axis=1).astype(np.int64).view(np.uint32).reshape(len(p), 4)
    return np.concatenate([words(p), t], axis=1)


def same_per_key(got, k_got, ref, k_ref, what="sort"):
    """For every key, the particles of `got` with that key are those of `ref` with that key, bit for bit, as multisets
    (the order inside a key is the atomics' order and is free).  k_got / k_ref: the key of every particle of got / ref.
    Raises with the first offending index (of got in key-and-record order) and its key."""
    if len(got) != len(ref):
        raise AssertionError(f"{what}: {len(got)} particles, {len(ref)} expected")
    if len(got) == 0:
        return
    tagged = bool(np.any(ref["tag"] != 0) or np.any(ref["tag2"] != 0) or np.any(got["tag"] != 0) or np.any(got["tag2"] != 0))
    if tagged and len(np.unique(ref["tag"])) == len(ref):
        # by tag: the same tags, and under every tag the same record with the same key
        og, orf = np.argsort(got["tag"], kind="stable"), np.argsort(ref["tag"], kind="stable")
        if not np.array_equal(got["tag"][og], ref["tag"][orf]):
            bad = int(np.flatnonzero(got["tag"][og] != ref["tag"][orf])[0])
            raise AssertionError(f"{what}: tags differ: the array holds tag {got['tag'][og][bad]} (index {og[bad]}, key {k_got[og[bad]]}) "
                                 f"where tag {ref['tag'][orf][bad]} is expected")
        wg, wr = _all_words(got)[og], _all_words(ref)[orf]
        diff = np.any(wg != wr, axis=1) | (np.asarray(k_got)[og] != np.asarray(k_ref)[orf])
        if diff.any():
            bad = int(np.flatnonzero(diff)[0])
            raise AssertionError(f"{what}: the particle of tag {got['tag'][og][bad]} at index {og[bad]} (key {k_got[og[bad]]}) differs: words "
                                 f"{wg[bad].tolist()} against {wr[bad].tolist()} (key {k_ref[orf[bad]]})")
        return
    wg, wr = _all_words(got), _all_words(ref)
    og = np.lexsort(tuple(wg.T[::-1]) + (np.asarray(k_got),))          # by key, then by record
    orf = np.lexsort(tuple(wr.T[::-1]) + (np.asarray(k_ref),))
    diff = np.any(wg[og] != wr[orf], axis=1) | (np.asarray(k_got)[og] != np.asarray(k_ref)[orf])
    if diff.any():
        bad = int(np.flatnonzero(diff)[0])
        raise AssertionError(f"{what}: the particles of key {k_got[og[bad]]} differ from the input's: index {og[bad]} holds "
                             f"{wg[og[bad]].tolist()}, expected (key {k_ref[orf[bad]]}) {wr[orf[bad]].tolist()}")


def _same_ints(got, ref, name):
    got, ref = np.asarray(got).astype(np.int64), np.asarray(ref).astype(np.int64)
    if got.shape != ref.shape:
        raise AssertionError(f"{name}: {got.shape[0]} entries, {ref.shape[0]} expected")
    if not np.array_equal(got, ref):
        bad = int(np.flatnonzero(got != ref)[0])
        raise AssertionError(f"{name}[{bad}] is {got[bad]}, expected {ref[bad]}")


def check(got, inputs_live, grid, order, partition=None, tpart=None):
    """`got` is `inputs_live` sorted in `order`.  Raises AssertionError with the first offending index and key.
      1. the keys of got are non-decreasing in `order`;
      2. len(got) == len(inputs_live), and no dead slot (i < 0) is left;
      3. the same particles bit for bit: by tag for a tagged species, as multisets of the eight 32-bit words for a tag-less
         one; and key by key as multisets (same_per_key);
      4. partition (when given): starts(inputs_live, "voxel"), all nv + 1 entries;
      5. tpart (when given): order "tile": starts(.., "tile"), all 64 ntiles + 1 entries.  Order "tile_only":
         starts(.., "tile_only"), all entries too: tpart[64 t] is where tile t begins and tpart[-1] the particle count,
         which is all the push (push.hip: first / last of a tile's workgroup), the moments and the distributions by tile
         and tile_max_kernel read; the entries in between hold what the scan of counts that all sit at 64 t leaves
         there, the start of tile t + 1 -- so that tpart[] is a partition of the array by tile at every entry
         (k_check_tile_partition relies on non-decreasing entries)."""
    assert order in ORDERS, order
    i_got = got["i"].astype(np.int64)
    if np.any(i_got < 0):
        bad = int(np.flatnonzero(i_got < 0)[0])
        raise AssertionError(f"sort ({order}): a dead slot (i = {i_got[bad]}) is left at index {bad}")
    if np.any(i_got >= nv_of(grid)):
        bad = int(np.flatnonzero(i_got >= nv_of(grid))[0])
        raise AssertionError(f"sort ({order}): index {bad} holds voxel {i_got[bad]}, the grid has {nv_of(grid)}")
    k = keys(i_got, grid, order)
    if np.any(np.diff(k) < 0):
        bad = int(np.flatnonzero(np.diff(k) < 0)[0]) + 1
        raise AssertionError(f"sort ({order}): key {k[bad]} at index {bad} follows key {k[bad - 1]}")
    if len(got) != len(inputs_live):
        raise AssertionError(f"sort ({order}): {len(got)} particles, {len(inputs_live)} went in")
    i_in = inputs_live["i"].astype(np.int64)
    assert np.all(i_in >= 0), "inputs_live holds dead slots"
    same_per_key(got, k, inputs_live, keys(i_in, grid, order), what=f"sort ({order})")
    if partition is not None:
        _same_ints(partition, starts(i_in, grid, "voxel"), "partition")
    if tpart is not None:
        assert order != "voxel", "tpart[] belongs to the tile orders"
        _same_ints(tpart, starts(i_in, grid, order), "tpart")
        if int(np.asarray(tpart)[-1]) != len(inputs_live):
            raise AssertionError(f"tpart[-1] is {np.asarray(tpart)[-1]}, the species has {len(inputs_live)} particles")


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def interior(grid):
    """the interior voxels, in voxel order"""
    nx, ny, nz = grid
    z, y, x = np.meshgrid(np.arange(1, nz + 1), np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    return (x + (nx + 2) * (y + (ny + 2) * z)).ravel().astype(np.int64)


def ghosts_of(grid):
    """the voxels of the ghost layers, in voxel order (voxel 0 the first, voxel nv - 1 the last)"""
    g = np.ones(nv_of(grid), bool)
    g[interior(grid)] = False
    return np.flatnonzero(g).astype(np.int64)


def arrangement(name, rng, grid, n, order="voxel"):
    """int32[n]: the voxel indices of n particles.  `order`: the target order of "sorted", "reversed" and "nearly".
      random          uniform over the interior
      sorted          already in the target order
      reversed        the target order, backwards
      one_cell        every particle in one voxel
      round_robin_20  20 voxels cycling, of 20 different tiles where the grid has as many (of all its tiles otherwise, then
                      further cells of them): every wavefront holds 20 distinct voxels three or four times each
      nearly          sorted, then 5 % of the positions permuted among themselves
      ghosts          random, with 2 % of the particles (two at least) moved to ghost voxels, voxel 0 and voxel nv - 1 among
                      them; every index satisfies 0 <= i < nv.  Only ever sorted, never pushed."""
    assert name in ARRANGEMENTS, name
    inside = interior(grid)
    i = rng.choice(inside, n)
    if name in ("sorted", "reversed", "nearly"):
        i = i[np.argsort(keys(i, grid, order), kind="stable")]
        if name == "reversed":
            i = i[::-1].copy()
        if name == "nearly" and n >= 2:
            pos = rng.choice(n, max(2, n // 20), replace=False)
            i[pos] = i[rng.permutation(pos)]
    elif name == "one_cell":
        i = np.full(n, inside[len(inside) // 2])
    elif name == "round_robin_20":
        by_tile = inside[np.argsort(keys(inside, grid, "tile"), kind="stable")]
        t = keys(by_tile, grid, "tile_only")
        first = np.flatnonzero(np.concatenate([[True], np.diff(t) > 0]))      # the first cell of every tile
        pick = [by_tile[first[j % len(first)] + j // len(first)] for j in range(20)]
        assert len(set(pick)) == 20 or len(inside) < 20
        i = np.array(pick, np.int64)[np.arange(n) % 20]
    elif name == "ghosts" and n > 0:
        gh = ghosts_of(grid)
        m = min(n, max(2, n // 50))
        pos = rng.choice(n, m, replace=False)
        v = rng.choice(gh, m)
        v[0] = 0
        if m > 1:
            v[1] = nv_of(grid) - 1
        i[pos] = v
    return i.astype(np.int32)


def particles(rng, i, tagged):
    """particle_t[len(i)] in voxels i whose seven float words are seeded random bit patterns of FINITE floats (a mixed-up
    word cannot go unseen); tags 1 .. n in a shuffled order, or none"""
    n = len(i)
    p = np.zeros(n, particle_dtype())
    p["i"] = i
    for name in WORDS[1:]:
        w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        w[(w & np.uint32(0x7F800000)) == np.uint32(0x7F800000)] &= np.uint32(0xBFFFFFFF)      # (inf / nan: clear an exponent bit)
        p[name] = w.view(np.float32)
    if tagged:
        p["tag"] = rng.permutation(n) + 1
        p["tag2"] = rng.integers(0, 1 << 40, n)
    return p


# ---- the cases tests/test_sort_ref.py and tests/test_gpu_sort.py share -----------------------------------------------------

GRIDS = {                                                   # grid: why it is there (the parameter ids carry it)
    (1, 1, 1): "sy=3, one partial tile",
    (3, 5, 2): "thinner than a tile on two axes",
    (4, 4, 4): "exactly one tile",
    (5, 4, 4): "one cell past a tile",
    (7, 9, 6): "partial tiles on every axis",
    (62, 3, 2): "sy=64",
    (63, 2, 3): "sy=65",
    (16, 8, 12): "the cell table overflows",
    (40, 40, 40): "the tile table of the coarse scatter overflows",
    (66, 64, 64): "the scan's carry loop in both orders",
}
MAIN_GRIDS = ((7, 9, 6), (16, 8, 12))                       # every arrangement runs on these
CHUNK = 2048                                                # particles of a sort workgroup (particles.hip: WG_CHUNK, COARSE_CHUNK)
WG_TABLE, COARSE_TABLE, SCAN_BLOCK, SCAN_BLOCKS_PER_ROUND = 512, 128, 1024, 256
# on (7,9,6): 14341, 16384, 18435 and 81937 are 7, 8, 9 and 40 chunks of 2048, plus a remainder for all but 16384 -- the edges of
# the scatter's grid (rounded up to a multiple of 8, whole workgroups return early) and of xcd_block
NP_EDGES = (0, 1, 63, 64, 65, 257, 2047, 2048, 2049, 14341, 16384, 16385, 18435, 81937)
N_DEFAULT = 5 * CHUNK + 777                                 # the other cases: a few chunks and a remainder
N_LARGE_GRID = 2 * CHUNK + 777                              # (66,64,64): a few thousand particles are enough


def default_n(grid):
    return N_LARGE_GRID if grid == (66, 64, 64) else N_DEFAULT


def grid_id(grid):
    return "%dx%dx%d %s" % (grid + (GRIDS[grid],))


def case_voxels(grid, name, n, order="voxel"):
    """the seeded voxel indices of one case (the same for the tagged and the tag-less species, on the CPU and the GPU)"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(repr((grid, name, int(n), order)).encode()))
    return arrangement(name, rng, grid, n, order)


def case_particles(grid, name, n, order, tagged):
    import zlib
    i = case_voxels(grid, name, n, order)
    rng = np.random.default_rng(zlib.crc32(repr(("words", grid, name, int(n), order, bool(tagged))).encode()))
    return particles(rng, i, tagged)
