"""Numpy restatement of THE RULE of vpic_hip_species_load_profile (include/vpic_hip.h): Philox-4x32-10, the map from a
particle's eight words to its numbers, the double arithmetic of the momentum, and the order and partition[] of a call.
Written from the text of the header alone; old-vpic_amd/csrc/load_rule.h is held == to it by tests/test_load_rule.py and
the device by tests/test_gpu_load.py."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
UNIT_OPEN_MAX = np.float32(1.0) - np.float32(2.0 ** -24)
LOAD_APPEND, LOAD_FLIP, LOAD_TAGS = 1, 2, 4

particle_t = np.dtype([("dx", "f4"), ("dy", "f4"), ("dz", "f4"), ("i", "i4"), ("ux", "f4"), ("uy", "f4"), ("uz", "f4"), ("q", "f4"),
                       ("tag", "i8"), ("tag2", "i8")], align=True)


def philox(counter, key):
    """counter: uint32[..., 4], key: (k0, k1), scalars or arrays shaped as counter[..., 0] -> uint32[..., 4], ten rounds"""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = np.asarray(key[0]).astype(np.uint64) & MASK, np.asarray(key[1]).astype(np.uint64) & MASK
    for rnd in range(10):
        if rnd > 0:
            k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # (32 x 32 bits: no overflow of 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(cell, j, seed, stream):
    """the eight words of particle j of global cell `cell` (uint64): uint32[n, 8]"""
    cell = np.asarray(cell, np.uint64)
    j = np.asarray(j, np.uint64)
    out = []
    for b in range(2):
        ctr = np.stack([cell & MASK, cell >> np.uint64(32), j & MASK, np.full(cell.shape, b, np.uint64)], axis=-1)
        out.append(philox(ctr, (seed, stream)))
    return np.concatenate(out, axis=-1)


def unit_open(r):
    x = ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(x, UNIT_OPEN_MAX)


def numbers(r):
    """float32[n, 7] = (x0, x1, x2, n0, n1, n2, U) of the words r[n, 8]; the normals with numpy's log / cos / sin (they are
    specified statistically: the device uses its own)"""
    r = np.asarray(r, np.uint32)
    u = unit_open(r)
    two_pi = np.float32(6.2831853)
    r1 = np.sqrt(np.float32(-2) * np.log(u[:, 3]))
    r2 = np.sqrt(np.float32(-2) * np.log(u[:, 5]))
    return np.stack([u[:, 0], u[:, 1], u[:, 2], r1 * np.cos(two_pi * u[:, 4]), r1 * np.sin(two_pi * u[:, 4]),
                     r2 * np.cos(two_pi * u[:, 6]), u[:, 7]], axis=1).astype(np.float32)


def offsets(x):
    return np.float32(2) * np.asarray(x, np.float32) - np.float32(1)


def momentum(uth, ud, n, U, flip, parts=False):
    """uth, ud, n: float32[m, 3], U: float32[m]; flip: bool or bool[m] -> float32[m, 3].  IEEE double, one rounding per operation.
    parts=True: (u, flipped, w after the flip, gw, gd, wD after the flip), u and the rest in double before the last rounding."""
    w = [np.asarray(uth, np.float32)[:, k].astype(np.float64) * np.asarray(n, np.float32)[:, k].astype(np.float64) for k in range(3)]
    gw = np.sqrt(1 + ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))
    D = [np.asarray(ud, np.float32)[:, k].astype(np.float64) for k in range(3)]
    D2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
    rest = D2 == 0
    safe = np.where(rest, 1.0, D2)
    gd = np.sqrt(1 + D2)
    wD = (w[0] * D[0] + w[1] * D[1]) + w[2] * D[2]
    flipped = np.broadcast_to(np.asarray(flip, bool), wD.shape) & ~rest & ((-wD) / (gd * gw) > np.asarray(U, np.float32).astype(np.float64))
    t = (2 * wD) / safe
    w = [np.where(flipped, w[k] - t * D[k], w[k]) for k in range(3)]
    wD = np.where(flipped, -wD, wD)
    f = ((gd - 1) * wD) / safe + gw
    u = [np.where(rest, w[k], w[k] + f * D[k]) for k in range(3)]
    if parts:
        return np.stack(u, axis=1), flipped, np.stack(w, axis=1), gw, gd, wD
    return np.stack(u, axis=1).astype(np.float32)


def table(t, dims):
    """a table (scalar or [tz, ty, tx], extents 1 or the grid's) over the cells of a grid dims = (nx, ny, nz): [nz, ny, nx]"""
    nx, ny, nz = dims
    return np.broadcast_to(np.asarray(t), (nz, ny, nx))


def load(dims, count, q, ud=None, uth=None, *, seed=0, stream=0, global_dims=None, offset=(0, 0, 0), flip=False, tag0=None,
         draws=None):
    """The particles of one call in its order and its partition[nv + 1]: (particle_t[n], int32[nv + 1], global cell uint64[n],
    j int64[n]).  Tables as Engine.load_profile takes them.  draws: float32[n, 7] of the parity mode, or None: the
    generator, normals by numpy."""
    nx, ny, nz = dims
    gdim = dims if global_dims is None else global_dims
    cnt = table(count, dims).astype(np.int64)
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")      # ascending voxel = z, y, x
    per_cell = cnt.ravel()
    n = int(per_cell.sum())
    start = np.concatenate([[0], np.cumsum(per_cell)])
    which = np.repeat(np.arange(per_cell.size), per_cell)                                     # the cell of every place m
    j = np.arange(n) - start[which]
    lx, ly, lz = cx.ravel()[which], cy.ravel()[which], cz.ravel()[which]
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    voxel = (lx + 1) + sy * (ly + 1) + sz * (lz + 1)
    cell = (np.uint64(offset[0]) + lx.astype(np.uint64)) + np.uint64(gdim[0]) * (
        (np.uint64(offset[1]) + ly.astype(np.uint64)) + np.uint64(gdim[1]) * (np.uint64(offset[2]) + lz.astype(np.uint64)))
    d = numbers(words(cell, j, seed, stream)) if draws is None else np.asarray(draws, np.float32).reshape(-1, 7)[:n]
    def per_particle(t):
        return np.zeros(n, np.float32) if t is None else table(t, dims).astype(np.float32).ravel()[which]
    uth3 = np.stack([per_particle(None if uth is None else uth[k]) for k in range(3)], axis=1)
    ud3 = np.stack([per_particle(None if ud is None else ud[k]) for k in range(3)], axis=1)
    u = momentum(uth3, ud3, d[:, 3:6], d[:, 6], flip)
    p = np.zeros(n, particle_t)
    p["dx"], p["dy"], p["dz"] = offsets(d[:, 0]), offsets(d[:, 1]), offsets(d[:, 2])
    p["i"] = voxel
    p["ux"], p["uy"], p["uz"] = u[:, 0], u[:, 1], u[:, 2]
    p["q"] = per_particle(q)
    if tag0 is not None:
        p["tag"] = tag0 + np.arange(n)
    nv = (nx + 2) * (ny + 2) * (nz + 2)
    per_voxel = np.zeros(nv + 1, np.int64)
    per_voxel[((cx + 1) + sy * (cy + 1) + sz * (cz + 1)).ravel()] = per_cell
    partition = np.concatenate([[0], np.cumsum(per_voxel)[:-1]]).astype(np.int32)
    return p, partition, cell, j
