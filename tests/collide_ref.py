"""The numpy reference of vpic_hip_collide, written from include/vpic_hip.h alone: mix32, the keys and ranks of a cell's
particles, the pairs, the arithmetic of one pair in np.float32 operation by operation (the parentheses of the header),
and the order of the pairs that share a particle.  tests/test_collide_ref.py pins it on the model (permutations, who
pairs with whom, |g + D| = |g|, momentum); tests/test_gpu_collide.py compares the device with it word for word."""
import numpy as np

F = np.float32
TWO64 = F(18446744073709551616.0)
MAX_CELL = 1024                                                 # VPIC_HIP_COLLIDE_MAX_CELL


def mix32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xffffffff)
    m = np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def _u32(x):
    return int(x) & 0xffffffff


def cell_c0(seed, call, species, rank, v):
    """c0_s = mix32((seed ^ mix32(call * 0x9e3779b9 + s)) + mix32(rank * 0x85ebca6b + v))"""
    h1 = int(mix32(_u32(call * 0x9e3779b9 + species)))
    h2 = int(mix32(_u32(rank * 0x85ebca6b + v)))
    return int(mix32(_u32((_u32(seed) ^ h1) + h2)))


def keys(c0, n):
    return mix32((np.arange(n, dtype=np.uint64) + np.uint64(c0)) & np.uint64(0xffffffff))


def perm(c0, n):
    """perm[r] = the k whose key is the r-th smallest (mix32 is a bijection and n < 2^32: no ties)"""
    k = keys(c0, n)
    assert len(np.unique(k)) == n
    return np.argsort(k, kind="stable")


def pairs_same(p):
    """[(k_first, k_second, pair number, half)] of one species' cell, in the order they are applied"""
    n = len(p)
    if n < 2:
        return []
    if n % 2 == 0:
        return [(int(p[2 * j]), int(p[2 * j + 1]), j, False) for j in range(n // 2)]
    p0, p1, p2 = int(p[0]), int(p[1]), int(p[2])
    out = [(p0, p1, 0, True), (p1, p2, 1, True), (p2, p0, 2, True)]
    return out + [(int(p[3 + 2 * m]), int(p[4 + 2 * m]), 3 + m, False) for m in range((n - 3) // 2)]


def pairs_two(perm_a, perm_b):
    """(swap, [(k_L, k_S, pair number)]) -- swap: L is species b; ascending j is the order of application"""
    n_a, n_b = len(perm_a), len(perm_b)
    swap = n_b > n_a
    pl, ps = (perm_b, perm_a) if swap else (perm_a, perm_b)
    if len(ps) == 0:
        return swap, []
    return swap, [(int(pl[j]), int(ps[j % len(ps)]), j) for j in range(len(pl))]


def scatter(uf, us, wf, ws, ff, fs, cvar, n, dt, den, half, draw):
    """One pair.  uf, us: float32[3] of the first and second particle; wf, ws their weights; ff, fs = m_ab / m of each;
    den = (V * m_ab) * m_ab; draw = (N, cos phi, sin phi, U).  Returns (uf', us', status, D) with status "skipped" or a
    pair of booleans (first updated, second updated); D is the change of g (None when skipped)."""
    uf, us = np.asarray(uf, F), np.asarray(us, F)
    dn, dc, ds, du = (F(x) for x in draw)
    with np.errstate(all="ignore"):
        gx, gy, gz = uf[0] - us[0], uf[1] - us[1], uf[2] - us[2]
        gq = gx * gx + gy * gy
        g2 = gq + gz * gz
        gm, gp = np.sqrt(g2), np.sqrt(gq)
        if gm == 0:
            return uf.copy(), us.copy(), "skipped", None
        s2 = (((F(cvar) * max(F(wf), F(ws))) * F(n)) * F(dt)) / (F(den) * ((gm * gm) * gm))
        if half:
            s2 = F(0.5) * s2
        dl = dn * np.sqrt(s2)
        t = dl * dl
        if t < TWO64:
            sin_t, omc = (F(2) * dl) / (F(1) + t), (F(2) * t) / (F(1) + t)
        else:
            sin_t, omc = F(0), F(2)
        sc, ss = sin_t * dc, sin_t * ds
        if gp != 0:
            ax, ay = gx / gp, gy / gp
            Dx = ((ax * gz) * sc - (ay * gm) * ss) - gx * omc
            Dy = ((ay * gz) * sc + (ax * gm) * ss) - gy * omc
            Dz = (-(gp * sc)) - gz * omc
        else:
            Dx, Dy, Dz = gm * sc, gm * ss, -(gz * omc)
        wf, ws = F(wf), F(ws)
        do_f = bool(ws >= wf or du * wf < ws)
        do_s = bool(wf >= ws or du * ws < wf)
        D = np.array([Dx, Dy, Dz], F)
        nf, ns = uf.copy(), us.copy()
        if do_f:
            nf = np.array([uf[0] + F(ff) * Dx, uf[1] + F(ff) * Dy, uf[2] + F(ff) * Dz], F)
        if do_s:
            ns = np.array([us[0] - F(fs) * Dx, us[1] - F(fs) * Dy, us[2] - F(fs) * Dz], F)
    assert all(isinstance(x, np.float32) for x in (gm, s2, dl, t, sin_t, omc, Dx, Dy, Dz)), "an operation left float32"
    return nf, ns, (do_f, do_s), D


def cell_ranges(voxels):
    """{voxel: (lo, n)} of an array whose particles lie cell by cell (any order of the cells)"""
    voxels = np.asarray(voxels)
    out = {}
    if len(voxels) == 0:
        return out
    cut = np.flatnonzero(np.diff(voxels) != 0) + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut, [len(voxels)]])
    for a, b in zip(lo, hi):
        v = int(voxels[a])
        assert v not in out, "the particles of voxel %d are not contiguous" % v
        out[v] = (int(a), int(b - a))
    return out


def collide(pa, pb, *, m_a, m_b=None, wq_a, wq_b=None, cvar, dt, seed, call, sp_a=0, sp_b=None, volume, draws, rank=0, log=None):
    """vpic_hip_collide on host copies.  pa, pb: particle_t arrays lying cell by cell (pb None: within one species);
    volume: (dx * dy) * dz as a float32; draws: float32[n, 4] by the index of the pair's first particle.  Returns
    (ua float32[n_a, 3], ub or None, stats) with stats = dict(cells, pairs, skipped, one_sided, fullest_cell).  log: a list
    that receives one record per pair (species of the first particle, index first, index second, status, g, D)."""
    same = pb is None
    m_a, wq_a = F(m_a), F(wq_a)
    m_b, wq_b = (m_a, wq_a) if same else (F(m_b), F(wq_b))
    sp_b = sp_a if same else sp_b
    m_ab = (m_a * m_b) / (m_a + m_b)
    den = (F(volume) * m_ab) * m_ab
    f_a, f_b = m_ab / m_a, m_ab / m_b
    ua = np.stack([pa["ux"], pa["uy"], pa["uz"]], 1).astype(F)
    wa = np.abs(pa["q"].astype(F)) * wq_a
    ra = cell_ranges(pa["i"])
    stats = dict(cells=0, pairs=0, skipped=0, one_sided=0, fullest_cell=max([n for _, n in ra.values()] + [0]))
    draws = np.asarray(draws, F).reshape(-1, 4)

    def apply(UF, kf, US, ks, WF, WS, ff, fs, n, half, first_index, tag):
        nf, ns, status, D = scatter(UF[kf], US[ks], WF[kf], WS[ks], ff, fs, cvar, n, dt, den, half, draws[first_index])
        if log is not None:
            log.append((tag, kf, ks, status, UF[kf] - US[ks], D))
        UF[kf], US[ks] = nf, ns
        if status == "skipped":
            stats["skipped"] += 1
        else:
            stats["pairs"] += 1
            stats["one_sided"] += 0 if all(status) else 1

    if same:
        for v, (lo, n) in sorted(ra.items()):
            prs = pairs_same(perm(cell_c0(seed, call, sp_a, rank, v), n))
            stats["cells"] += 1 if prs else 0
            for kf, ks, _, half in prs:
                apply(ua, lo + kf, ua, lo + ks, wa, wa, f_a, f_a, n, half, lo + kf, sp_a)
        return ua, None, stats
    ub = np.stack([pb["ux"], pb["uy"], pb["uz"]], 1).astype(F)
    wb = np.abs(pb["q"].astype(F)) * wq_b
    rb = cell_ranges(pb["i"])
    stats["fullest_cell"] = max([stats["fullest_cell"]] + [n for _, n in rb.values()])
    for v in sorted(set(ra) & set(rb)):
        (lo_a, n_a), (lo_b, n_b) = ra[v], rb[v]
        swap, prs = pairs_two(perm(cell_c0(seed, call, sp_a, rank, v), n_a), perm(cell_c0(seed, call, sp_b, rank, v), n_b))
        stats["cells"] += 1 if prs else 0
        n = min(n_a, n_b)
        for kl, ks, _ in prs:
            if swap:
                apply(ub, lo_b + kl, ua, lo_a + ks, wb, wa, f_b, f_a, n, False, lo_b + kl, sp_b)
            else:
                apply(ua, lo_a + kl, ub, lo_b + ks, wa, wb, f_a, f_b, n, False, lo_a + kl, sp_a)
    return ua, ub, stats
