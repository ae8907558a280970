"""The numpy reference of vpic_hip_collide_relativistic, written from include/vpic_hip.h alone.  Everything the header
declares shared with vpic_hip_collide -- mix32, the keys and ranks, the pairs, the order of pairs that share a particle,
the weight rule, the draws table -- is imported from tests/collide_ref.py; only the pair is restated here, in np.float64
operation by operation (the parentheses of the header), the two new momenta rounded to float32 once each at the end.
tests/test_collide_rel_ref.py pins it on the model; tests/test_gpu_collide_rel.py compares the device with it word for word."""
import numpy as np

from collide_ref import MAX_CELL, cell_c0, cell_ranges, mix32, pairs_same, pairs_two, perm  # noqa: F401

F = np.float32
D = np.float64
TWO64 = D(18446744073709551616.0)


def _in(x):
    """an input promoted to double: through float32 as the device reads it -- a np.float64 is taken as it is (the covariance
    test of tests/test_collide_rel_ref.py hands in a second frame's momenta and dt unrounded)"""
    return x if isinstance(x, np.float64) else D(F(x))


def scatter(uf, us, wf, ws, m_f, m_s, cvar, n, dt, volume, half, draw, detail=None):
    """One pair.  uf, us: float32[3] of the first and second particle; wf, ws their weights; m_f, m_s their masses; volume =
    (dx * dy) * dz as a float32; draw = (N, cos phi, sin phi, U).  Returns (uf', us', status) with status "skipped" or a pair
    of booleans (first updated, second updated).  detail: a dict that receives the pair's double intermediates (v, gC, p*, q,
    pm, s2, the unrounded new momenta nf, ns, ...) for the tests of the model."""
    uf, us = (np.asarray(x, D if np.asarray(x).dtype == D else F) for x in (uf, us))
    if uf[0] == us[0] and uf[1] == us[1] and uf[2] == us[2]:
        return uf.copy(), us.copy(), "skipped"
    ufx, ufy, ufz = (D(x) for x in uf)
    usx, usy, usz = (D(x) for x in us)
    wf, ws = F(wf), F(ws)
    mf, ms = D(F(m_f)), D(F(m_s))
    cvar, dt, V, N = D(F(cvar)), _in(dt), D(F(volume)), D(F(n))
    dn, dc, ds = (D(F(x)) for x in draw[:3])
    du = F(draw[3])
    one, two = D(1), D(2)
    with np.errstate(all="ignore"):
        gf = np.sqrt(one + ((ufx * ufx + ufy * ufy) + ufz * ufz))
        gs = np.sqrt(one + ((usx * usx + usy * usy) + usz * usz))
        ef, es = mf * gf, ms * gs
        E = ef + es
        rE = one / E
        vx, vy, vz = (mf * ufx + ms * usx) * rE, (mf * ufy + ms * usy) * rE, (mf * ufz + ms * usz) * rE
        gC = one / np.sqrt(one - ((vx * vx + vy * vy) + vz * vz))
        kC = (gC * gC) / (gC + one)
        vuf = (vx * ufx + vy * ufy) + vz * ufz
        vus = (vx * usx + vy * usy) + vz * usz
        cf = kC * vuf - gC * gf
        px, py, pz = mf * (ufx + cf * vx), mf * (ufy + cf * vy), mf * (ufz + cf * vz)
        esf, ess = mf * (gC * (gf - vuf)), ms * (gC * (gs - vus))
        pq = px * px + py * py
        p2 = pq + pz * pz
        pm, gp = np.sqrt(p2), np.sqrt(pq)
        if pm == 0:
            return uf.copy(), us.copy(), "skipped"
        r = (esf * ess) / (pm * pm) + one
        s2 = ((((cvar * D(max(wf, ws))) * N) * dt) * (((gC * pm) * rE) * (r * r))) / (V * (ef * es))
        if half:
            s2 = D(0.5) * s2
        dl = dn * np.sqrt(s2)
        t = dl * dl
        if t < TWO64:
            sin_t, omc = (two * dl) / (one + t), (two * t) / (one + t)
        else:
            sin_t, omc = D(0), two
        sc, ss = sin_t * dc, sin_t * ds
        if gp != 0:
            ax, ay = px / gp, py / gp
            Dx = ((ax * pz) * sc - (ay * pm) * ss) - px * omc
            Dy = ((ay * pz) * sc + (ax * pm) * ss) - py * omc
            Dz = (-(gp * sc)) - pz * omc
        else:
            Dx, Dy, Dz = pm * sc, pm * ss, -(pz * omc)
        qx, qy, qz = px + Dx, py + Dy, pz + Dz
        kvq = kC * ((vx * qx + vy * qy) + vz * qz)
        a_f = kvq + esf * gC
        a_s = ess * gC - kvq
        rmf, rms = one / mf, one / ms
        nfd = np.array([(qx + vx * a_f) * rmf, (qy + vy * a_f) * rmf, (qz + vz * a_f) * rmf], D)
        nsd = np.array([(vx * a_s - qx) * rms, (vy * a_s - qy) * rms, (vz * a_s - qz) * rms], D)
        do_f = bool(ws >= wf or du * wf < ws)
        do_s = bool(wf >= ws or du * ws < wf)
        nf = nfd.astype(F) if do_f else uf.copy()
        ns = nsd.astype(F) if do_s else us.copy()
    assert all(isinstance(x, np.float64) for x in (gf, E, vx, gC, kC, px, pm, s2, dl, t, sin_t, omc, Dx, Dy, Dz, a_f, a_s)), "an operation left float64"
    if detail is not None:
        detail.update(v=np.array([vx, vy, vz]), gC=gC, kC=kC, p=np.array([px, py, pz]), q=np.array([qx, qy, qz]), pm=pm, gp=gp, s2=s2, t=t,
                      sin_t=sin_t, omc=omc, E=E, gf=gf, gs=gs, esf=esf, ess=ess, nf=nfd, ns=nsd)
    return nf, ns, (do_f, do_s)


def collide(pa, pb, *, m_a, m_b=None, wq_a, wq_b=None, cvar, dt, seed, call, sp_a=0, sp_b=None, volume, draws, rank=0, log=None):
    """vpic_hip_collide_relativistic on host copies: the signature, the returned values and the log of collide_ref.collide
    (the log's two last entries are u_f - u_s before the pair and None)."""
    same = pb is None
    m_a, wq_a = F(m_a), F(wq_a)
    m_b, wq_b = (m_a, wq_a) if same else (F(m_b), F(wq_b))
    sp_b = sp_a if same else sp_b
    ua = np.stack([pa["ux"], pa["uy"], pa["uz"]], 1).astype(F)
    wa = np.abs(pa["q"].astype(F)) * wq_a
    ra = cell_ranges(pa["i"])
    stats = dict(cells=0, pairs=0, skipped=0, one_sided=0, fullest_cell=max([n for _, n in ra.values()] + [0]))
    draws = np.asarray(draws, F).reshape(-1, 4)

    def apply(UF, kf, US, ks, WF, WS, mf, ms, n, half, first_index, tag):
        nf, ns, status = scatter(UF[kf], US[ks], WF[kf], WS[ks], mf, ms, cvar, n, dt, volume, half, draws[first_index])
        if log is not None:
            log.append((tag, kf, ks, status, UF[kf] - US[ks], None))
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
                apply(ua, lo + kf, ua, lo + ks, wa, wa, m_a, m_a, n, half, lo + kf, sp_a)
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
                apply(ub, lo_b + kl, ua, lo_a + ks, wb, wa, m_b, m_a, n, False, lo_b + kl, sp_b)
            else:
                apply(ua, lo_a + kl, ub, lo_b + ks, wa, wb, m_a, m_b, n, False, lo_a + kl, sp_a)
    return ua, ub, stats
