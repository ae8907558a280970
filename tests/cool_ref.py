"""THE RULE of vpic_hip_species_cool (include/vpic_hip.h) in numpy: what tests/test_gpu_cool.py holds the kernel to, word
for word.  float64 array arithmetic is IEEE and unfused, np.sqrt and / are correctly rounded, np.rint rounds to nearest
with ties to even as llrint does: every line below is one line of the header, in its order and with its parentheses.  The
fields at the particle are test_select_ref.fields_ref's (float32, one numpy operation per rounding)."""
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_select_ref import fields_ref  # noqa: E402

# u: float32[n, 3], the momenta after the call (a dead slot's, a left-alone particle's: as they were); addend: int64[n],
# what each particle adds (0 where it adds nothing); val: float64[n], |q| (gamma - gamma') (NaN where not computed);
# live, changed, refused, alone: bool[n]; isum: int; cell_isums: int64[nv]; stats: the four of vpic_hip_species_cool_stats
CoolRef = collections.namedtuple("CoolRef", "u addend val live changed refused alone isum cell_isums stats")
STAT_KEYS = ("seen", "changed", "refused", "left_alone")


def cool_fields(fields, u, q, sync, ic, quantum):
    """the rule behind the fields at the particle: fields float32[n, 6] (ex, ey, ez, cbx, cby, cbz), u float32[n, 3],
    q float32[n].  Returns (new u float32[n, 3], val float64[n], ok bool[n]: not left alone); a particle that is left
    alone keeps its u."""
    assert fields.dtype == np.float32 and u.dtype == np.float32 and q.dtype == np.float32
    sync, ic, quantum = np.float64(sync), np.float64(ic), np.float64(quantum)
    Ex, Ey, Ez, Bx, By, Bz = (fields[:, c].astype(np.float64) for c in range(6))
    ux, uy, uz = (u[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        new, _, ok = cool_double(Ex, Ey, Ez, Bx, By, Bz, ux, uy, uz, sync, ic)
        fx, fy, fz = (c.astype(np.float32) for c in new)
        wx, wy, wz = (c.astype(np.float64) for c in (fx, fy, fz))
        u2 = (ux * ux + uy * uy) + uz * uz
        g = np.sqrt(1.0 + u2)
        u2n = (wx * wx + wy * wy) + wz * wz
        g1 = np.sqrt(1.0 + u2n)
        val = np.abs(q).astype(np.float64) * ((u2 - u2n) / (g + g1))
    out = u.copy()
    out[ok, 0], out[ok, 1], out[ok, 2] = fx[ok], fy[ok], fz[ok]
    return out, np.where(ok, val, np.nan), ok


def cool_double(Ex, Ey, Ez, Bx, By, Bz, ux, uy, uz, sync, ic):
    """the double part of the rule up to nx, ny, nz (float64 arrays in, unrounded new momenta out): ((nx, ny, nz), D, ok)"""
    u2 = (ux * ux + uy * uy) + uz * uz
    g = np.sqrt(1.0 + u2)
    rg = 1.0 / g
    vx, vy, vz = ux * rg, uy * rg, uz * rg
    Lx = Ex + (vy * Bz - vz * By)
    Ly = Ey + (vz * Bx - vx * Bz)
    Lz = Ez + (vx * By - vy * Bx)
    vE = (vx * Ex + vy * Ey) + vz * Ez
    Ax = (Ly * Bz - Lz * By) + vE * Ex
    Ay = (Lz * Bx - Lx * Bz) + vE * Ey
    Az = (Lx * By - Ly * Bx) + vE * Ez
    L2 = (Lx * Lx + Ly * Ly) + Lz * Lz
    chi = L2 - vE * vE
    chi = np.where(chi < 0.0, 0.0, chi)                       # (a NaN stays a NaN)
    D = g * (sync * chi + ic)
    den = 1.0 + D
    nx, ny, nz = (ux + sync * Ax) / den, (uy + sync * Ay) / den, (uz + sync * Az) / den
    ok = np.isfinite(D) & np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz)
    return (nx, ny, nz), D, ok


def chi_raw(fields, u):
    """L2 - vE*vE before the clamp, float64[n] (the search for a clamped particle)"""
    Ex, Ey, Ez, Bx, By, Bz = (fields[:, c].astype(np.float64) for c in range(6))
    ux, uy, uz = (u[:, c].astype(np.float64) for c in range(3))
    u2 = (ux * ux + uy * uy) + uz * uz
    rg = 1.0 / np.sqrt(1.0 + u2)
    vx, vy, vz = ux * rg, uy * rg, uz * rg
    Lx = Ex + (vy * Bz - vz * By)
    Ly = Ey + (vz * Bx - vx * Bz)
    Lz = Ez + (vx * By - vy * Bx)
    vE = (vx * Ex + vy * Ey) + vz * Ez
    return ((Lx * Lx + Ly * Ly) + Lz * Lz) - vE * vE


def tally(val, ok, quantum):
    """(addend int64[n], refused bool[n]) of the particles that were not left alone"""
    with np.errstate(all="ignore"):
        t = val / np.float64(quantum)
        taken = ok & (np.abs(t) < 4294967296.0)               # (a NaN is refused)
    addend = np.zeros(len(val), np.int64)
    addend[taken] = np.rint(t[taken]).astype(np.int64)
    return addend, ok & ~taken


def cool_ref(p, fi, sync, ic, quantum):
    """CoolRef of the array p (particle_t[n], dead slots and any voxel allowed) under the interpolator fi[nv]"""
    nv = len(fi)
    n = len(p)
    live = (p["i"] >= 0) & (p["i"] < nv)
    u = np.stack([p["ux"], p["uy"], p["uz"]], axis=1).astype(np.float32)
    idx = np.flatnonzero(live)
    pl = p[idx]
    new, val_l, ok_l = cool_fields(fields_ref(pl, fi), u[idx], pl["q"].astype(np.float32), sync, ic, quantum)
    addend_l, refused_l = tally(val_l, ok_l, quantum)
    out = u.copy()
    out[idx] = new
    val = np.full(n, np.nan)
    val[idx] = val_l
    addend = np.zeros(n, np.int64)
    addend[idx] = addend_l
    changed = np.zeros(n, bool)
    changed[idx] = ok_l & np.any(new.view(np.uint32) != u[idx].view(np.uint32), axis=1)
    refused = np.zeros(n, bool)
    refused[idx] = refused_l
    alone = np.zeros(n, bool)
    alone[idx] = ~ok_l
    cells = np.zeros(nv, np.int64)
    np.add.at(cells, p["i"][idx], addend_l)
    stats = dict(zip(STAT_KEYS, (int(live.sum()), int(changed.sum()), int(refused.sum()), int(alone.sum()))))
    return CoolRef(out, addend, val, live, changed, refused, alone, int(addend.sum()), cells, stats)


def apply_ref(p, ref):
    """p with the reference's momenta"""
    q = p.copy()
    q["ux"], q["uy"], q["uz"] = ref.u[:, 0], ref.u[:, 1], ref.u[:, 2]
    return q


def kinetic(p):
    """sum |q| (gamma - 1) of the live particles (i >= 0), in double, gamma - 1 = u2 / (gamma + 1)"""
    p = p[p["i"] >= 0]
    ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    u2 = (ux * ux + uy * uy) + uz * uz
    return float(np.sum(np.abs(p["q"]).astype(np.float64) * (u2 / (np.sqrt(1.0 + u2) + 1.0))))
