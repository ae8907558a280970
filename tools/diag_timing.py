"""What tools/spectrum_time.py, distribution_time.py, select_time.py and moments_time.py share: the species they time,
events around a call, the alternating loop, and the report lines.

The species is that of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread 0.02 c) in tile order,
with an EMPTY species beside it in the same engine: a diagnostic called on the empty one clears, copies and waits for
exactly the same bytes and launches nothing, so "events around the call minus events around the same call on the empty
species" is the kernels' share of a call."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
VTH = 0.02


def parser(reps):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=32)
    return ap


def species(args, before_sort=None):
    """(package, engine, species, empty species, torch stream of the engine) -- the species loaded and sorted by tile;
    before_sort(engine, species): what a tool does to the loaded particles before the sort (tags)"""
    import torch
    V = importlib.import_module("old-vpic_amd")
    n, ppc = args.cells, args.ppc
    e = V.Engine(V.make_grid(n, n, n, float(n), float(n), float(n), np.float32(0.95 / np.sqrt(3.0))))
    e.set_vacuum()
    e.set_sort_order("engine")
    np_ = n ** 3 * ppc
    sp = e.new_species(-1.0, np_ + 4096, np_ // 8)
    empty = e.new_species(-1.0, 4096, 64)
    e.load_maxwellian(sp, ppc, 1, -1.0 / ppc, (0.2, 0.0, 0.0), VTH)
    if before_sort:
        before_sort(e, sp)
    e.load_interpolator()
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    return V, e, sp, empty, torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", 0))


def set_field(V, e, cells, seed=4):
    """A magnetic and an electric field for the coordinates in the frame of the local field (the species above is loaded
    in vacuum, where every one of them is NaN): a guide field of 0.5 along x plus seeded values in every voxel and
    component of the interpolator, set as loaded.  What a pass costs does not depend on the values."""
    nv = (cells + 2) ** 3
    rng = np.random.default_rng(seed)
    fi = np.zeros(nv, V.layout.interpolator_t)
    for name in fi.dtype.names:
        if name != "_pad":
            fi[name] = rng.uniform(-0.25, 0.25, nv).astype(np.float32)
    fi["cbx"] += np.float32(0.5)
    e.set_interpolator(fi)
    return fi


def timed(stream, fn):
    """(ms between events on the stream around fn(), ms of the host clock around it, what fn returned)"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def alternate(stream, reps, full, hollow=None):
    """{name: [(event ms, host ms)] * reps} of the calls in `full`, and of the same calls in `hollow` (the empty
    species) where given: three warm-up calls each (code objects, the scratch buffers), then all of them in turn."""
    for group in (full, hollow or {}):
        for fn in group.values():
            for _ in range(3):
                fn()
    ms, ms0 = {k: [] for k in full}, {k: [] for k in full}
    for _ in range(reps):
        for k in full:
            ms[k].append(timed(stream, full[k])[:2])
            if hollow:
                ms0[k].append(timed(stream, hollow[k])[:2])
    return ms, ms0


def header(what, args, extra=""):
    import torch
    return [f"{what} of one species: {args.cells}^3 cells x {args.ppc} per cell = {args.cells ** 3 * args.ppc} particles, tile order, {extra}{args.reps} alternating repeats",
            f"device: {torch.cuda.get_device_name(0)}"]


def call_lines(ms, ms0=None, less="kernel", extras=None):
    """one report line per call, and {name: median}, {name: median less the empty species' median}"""
    lines, med, kern = [], {}, {}
    for k, v in ms.items():
        ev, host = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        med[k] = float(np.median(ev))
        line = f"  ({k}): {np.median(ev):.3f} [{ev.min():.3f} .. {ev.max():.3f}]  (host {np.median(host):.3f})"
        if ms0 and ms0[k]:
            ev0 = np.array([x[0] for x in ms0[k]])
            kern[k] = float(np.median(ev) - np.median(ev0))
            line += f"  empty {np.median(ev0):.3f}  {less} {kern[k]:.3f}"
        lines.append(line + (extras or {}).get(k, ""))
    return lines, med, kern


def host_route(e, sp, reps, restate):
    """[(ms of get_particles, ms of restate(particles))] * reps, and what the last restate returned"""
    out, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        p = e.get_particles(sp)
        t1 = time.perf_counter()
        res = restate(p)
        out.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    return out, res


def finish(lines, out):
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
