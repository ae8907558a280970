"""What radiative cooling of a species costs (vpic_hip_species_cool, csrc/cool.hip) beside the passes that read the same
arrays, in the SAME run.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread 0.02 c:
67 M particles), freshly sorted, in tile order, with the seeded interpolator of tools/distribution_time.py
(diag_timing.set_field), in ONE process; the calls alternate:
  (a) cool, applying (32 B per particle and 72 B of the voxel's interpolator record read, 12 B written)
  (b) cool, dry (the same reads, nothing written)
  (c) cool, applying, with the per-voxel sums (64-bit global adds, and nv words copied back)
  (d) energy_p: the same arrays and the same interpolator record
  (e) 1-D cos_pitch at 512 bins: the cheapest existing pass that gathers the interpolator (24 B of the record)
and once, with the host clock: (f) get_particles + set_particles, the route a host hook over sp->p takes.
Every call is timed with events on the engine's stream around it and with the host clock; three warm-up calls each, then
the median of the repeats with their range.  The KERNEL alone is given as: events around the call minus events around the
same call on an EMPTY species of the same engine, which clears, copies and waits for exactly the same bytes and launches
nothing (energy_p launches its kernel on an empty species too).  No ratio is fixed in advance.
    python tools/cool_time.py [--out profiles/cool_time.txt] [--reps 20]        (GPU box)"""
import time

import numpy as np

import diag_timing as T

SYNC, IC, QUANTUM = 1e-4, 1e-5, 2.0 ** -50                      # (small: sixty calls leave the species where it was, nearly)


def main():
    ap = T.parser(reps=20)
    ap.add_argument("--no-route", action="store_true", help="leave (f) out (runs under a profiler)")
    args = ap.parse_args()
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc
    V, e, sp, empty, stream = T.species(args)
    T.set_field(V, e, n)
    pitch_1d = [("cos_pitch", -1.0, 2.0 / 512, 512)]
    seen = {}

    def cool(name, s, **kw):
        r = e.cool(s, SYNC, IC, QUANTUM, **kw)
        if s == sp:
            seen[name] = r
        return r

    def calls(s):
        return {"a cool, applying": lambda: cool("a", s),
                "b cool, dry": lambda: cool("b", s, dry=True),
                "c cool, applying, per-voxel sums": lambda: cool("c", s, cells=True),
                "d energy_p": lambda: e.energy_p(s),
                "e cos_pitch 512": lambda: e.distribution(s, pitch_1d)}

    ms, ms0 = T.alternate(stream, args.reps, calls(sp), calls(empty))
    assert e.species_order(sp) == "tile"
    route = None
    if not args.no_route:
        t0 = time.perf_counter()
        p = e.get_particles(sp)
        t1 = time.perf_counter()
        e.set_particles(sp, p)
        route = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3)
        del p
    e.close()

    lines = T.header("radiative cooling", args)
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call);",
              "  kernel: that median minus the median of the same call on an empty species (the same clearing, copies and wait, no launch)"]
    extras = {k: f"  {seen[k[0]].stats}" for k in ms if k[0] in seen}
    more, med, kern = T.call_lines(ms, ms0, "kernel", extras)
    lines += more
    a, b, c, d, pitch = (kern[k] for k in ms)
    lines.append(f"kernels: applying / cos_pitch (a) / (e) = {a / pitch:.2f}   applying / energy_p (a) / (d) = {a / d:.2f}   dry / applying (b) / (a) = {b / a:.2f}"
                 f"   with per-voxel sums / applying (c) / (a) = {c / a:.2f}   (nothing was fixed in advance)")
    lines.append(f"bytes of the particle arrays: (a) 32 B read + 12 B written per particle = {44 * np_ / 1e9:.3f} GB -> {44 * np_ / a / 1e6:.0f} GB/s; (b) 32 B -> {32 * np_ / b / 1e6:.0f} GB/s;"
                 f" (e) 28 B -> {28 * np_ / pitch / 1e6:.0f} GB/s; particles per second (a) {np_ / (a * 1e-3):.3e}")
    if route:
        lines.append(f"  (f get_particles + set_particles, once, host clock): {route[0]:.0f} ms + {route[1]:.0f} ms")
        lines.append(f"(f) / (a), whole calls = {(route[0] + route[1]) / med['a cool, applying']:.0f}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
