"""What binary collisions on the device cost (vpic_hip_collide, csrc/collide.hip) beside two streaming passes over the same
species and beside the route they replace.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c,
thermal spread 0.02 c: 67 M particles), freshly sorted, in tile order, and a second species of the same size beside it
(mass 100, a tenth of the thermal spread), in ONE process; the calls alternate:
  (a) collide within the one species                      (b) collide between the two
  (c) the checking pass alone: collide against an EMPTY species -- the pass over the 67 M voxel indices and the ranges, and
      a launch whose workgroups all leave at once
  (d) sort_p of the species (which leaves it freshly sorted for the next round)        (e) energy_p of it
Every call is timed with events on the engine's stream around it and with the host clock; three warm-up calls each, then
the median of the repeats with their range.  Every collide call must report that it sorted nothing.
  (f) the route the call replaces, a deck that collides on the host: get_particles (48 B per particle down), the pairing
      and scattering on the host, set_particles (48 B per particle up).  The two copies are timed whole, three times; the
      host loop is tests/collide_ref.py -- numpy scalars in a Python loop, NOT what a compiled deck would run -- timed on
      the first 2048 cells and scaled to the species, and reported apart so that the copies alone can be read off.
No figure is fixed in advance: nobody has measured this operator.
    python tools/collide_time.py [--out profiles/collide_time.txt] [--reps 20]        (GPU box)"""
import time

import numpy as np

import diag_timing as T


def main():
    ap = T.parser(reps=20)
    args = ap.parse_args()
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc
    V, e, sp, empty, stream = T.species(args)
    dt = float(e.grid.dt)
    ion = e.new_species(0.01, np_ + 4096, np_ // 8)
    e.load_maxwellian(ion, ppc, 2, 1.0 / ppc, (0.0, 0.0, 0.0), T.VTH / 10)
    e.sort_p(ion)
    assert e.species_order(ion) == "tile"
    # w = |q| wq = 1; s2 = cvar w N dt / (V m_ab^2 g^3) is a few tenths at g ~ 0.03 (what a call costs does not depend on it)
    one = dict(m_a=1.0, wq_a=float(ppc), cvar=1e-7, dt=dt, seed=1)
    two = dict(one, m_b=100.0, wq_b=float(ppc), cvar=4e-7)
    counter, seen = [0], {}

    def collide(name, *species, **kw):
        counter[0] += 1
        e.collide(*species, call=counter[0], **kw)
        seen[name] = e.collide_stats()
        assert seen[name]["sorted_first"] == 0, seen[name]

    calls = {"a collide, one species": lambda: collide("a", sp, **one),
             "b collide, two species": lambda: collide("b", sp, ion, **two),
             "c checking pass alone (collide against an empty species)": lambda: collide("c", sp, empty, **two),
             "d sort_p": lambda: e.sort_p(sp),
             "e energy_p": lambda: e.energy_p(sp)}
    ms, _ = T.alternate(stream, args.reps, calls)
    assert e.species_order(sp) == "tile" and e.species_order(ion) == "tile"

    # (f) the host route
    import collide_ref as R
    copies = []
    for _ in range(3):
        t0 = time.perf_counter()
        p = e.get_particles(sp)
        t1 = time.perf_counter()
        e.set_particles(sp, p)
        e.sync()
        copies.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    sub = p[:2048 * ppc]
    rng = np.random.default_rng(1)
    draws = np.stack([rng.standard_normal(len(sub)), np.ones(len(sub)), np.zeros(len(sub)), rng.uniform(0, 1, len(sub))], 1).astype(np.float32)
    t0 = time.perf_counter()
    _, _, st = R.collide(sub, None, volume=np.float32(1.0), draws=draws, sp_a=sp, call=1, **one)
    loop_ms = (time.perf_counter() - t0) * 1e3 * np_ / len(sub)
    e.close()

    lines = T.header("binary collisions", args, "a second species of the same size beside it, ")
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call)"]
    extras = {k: "  " + ", ".join(f"{a} {b}" for a, b in seen[k[0]].items()) for k in calls if k[0] in seen}
    more, med, _ = T.call_lines(ms, None, "", extras)
    lines += more
    a, b, c, d, en = (med[k] for k in calls)
    down, up = float(np.median([x[0] for x in copies])), float(np.median([x[1] for x in copies]))
    lines.append(f"  (f) the host route, host clock: get_particles {down:.0f} ms, set_particles {up:.0f} ms (medians of 3); the pairing and scattering in "
                 f"tests/collide_ref.py (a Python loop, {st['pairs']} pairs of 2048 cells timed, scaled to the species) {loop_ms / 1e3:.0f} s")
    lines.append(f"one species: (a) / (d) sort_p = {a / d:.2f}   (a) / (e) energy_p = {a / en:.2f}   checking pass (c) / (a) = {c / a:.2f}   "
                 f"the copies of (f) alone / (a) = {(down + up) / a:.0f}   (f) with the Python loop / (a) = {(down + up + loop_ms) / a:.0f}")
    lines.append(f"two species: (b) / (d) sort_p = {b / d:.2f}   (b) / (a) = {b / a:.2f}")
    lines.append(f"bytes the call streams per particle of a species: 4 (the checking pass) + 16 read + 12 written (the launch) = 32; at (a) that is "
                 f"{32.0 * np_ / (a * 1e-3) / 1e9:.0f} GB/s")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
