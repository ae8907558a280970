"""What the hydro moments of a SELECTION of a species cost (vpic_hip_accumulate_hydro_p_select, csrc/moments.hip) beside
the whole species' and beside the route there was.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift
0.2 c, thermal spread 0.02 c: 67 M particles) in tile order with tags 1..np and a guide field plus seeded values in the
interpolator (diag_timing.set_field), float accumulation, in ONE process; the calls alternate:
  (a) accumulate_hydro_p of the whole species: the baseline
  (b) the selected call with a selection that keeps everything (0 <= ke): the predicate's own cost
  (c) the energetic 1 %: ke >= the edge that about 1 % of the particles exceed (found from a device histogram)
  (d) a box of 1/16 of the domain (a quarter of x by a quarter of z)
  (e) ke (the energetic 10 %) and 0.5 <= cos_pitch < 1 together: the instance that reads the field for its coordinates
  (f) every 100th tag
  (g) the route this replaces, for (c): select() of the same particles to the host, upload into a scratch species,
      accumulate_hydro_p of that species
Every call is timed with events on the engine's stream around it (for (g) they enclose the copies) and with the host
clock; three warm-up calls each, then the median of the repeats with their range.
Expectation to report against: (b) within a few percent of (a) -- the predicate is arithmetic on loaded registers --
and (c) well below (a): a particle that is not kept skips its 112 atomic adds.
    python tools/moments_select_time.py [--out profiles/moments_select_time.txt] [--reps 20]        (GPU box)"""
import numpy as np

import diag_timing as T

INF = float("inf")


def main():
    ap = T.parser(reps=20)
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20"
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc

    def tag(e, sp):                                          # the loader sets no tags: give every particle its own, in the loader's order
        p = e.get_particles(sp)
        p["tag"] = np.arange(np_, dtype=np.int64) + 1
        e.set_particles(sp, p)

    V, e, sp, _, stream = T.species(args, before_sort=tag)
    T.set_field(V, e, n)
    ke_axis = [("ke", 0.0, 0.05 / 4096, 4096)]
    above = np.cumsum(e.distribution(sp, ke_axis)[::-1])[::-1]
    edge1 = float(np.argmax(above <= 0.01 * np_)) * ke_axis[0][2]
    edge10 = float(np.argmax(above <= 0.10 * np_)) * ke_axis[0][2]
    sel = {
        "b keeps everything, 0 <= ke": dict(select=[("ke", 0.0, INF)]),
        "c energetic 1 %%, ke >= %.6f" % edge1: dict(select=[("ke", edge1, INF)]),
        "d box 1/16": dict(select=[("x", 0.0, n / 4.0), ("z", 0.0, n / 4.0)]),
        "e ke >= %.6f and 0.5 <= cos_pitch < 1" % edge10: dict(select=[("ke", edge10, INF), ("cos_pitch", 0.5, 1.0)]),
        "f tag_every (100, 7)": dict(tag_every=(100, 7)),
    }
    name_c = [k for k in sel if k.startswith("c ")][0]
    count_c = e.select_count(sp, **sel[name_c])
    scratch = e.new_species(-1.0, count_c + 4096, 4096)

    def route_g():
        r = e.select(sp, cap=count_c, **sel[name_c])
        e.set_particles(scratch, r.particles)
        e.accumulate_hydro_p(scratch)

    calls = {"a whole species": lambda: e.accumulate_hydro_p(sp)}
    calls.update({k: (lambda d=d: e.accumulate_hydro_p(sp, **d)) for k, d in sel.items()})
    calls["g select + upload + accumulate_hydro_p, for (c)"] = route_g
    e.clear_hydro()
    ms, _ = T.alternate(stream, args.reps, calls)
    extras = {}
    for k, fn in calls.items():
        e.clear_hydro()
        fn()
        s = e.moments_stats()
        extras[k] = f"  summed {s[0]} ({100.0 * s[0] / np_:.2f} %): through LDS {s[1]}, through global memory {s[2]}"
    assert e.species_order(sp) == "tile"
    e.close()

    lines = T.header("hydro moments of a selection", args, "tags 1..np, float accumulation, ")
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call)"]
    more, med, _ = T.call_lines(ms, None, "", extras)
    lines += more
    a, b, c, g = med["a whole species"], med["b keeps everything, 0 <= ke"], med[name_c], med["g select + upload + accumulate_hydro_p, for (c)"]
    lines.append(f"(b) / (a) = {b / a:.3f} (expected: within a few percent of 1)   (c) / (a) = {c / a:.3f} (expected: well below 1)   (g) / (c) = {g / c:.1f}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
