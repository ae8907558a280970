"""What accumulate_hydro_p / accumulate_rho_p cost summed by tile (csrc/moments.hip) beside the paths there were before.
One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread 0.02 c: 67 M particles) in tile
order, pushed a few steps since its sort, in ONE process on two engines that hold the same particles: "before" is created
under VPIC_HIP_MOMENTS_TILED=0 (the float paths sort by voxel and sum by cell, the deterministic rho is one global 64-bit
atomic per node and particle; there was no deterministic hydro), "tiled" without it.
  (a) float accumulate_hydro_p before: the call (it sorts by voxel) AND the sort by tile the next push then needs
  (b) float accumulate_hydro_p by tile        (c) deterministic accumulate_hydro_p by tile (with its one wait for the stream)
  (d) deterministic accumulate_rho_p per particle / by tile        (e) float accumulate_rho_p before (+ the tile sort) / by tile
The calls alternate; each is timed with events on the engine's stream, medians over the repeats after a warm-up.
    python tools/moments_time.py [--out profiles/moments_time.txt] [--reps 10]        (GPU box)"""
import os

import numpy as np

import diag_timing as T


def main():
    ap = T.parser(reps=10)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc

    def engine(tiled):
        if not tiled:
            os.environ["VPIC_HIP_MOMENTS_TILED"] = "0"        # (read when the engine is created)
        _, e, sp, _, stream = T.species(args)
        os.environ.pop("VPIC_HIP_MOMENTS_TILED", None)
        e.clear_accumulators()
        for _ in range(args.steps):
            e.advance_p(sp)
        assert e.species_order(sp) == "tile" and e.nm(sp) == 0
        return e, sp, stream

    before, tiled = engine(False), engine(True)

    def timed(side, fn):
        return T.timed(side[2], lambda: fn(side[0], side[1]))[0]

    def resort(e, sp):
        e.sort_p(sp)
        assert e.species_order(sp) == "tile"

    def hydro(e, sp):
        e.accumulate_hydro_p(sp)

    def rho(e, sp):
        e.accumulate_rho_p(sp)

    ms, stats = {}, {}

    def measure(key, side, fn, then_resort=False):
        t = timed(side, fn)
        s = side[0].moments_stats()
        order = side[0].species_order(side[1])
        t2 = timed(side, resort) if then_resort else 0.0
        ms.setdefault(key, []).append((t, t2))
        stats[key] = (s, order)

    for rep in range(-2, args.reps):                         # two warm-up rounds: code objects, scratch buffers, the 64-bit words
        for e, _, _ in (before, tiled):
            e.set_accumulation("float")
            e.clear_hydro(); e.clear_rhof()
        measure("a float hydro, before", before, hydro, then_resort=True)
        measure("b float hydro, by tile", tiled, hydro)
        measure("e float rho, before", before, rho, then_resort=True)
        measure("e float rho, by tile", tiled, rho)
        for e, _, _ in (before, tiled):
            e.set_accumulation("deterministic")
        measure("c deterministic hydro, by tile", tiled, hydro)
        measure("c deterministic hydro, per particle", before, hydro)
        measure("d deterministic rho, per particle", before, rho)
        measure("d deterministic rho, by tile", tiled, rho)
        if rep < 0:
            ms.clear()
    for e, _, _ in (before, tiled):
        e.close()

    lines = T.header("hydro moments and rho", args, f"{args.steps} pushes since the sort, ")
    lines += ["milliseconds: median [min .. max] between events on the engine's stream around the call; '+ sort': the sort by tile that puts",
              "  the species back into the order the push needs, timed the same way right after the call; statistics: live, through LDS, through global memory, out of range"]
    med = {}
    for k, v in ms.items():
        t, t2 = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        med[k] = float(np.median(t + t2))
        line = f"  ({k}): {np.median(t):.3f} [{t.min():.3f} .. {t.max():.3f}]"
        if t2.any():
            line += f" + sort {np.median(t2):.3f} [{t2.min():.3f} .. {t2.max():.3f}] = {med[k]:.3f}"
        lines.append(line + f"   statistics {stats[k][0]}, order after the call: {stats[k][1]}")
    a, b, c = med["a float hydro, before"], med["b float hydro, by tile"], med["c deterministic hydro, by tile"]
    d0, d1 = med["d deterministic rho, per particle"], med["d deterministic rho, by tile"]
    e0, e1 = med["e float rho, before"], med["e float rho, by tile"]
    lines.append(f"hydro: (b) / (a) = {b / a:.2f}   (c) / (a) = {c / a:.2f} (hoped for: up to 1)   deterministic per particle / by tile = {med['c deterministic hydro, per particle'] / c:.1f}")
    lines.append(f"rho: deterministic by tile / per particle = {d1 / d0:.2f} ({d1 * 26e6 / np_:.2f} ms per 26 M particles; hoped for: well under the 9.6 ms of"
                 f" profiles/r04_production_deck_slab_kernel_stats.csv)   float by tile / before = {e1 / e0:.2f}")
    lines.append(f"decision (float mode keeps the path there was before where the tile path is not faster): hydro {'by tile' if b < a else 'AS BEFORE'}, rho {'by tile' if e1 < e0 else 'AS BEFORE'}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
