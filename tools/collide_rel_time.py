"""What the relativistic pair costs (vpic_hip_collide_relativistic, csrc/collide.hip: collide_pair_rel, in double) beside the
existing one (vpic_hip_collide, in float), the yardstick, in the SAME run.  One species of BASELINE configs[1] (128^3 cells,
32 per cell, drift 0.2 c, thermal spread 0.02 c: 67 M particles), freshly sorted, in tile order, and a second species of the
same size beside it (mass 100, a tenth of the thermal spread), in ONE process as tools/collide_time.py does it; the calls
alternate:
  (a) vpic_hip_collide within the one species               (A) vpic_hip_collide_relativistic within it
  (b) vpic_hip_collide between the two                      (B) vpic_hip_collide_relativistic between the two
  (c) the checking pass alone: collide against an EMPTY species (both models share it)
Every call is timed with events on the engine's stream around it and with the host clock; three warm-up calls each, then
the median of the repeats with their range.  Every call must report that it sorted nothing.  No ratio is fixed in advance.
    python tools/collide_rel_time.py [--out profiles/collide_rel_time.txt] [--reps 20]        (GPU box)"""
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
    one = dict(m_a=1.0, wq_a=float(ppc), cvar=1e-7, dt=dt, seed=1)
    two = dict(one, m_b=100.0, wq_b=float(ppc), cvar=4e-7)
    counter, seen = [0], {}

    def collide(name, *species, **kw):
        counter[0] += 1
        e.collide(*species, call=counter[0], **kw)
        seen[name] = e.collide_stats()
        assert seen[name]["sorted_first"] == 0, seen[name]

    calls = {"a collide, one species": lambda: collide("a", sp, **one),
             "A collide relativistic, one species": lambda: collide("A", sp, relativistic=True, **one),
             "b collide, two species": lambda: collide("b", sp, ion, **two),
             "B collide relativistic, two species": lambda: collide("B", sp, ion, relativistic=True, **two),
             "c checking pass alone (collide against an empty species)": lambda: collide("c", sp, empty, **two)}
    ms, _ = T.alternate(stream, args.reps, calls)
    assert e.species_order(sp) == "tile" and e.species_order(ion) == "tile"
    e.close()

    lines = T.header("binary collisions, the relativistic pair beside the existing one,", args, "a second species of the same size beside it, ")
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call)"]
    extras = {k: "  " + ", ".join(f"{a} {b}" for a, b in seen[k[0]].items()) for k in calls if k[0] in seen}
    more, med, _ = T.call_lines(ms, None, "", extras)
    lines += more
    a, A, b, B, c = (med[k] for k in calls)
    lines.append(f"one species: relativistic / existing, whole call (A) / (a) = {A / a:.2f}; less the shared checking pass ((A) - (c)) / ((a) - (c)) = {(A - c) / (a - c):.2f}")
    lines.append(f"two species: relativistic / existing, whole call (B) / (b) = {B / b:.2f}; less the shared checking pass ((B) - (c)) / ((b) - (c)) = {(B - c) / (b - c):.2f}")
    lines.append(f"pairs per second of the relativistic launch alone: one species {seen['A']['pairs'] / ((A - c) * 1e-3):.3e}, two species {seen['B']['pairs'] / ((B - c) * 1e-3):.3e}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
