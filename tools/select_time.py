"""What gathering a few particles of a species costs (vpic_hip_species_select, csrc/select.hip) beside the route there
was.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread 0.02 c) in tile order
with tags 1..np -- the state profiles/distribution_time.txt used, plus the tags -- in ONE process:
  (a)  the energetic tail: ke >= the edge that about 1 % of the particles exceed (found from a device histogram)
  (b)  tag_every = (100, 7)
  (c)  a box of 1/16 of the domain (a quarter of x by a quarter of z), particles only
  (cf) the same with fields and index
  (a0) select_count of (a): launches 1 and 2 alone
  (p0) select_count of 0.9 <= pitch < 1, in the frame of the local field (i, the offsets, the momenta and 24 B of the voxel's
       interpolator record, which holds a guide field plus seeded values: diag_timing.set_field): its neighbour is (a0)
  (d)  the 1-D ke distribution over the same species (i, ux, uy, uz: the bytes launch 1 of (a) reads): the yardstick
  (e)  get_particles + a numpy mask: the only route there was, for (a)
(a) to (d) alternate.  Every call is timed with the host clock, and with events on the engine's stream around it; the
events enclose the copies of the result as well.  "kernels" is: events around the call minus events around the same
call on an EMPTY species of the same engine (the same clearing, copies of statistics and waits, no launch) -- for a
selection that still holds the copy of its records to the host, so the kernels by themselves are (a0) and what
`rocprofv3 --kernel-trace --stats -- python tools/select_time.py --no-route-e --only ''` reports (a run of its own, (a) alone).
Expectation to report against: launch 1 reads what (d) reads and writes 1 bit per particle; launch 3 reads np / 8 bytes
and 48 B per kept particle; so the kernels of (a) together should cost little more than the kernel of (d).
    python tools/select_time.py [--out profiles/select_time.txt] [--reps 20]        (GPU box)"""
import numpy as np

import diag_timing as T


def main():
    ap = T.parser(reps=20)
    ap.add_argument("--no-route-e", action="store_true", help="leave (e) out (runs under a profiler)")
    ap.add_argument("--only", default=None, help="selections to run beside (a), (a0) and (d), e.g. 'b' or 'c,cf' or '' (so that a kernel trace's "
                                                 "per-kernel averages are those of one selection)")
    ap.add_argument("--box-frame-only", action="store_true", help="leave (p0) out: a library from before the field-frame coordinates (VPIC_HIP_LIB)")
    args = ap.parse_args()
    field = not args.box_frame_only
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc

    def tag(e, sp):                                          # the loader sets no tags: give every particle its own, in the loader's order
        p = e.get_particles(sp)
        p["tag"] = np.arange(np_, dtype=np.int64) + 1
        e.set_particles(sp, p)

    V, e, sp, empty, stream = T.species(args, before_sort=tag)
    T.set_field(V, e, n)
    # the edge of the energetic 1 %: from the 1-D ke histogram on the device
    ke_axis = [("ke", 0.0, 0.05 / 4096, 4096)]
    h = e.distribution(sp, ke_axis)
    above = np.cumsum(h[::-1])[::-1]
    edge = float(np.argmax(above <= 0.01 * np_)) * ke_axis[0][2]
    sel = {
        "a tail, ke >= %.6f" % edge: dict(select=[("ke", edge, float("inf"))]),
        "b tag_every (100, 7)": dict(tag_every=(100, 7)),
        "c box 1/16": dict(select=[("x", 0.0, n / 4.0), ("z", 0.0, n / 4.0)]),
        "cf box 1/16, fields and index": dict(select=[("x", 0.0, n / 4.0), ("z", 0.0, n / 4.0)], fields=True, index=True),
    }
    name_a = next(iter(sel))
    if args.only is not None:
        sel = {k: d for k, d in sel.items() if k == name_a or k.split()[0] in args.only.split(",")}
    counts = {k: e.select_count(sp, **{a: b for a, b in d.items() if a not in ("fields", "index")}) for k, d in sel.items()}
    def calls(s):
        c = {k: (lambda d=d, k=k: e.select(s, cap=counts[k], **d)) for k, d in sel.items()}     # (cap given: one call, no counting call first)
        c["a0 select_count of (a)"] = lambda: e.select_count(s, **sel[name_a])
        if field:
            c["p0 select_count of 0.9 <= pitch < 1"] = lambda: e.select_count(s, select=[("cos_pitch", 0.9, 1.0)])
        c["d ke distribution, 4096 bins"] = lambda: e.distribution(s, ke_axis)
        return c

    full = calls(sp)
    ms, ms0 = T.alternate(stream, args.reps, full, calls(empty))
    stats = {}
    for k in sel:
        r = full[k]()
        stats[k] = (e.select_stats(), r)
    route_e, same = [], None
    if not args.no_route_e:
        def mask(p):
            u = [p[c].astype(np.float64) for c in ("ux", "uy", "uz")]
            return p[np.sqrt(((1.0 + u[0] * u[0]) + u[1] * u[1]) + u[2] * u[2]) - 1.0 >= edge]
        want = stats[name_a][1]
        route_e, kept = T.host_route(e, sp, 3, mask)
        same = (len(kept), want.count, kept.tobytes() == want.particles.tobytes())
    e_pitch = e.select_count(sp, select=[("cos_pitch", 0.9, 1.0)]) if field else 0
    e.close()

    lines = T.header("selected particles", args, "tags 1..np, ")
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call);",
              "  less empty: that median minus the median of the same call on an empty species (the same clearing, waits and copies of statistics,",
              "  no launch); for a selection it still holds the copy of the records to the host"]
    extras = {}
    for k, (s, r) in stats.items():
        per = 48 + (32 if r.fields is not None else 0)
        extras[k] = f"  seen {s[0]} kept {s[1]} ({100.0 * s[1] / max(s[0], 1):.2f} %) written {s[2]} chunks {s[3]}; {s[2] * per / 1e6:.1f} MB to the host"
    more, med, kern = T.call_lines(ms, ms0, "less empty", extras)
    lines += more
    if route_e:
        total = float(np.median([c[0] + c[1] for c in route_e]))
        lines.append(f"  (e get_particles + numpy mask for (a), 3 repeats): download {np.median([c[0] for c in route_e]):.0f} ms + numpy {np.median([c[1] for c in route_e]):.0f} ms;"
                     f" numpy kept {same[0]}, the device {same[1]}, identical bytes: {same[2]}")
        lines.append(f"(e) / (a) = {total / med[name_a]:.0f}")
    k0, kd = kern["a0 select_count of (a)"], kern["d ke distribution, 4096 bins"]
    lines.append(f"launches 1 and 2 of (a) against the ke distribution kernel: (a0) / (d) = {k0 / kd:.2f}; (a) less empty / (d) = {kern[name_a] / kd:.2f}"
                 " (expected: little more than 1, plus the copy of the records)")
    lines.append(f"bytes launch 1 of (a) reads: 16 B per particle = {16 * np_ / 1e9:.3f} GB -> {16 * np_ / k0 / 1e6:.0f} GB/s over (a0); "
                 f"(b) reads 12 B per particle (i, tag), (c) 12 B (i, dx, dz)")
    if not field:
        return T.finish(lines, args.out)
    kp = kern["p0 select_count of 0.9 <= pitch < 1"]
    lines.append(f"in the frame of the local field: (p0) / (a0) = {kp / k0:.2f}; (p0) keeps {e_pitch} of {np_}  (nothing was fixed in advance; above 2: say where the time goes)")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
