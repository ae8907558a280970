"""What per-bin sums of particle quantities cost (vpic_hip_species_distribution_sums, csrc/distribution.hip) beside the
unweighted histogram of the same descriptor.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c,
thermal spread 0.02 c) in tile order, the interpolator a guide field plus seeded values in every voxel
(diag_timing.set_field), in ONE process, every sums call beside `distribution` of the same descriptor, alternating:
  (a) 1-D ke at 512 bins with one value, q (i, ux, uy, uz, q: 20 B per particle; counts and sums in LDS)
  (b) 1-D ke at 512 bins with four values, q; q ke; q edotv; mu (32 B per particle and the 72 B of the voxel's
      interpolator record; LDS) -- the histogram beside it reads 16 B per particle and no record
  (c) ux-uz at 256 x 256 bins with one value, q (i, ux, uz, q: 16 B per particle; global adds)
  (r) select(fields=True) of every particle + numpy: the route (b) replaces (72 B per particle to the host), once
Every call is timed with the host clock, and with events on the engine's stream around it; the KERNEL alone is given as
events around the call minus events around the same call on an EMPTY species of the same engine (the same clearing, copies
and wait, no launch).
    python tools/dist_sums_time.py [--out profiles/dist_sums_time.txt] [--reps 20] [--no-route]        (GPU box)"""
import time

import numpy as np

import diag_timing as T


def main():
    ap = T.parser(reps=20)
    ap.add_argument("--no-route", action="store_true", help="leave (r) out (runs under a profiler)")
    args = ap.parse_args()
    n, ppc, vth = args.cells, args.ppc, T.VTH
    np_ = n ** 3 * ppc
    V, e, sp, empty, stream = T.species(args)
    T.set_field(V, e, n)
    ke = [("ke", 0.0, 0.05 / 512, 512)]
    ux_uz = [("ux", 0.2 - 6 * vth, 12 * vth / 256, 256), ("uz", -6 * vth, 12 * vth / 256, 256)]
    one = [(("q",), 1e-10)]
    four = [(("q",), 1e-10), (("q", "ke"), 1e-12), (("q", "edotv"), 1e-11), (("mu", "one"), 1e-8)]
    shapes = {"a ke 512, 1 value": (ke, one), "b ke 512, 4 values": (ke, four), "c ux-uz 256 x 256, 1 value": (ux_uz, one)}

    def calls(s):
        c = {}
        for name, (axes, values) in shapes.items():
            c[name] = lambda axes=axes, values=values: e.distribution_sums(s, axes, values)
            c[name + ": the histogram alone"] = lambda axes=axes: e.distribution(s, axes)
        return c

    ms, ms0 = T.alternate(stream, args.reps, calls(sp), calls(empty))
    extras, results = {}, {}
    for name, (axes, values) in shapes.items():
        results[name] = e.distribution_sums(sp, axes, values)
        s = e.distribution_sums_stats()
        same = np.array_equal(results[name].counts, e.distribution(sp, axes))
        extras[name] = (f"  seen {s[0]} kept {s[1]} counted {s[2]} through global memory {s[3]} refused {list(s[4:4 + len(values)])};"
                        f" counts equal the histogram's: {same}")
    route = None
    if not args.no_route:
        t0 = time.perf_counter()
        r = e.select(sp, cap=np_, fields=True)
        t1 = time.perf_counter()
        u = [r.particles[c].astype(np.float64) for c in ("ux", "uy", "uz")]
        f = [r.fields[:, k].astype(np.float64) for k in range(6)]
        q = r.particles["q"].astype(np.float64)
        gamma = np.sqrt(((1.0 + u[0] * u[0]) + u[1] * u[1]) + u[2] * u[2])
        b = np.sqrt((f[3] * f[3] + f[4] * f[4]) + f[5] * f[5])
        u_par = ((u[0] * f[3] + u[1] * f[4]) + u[2] * f[5]) / b
        mu = np.maximum(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) - u_par * u_par, 0.0) / (2.0 * b)
        edotv = ((f[0] * u[0] + f[1] * u[1]) + f[2] * u[2]) / gamma
        t = (gamma - 1.0) / ke[0][2]
        ok = (t >= 0) & (t < 512)
        bins = t[ok].astype(np.int64)
        want = [np.bincount(bins, weights=w[ok], minlength=512) for w in (q, q * (gamma - 1.0), q * edotv, mu)]
        t2 = time.perf_counter()
        got = results["b ke 512, 4 values"].sums
        worst = [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, want)]
        route = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, worst)
        del r, u, f
    e.close()

    lines = T.header("per-bin sums beside the histograms", args)
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call);",
              "  kernel: that median minus the median of the same call on an empty species (the same clearing, copies and wait, no launch)"]
    more, med, kern = T.call_lines(ms, ms0, "kernel", extras)
    lines += more
    for name in shapes:
        lines.append(f"({name[0]}) sums / histogram of the same descriptor: kernels {kern[name] / kern[name + ': the histogram alone']:.2f}, "
                     f"calls {med[name] / med[name + ': the histogram alone']:.2f}")
    ka, kb, kc = (kern[name] for name in shapes)
    lines.append(f"bytes the kernels read of the particle arrays: (a) 20 B per particle = {20 * np_ / 1e9:.3f} GB -> {20 * np_ / ka / 1e6:.0f} GB/s; "
                 f"(b) 32 B (+ 72 B of the voxel's record through the caches) -> {32 * np_ / kb / 1e6:.0f} GB/s; (c) 16 B -> {16 * np_ / kc / 1e6:.0f} GB/s")
    if route:
        lines.append(f"  (r select(fields=True) of everything + numpy, the four sums of (b), once): select {route[0]:.0f} ms + numpy {route[1]:.0f} ms; "
                     f"largest |device sum - numpy's float sum| over the bins, relative to the largest bin: {', '.join(f'{w:.1e}' for w in route[2])}")
        lines.append(f"(r) / (b) = {(route[0] + route[1]) / med['b ke 512, 4 values']:.0f}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
