"""What a phase-space distribution of a species costs (vpic_hip_species_distribution, csrc/distribution.hip) beside the
passes a user had before it.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread
0.02 c) in tile order -- the state profiles/spectrum_time.txt used -- in ONE process:
  (a) x-ux at 256 x 256 bins (i, dx, ux: 12 B per particle; x bins of half a cell: the sliding window)
  (b) 1-D ux at 512 bins (i, ux: 8 B per particle; the histogram in LDS)
  (c) energy_spectrum, log bins only (16 B per particle): the yardstick, re-measured here
  (d) energy_p (32 B per particle and the interpolator)
  (e) get_particles + numpy.histogram2d: the only route there was
and, in the frame of the local magnetic field (csrc/dist_coords.h; the interpolator holds a guide field plus seeded values
in every voxel, diag_timing.set_field), each beside the box-frame row of the same shape:
  (f) u_par-u_perp at 256 x 256 bins (i, dx, dy, dz, ux, uy, uz and 24 B of the voxel's interpolator record; global adds)
  (g) ux-uz at 256 x 256 bins (i, ux, uz; global adds): the neighbour of (f)
  (h) 1-D pitch at 512 bins (the same reads as (f); LDS): its neighbour is (b)
  (i) select(fields=True) of every particle + numpy: the route (f) and (h) replace (72 B per particle to the host)
(a) to (d) alternate.  Every call is timed with the host clock, and with events on the engine's stream around it.  The
events enclose the clearing of the counters and the copy of the result as well, so the KERNEL alone is given as: events
around the call minus events around the same call on an EMPTY species of the same engine, which clears, copies and
waits for exactly the same bytes and launches nothing (energy_p launches its kernel on an empty species too, so its
difference leaves the launch itself out).
`rocprofv3 --kernel-trace --stats -- python tools/distribution_time.py --no-route-e` gives the kernels' own durations.
    python tools/distribution_time.py [--out profiles/distribution_time.txt] [--reps 20]        (GPU box)"""
import numpy as np

import diag_timing as T


def main():
    ap = T.parser(reps=20)
    ap.add_argument("--no-route-e", action="store_true", help="leave (e) out (runs under a profiler)")
    ap.add_argument("--box-frame-only", action="store_true", help="leave (f), (h) and (i) out: a library from before the field-frame coordinates "
                                                                  "(VPIC_HIP_LIB), to compare the other rows with it")
    args = ap.parse_args()
    field = not args.box_frame_only
    from test_spectrum_ref import deck_params
    n, ppc, vth = args.cells, args.ppc, T.VTH
    np_ = n ** 3 * ppc
    V, e, sp, empty, stream = T.species(args)
    T.set_field(V, e, n)
    prm = deck_params(vth)
    x_ux = [("x", 0.0, n / 256.0, 256), ("ux", 0.2 - 6 * vth, 12 * vth / 256, 256)]
    ux_1d = [("ux", 0.2 - 6 * vth, 12 * vth / 512, 512)]
    par_perp = [("u_par", -0.32, 0.64 / 256, 256), ("u_perp", 0.0, 0.32 / 256, 256)]
    ux_uz = [("ux", 0.2 - 6 * vth, 12 * vth / 256, 256), ("uz", -6 * vth, 12 * vth / 256, 256)]
    pitch_1d = [("cos_pitch", -1.0, 2.0 / 512, 512)]

    def calls(s):
        c = {
            "a x-ux 256 x 256": lambda: e.distribution(s, x_ux),
            "b ux 512": lambda: e.distribution(s, ux_1d),
            "c energy_spectrum, log bins only": lambda: e.energy_spectrum(s, n_log=prm["n_log"], log_lo=prm["log_lo"], d_log=prm["d_log"]),
            "d energy_p": lambda: e.energy_p(s),
            "g ux-uz 256 x 256": lambda: e.distribution(s, ux_uz),
        }
        if field:
            c["f u_par-u_perp 256 x 256"] = lambda: e.distribution(s, par_perp)
            c["h pitch 512"] = lambda: e.distribution(s, pitch_1d)
        return c

    ms, ms0 = T.alternate(stream, args.reps, calls(sp), calls(empty))
    stats = {}
    hist = e.distribution(sp, x_ux)
    stats["a x-ux 256 x 256"] = e.distribution_stats()
    hist1 = e.distribution(sp, ux_1d)
    stats["b ux 512"] = e.distribution_stats()
    for name, axes in (("f u_par-u_perp 256 x 256", par_perp), ("g ux-uz 256 x 256", ux_uz), ("h pitch 512", pitch_1d)):
        if not field and axes is not ux_uz:
            continue
        e.distribution(sp, axes)
        stats[name] = e.distribution_stats()
    route_e, same = [], None
    if not args.no_route_e:
        def histogram(p):
            x = (p["i"].astype(np.int64) % (n + 2) - 1).astype(np.float64) + (p["dx"].astype(np.float64) + 1.0) * 0.5
            return np.histogram2d(p["ux"].astype(np.float64), x, bins=(256, 256),
                                  range=((x_ux[1][1], x_ux[1][1] + 256 * x_ux[1][2]), (0.0, float(n))))[0]
        route_e, want = T.host_route(e, sp, 3, histogram)
        # numpy's bins are found by another arithmetic (and its last bin is closed): totals are compared, bins nearly
        same = (int(want.sum()), int(hist.sum()), int(np.abs(want.astype(np.int64) - hist.astype(np.int64)).sum()))
    route_i = None
    if field and not args.no_route_e:
        import time
        t0 = time.perf_counter()
        r = e.select(sp, cap=np_, fields=True)
        t1 = time.perf_counter()
        u = [r.particles[c].astype(np.float64) for c in ("ux", "uy", "uz")]
        b = [r.fields[:, k].astype(np.float64) for k in (3, 4, 5)]
        u_par = ((u[0] * b[0] + u[1] * b[1]) + u[2] * b[2]) / np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        u_perp = np.sqrt(np.maximum(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) - u_par * u_par, 0.0))
        want = np.histogram2d(u_perp, u_par, bins=(256, 256), range=((0.0, 0.32), (-0.32, 0.32)))[0]
        route_i = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, int(want.sum()), int(e.distribution(sp, par_perp).sum()))
        del r, u, b
    e.close()

    lines = T.header("phase-space distributions", args)
    lines += ["milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call);",
              "  kernel: that median minus the median of the same call on an empty species (the same clearing, copies and wait, no launch)"]
    extras = {k: f"  seen {s[0]} kept {s[1]} counted {s[2]} through global memory (out[3]) {s[3]}" for k, s in stats.items()}
    more, med, kern = T.call_lines(ms, ms0, "kernel", extras)
    lines += more
    if route_e:
        lines.append(f"  (e get_particles + numpy.histogram2d, 3 repeats): download {np.median([c[0] for c in route_e]):.0f} ms + numpy {np.median([c[1] for c in route_e]):.0f} ms;"
                     f" numpy counted {same[0]}, the device {same[1]}, sum of |differences| over the bins {same[2]}")
        lines.append(f"(e) / (a) = {np.median([c[0] + c[1] for c in route_e]) / med['a x-ux 256 x 256']:.0f}")
    ka, kb, kc = kern["a x-ux 256 x 256"], kern["b ux 512"], kern["c energy_spectrum, log bins only"]
    lines.append(f"kernels: (a) / (c) = {ka / kc:.2f} (hoped for: up to 1.5)   (b) / (c) = {kb / kc:.2f} (hoped for: up to 1)")
    lines.append(f"bytes the kernels read: (a) 12 B per particle = {12 * np_ / 1e9:.3f} GB -> {12 * np_ / ka / 1e6:.0f} GB/s; (b) 8 B -> {8 * np_ / kb / 1e6:.0f} GB/s;"
                 f" (c) 16 B -> {16 * np_ / kc / 1e6:.0f} GB/s")
    lines.append(f"x-ux: {int(np.count_nonzero(hist))} of {hist.size} bins populated, fullest {int(hist.max())}; ux: fullest {int(hist1.max())}")
    if not field:
        return T.finish(lines, args.out)
    kf, kg, kh = kern["f u_par-u_perp 256 x 256"], kern["g ux-uz 256 x 256"], kern["h pitch 512"]
    lines.append(f"in the frame of the local field, kernels: (f) / (g) = {kf / kg:.2f}   (h) / (b) = {kh / kb:.2f}   (nothing was fixed in advance; above 2: say where the time goes)")
    lines.append(f"bytes the kernels read: (f) and (h) 28 B per particle + 24 B of the voxel's record per particle through the caches; (f) {28 * np_ / kf / 1e6:.0f} GB/s of particle arrays,"
                 f" (g) 12 B -> {12 * np_ / kg / 1e6:.0f} GB/s, (h) {28 * np_ / kh / 1e6:.0f} GB/s")
    if route_i:
        lines.append(f"  (i select(fields=True) of everything + numpy.histogram2d, once): select {route_i[0]:.0f} ms + numpy {route_i[1]:.0f} ms; numpy counted {route_i[2]}, the device {route_i[3]}")
        lines.append(f"(i) / (f) = {(route_i[0] + route_i[1]) / med['f u_par-u_perp 256 x 256']:.0f}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
