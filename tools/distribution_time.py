"""What a phase-space distribution of a species costs (vpic_hip_species_distribution, csrc/distribution.hip) beside the
passes a user had before it.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread
0.02 c) in tile order -- the state profiles/spectrum_time.txt used -- in ONE process:
  (a) x-ux at 256 x 256 bins (i, dx, ux: 12 B per particle; x bins of half a cell: the sliding window)
  (b) 1-D ux at 512 bins (i, ux: 8 B per particle; the histogram in LDS)
  (c) energy_spectrum, log bins only (16 B per particle): the yardstick, re-measured here
  (d) energy_p (32 B per particle and the interpolator)
  (e) get_particles + numpy.histogram2d: the only route there was
(a) to (d) alternate.  Every call is timed with the host clock, and with events on the engine's stream around it.  The
events enclose the clearing of the counters and the copy of the result as well, so the KERNEL alone is given as: events
around the call minus events around the same call on an EMPTY species of the same engine, which clears, copies and
waits for exactly the same bytes and launches nothing (energy_p launches its kernel on an empty species too, so its
difference leaves the launch itself out).
`rocprofv3 --kernel-trace --stats -- python tools/distribution_time.py --no-route-e` gives the kernels' own durations.
    python tools/distribution_time.py [--out profiles/distribution_time.txt] [--reps 20]        (GPU box)"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=32)
    ap.add_argument("--no-route-e", action="store_true", help="leave (e) out (runs under a profiler)")
    args = ap.parse_args()
    import torch
    from test_spectrum_ref import deck_params
    V = importlib.import_module("old-vpic_amd")
    n, ppc, vth = args.cells, args.ppc, 0.02
    e = V.Engine(V.make_grid(n, n, n, float(n), float(n), float(n), np.float32(0.95 / np.sqrt(3.0))))
    e.set_vacuum()
    e.set_sort_order("engine")
    np_ = n ** 3 * ppc
    sp = e.new_species(-1.0, np_ + 4096, np_ // 8)
    empty = e.new_species(-1.0, 4096, 64)
    e.load_maxwellian(sp, ppc, 1, -1.0 / ppc, (0.2, 0.0, 0.0), vth)
    e.load_interpolator()
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    prm = deck_params(vth)
    x_ux = [("x", 0.0, n / 256.0, 256), ("ux", 0.2 - 6 * vth, 12 * vth / 256, 256)]
    ux_1d = [("ux", 0.2 - 6 * vth, 12 * vth / 512, 512)]
    stream = torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", 0))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    def calls(s):
        return {
            "a x-ux 256 x 256": lambda: e.distribution(s, x_ux),
            "b ux 512": lambda: e.distribution(s, ux_1d),
            "c energy_spectrum, log bins only": lambda: e.energy_spectrum(s, n_log=prm["n_log"], log_lo=prm["log_lo"], d_log=prm["d_log"]),
            "d energy_p": lambda: e.energy_p(s),
        }

    full, hollow = calls(sp), calls(empty)
    for group in (full, hollow):                             # warm-up: code objects, the scratch buffers
        for fn in group.values():
            for _ in range(3):
                fn()
    ms = {k: [] for k in full}
    ms0 = {k: [] for k in full}
    for _ in range(args.reps):                               # alternating
        for k in full:
            ms[k].append(timed(full[k])[:2])
            ms0[k].append(timed(hollow[k])[:2])
    stats = {}
    hist = e.distribution(sp, x_ux)
    stats["a x-ux 256 x 256"] = e.distribution_stats()
    hist1 = e.distribution(sp, ux_1d)
    stats["b ux 512"] = e.distribution_stats()
    route_e, same = [], None
    if not args.no_route_e:
        for _ in range(3):
            t0 = time.perf_counter()
            p = e.get_particles(sp)
            t1 = time.perf_counter()
            i = p["i"].astype(np.int64)
            x = (i % (n + 2) - 1).astype(np.float64) + (p["dx"].astype(np.float64) + 1.0) * 0.5
            want, _, _ = np.histogram2d(p["ux"].astype(np.float64), x, bins=(256, 256),
                                        range=((x_ux[1][1], x_ux[1][1] + 256 * x_ux[1][2]), (0.0, float(n))))
            route_e.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        # numpy's bins are found by another arithmetic (and its last bin is closed): totals are compared, bins nearly
        same = (int(want.sum()), int(hist.sum()), int(np.abs(want.astype(np.int64) - hist.astype(np.int64)).sum()))
    e.close()

    lines = [f"phase-space distributions of one species: {n}^3 cells x {ppc} per cell = {np_} particles, tile order, {args.reps} alternating repeats",
             f"device: {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call);",
             "  kernel: that median minus the median of the same call on an empty species (the same clearing, copies and wait, no launch)"]
    med, kern = {}, {}
    for k, v in ms.items():
        ev, host = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        ev0 = np.array([x[0] for x in ms0[k]])
        med[k], kern[k] = float(np.median(ev)), float(np.median(ev) - np.median(ev0))
        extra = ""
        if k in stats:
            s = stats[k]
            extra = f"  seen {s[0]} kept {s[1]} counted {s[2]} through global memory (out[3]) {s[3]}"
        lines.append(f"  ({k}): {np.median(ev):.3f} [{ev.min():.3f} .. {ev.max():.3f}]  (host {np.median(host):.3f})  empty {np.median(ev0):.3f}  kernel {kern[k]:.3f}{extra}")
    if route_e:
        lines.append(f"  (e get_particles + numpy.histogram2d, 3 repeats): download {np.median([c[0] for c in route_e]):.0f} ms + numpy {np.median([c[1] for c in route_e]):.0f} ms;"
                     f" numpy counted {same[0]}, the device {same[1]}, sum of |differences| over the bins {same[2]}")
        lines.append(f"(e) / (a) = {np.median([c[0] + c[1] for c in route_e]) / med['a x-ux 256 x 256']:.0f}")
    ka, kb, kc = kern["a x-ux 256 x 256"], kern["b ux 512"], kern["c energy_spectrum, log bins only"]
    lines.append(f"kernels: (a) / (c) = {ka / kc:.2f} (hoped for: up to 1.5)   (b) / (c) = {kb / kc:.2f} (hoped for: up to 1)")
    lines.append(f"bytes the kernels read: (a) 12 B per particle = {12 * np_ / 1e9:.3f} GB -> {12 * np_ / ka / 1e6:.0f} GB/s; (b) 8 B -> {8 * np_ / kb / 1e6:.0f} GB/s;"
                 f" (c) 16 B -> {16 * np_ / kc / 1e6:.0f} GB/s")
    lines.append(f"x-ux: {int(np.count_nonzero(hist))} of {hist.size} bins populated, fullest {int(hist.max())}; ux: fullest {int(hist1.max())}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
