"""What a cell distribution costs (vpic_hip_cell_distribution, csrc/cell_dist.hip) beside energy_f, the existing streaming
reduction over six of the same arrays, and beside the route it replaces.  The grid of BASELINE configs[2] (256^3 cells)
with seeded values in every component of the field array, in ONE process, the calls alternating:
  (a) the profile along z (256 bins) of one raw word, cbx: 4 B per cell read; counts and sums in LDS
  (b) the profile along z of e_c, b_c, e_par_c and jdote_c: all six centred fields and the centred current, nine component
      arrays, 36 B per cell (their neighbour words come through the caches); LDS
  (c) the map over x and z, 256 x 256 bins, of cbx: above the LDS budget, every cell adds in global memory
  (d) energy_f: six component arrays, 24 B per cell
  (e) get_fields + numpy, the four sums of (b) in float64: the route replaced (80 B per voxel to the host), twice
Every call is timed with the host clock, and with events on the engine's stream around it; the KERNEL alone is given as
events around the call minus events around the same call on a 2 x 2 x 2 grid in the same process (the same clearing, copies
and wait, a launch of one workgroup).
    python tools/cell_dist_time.py [--out profiles/cell_dist_time.txt] [--reps 20] [--cells 256] [--no-route]        (GPU box)"""
import importlib
import time

import numpy as np

import diag_timing as T


def seeded_fields(V, n, seed=7):
    nv = (n + 2) ** 3
    rng = np.random.default_rng(seed)
    f = np.zeros(nv, V.layout.field_t)
    for name in ("ex", "ey", "ez", "cbx", "cby", "cbz", "jfx", "jfy", "jfz", "rhof", "rhob", "tcax", "tcay", "tcaz", "div_e_err", "div_b_err"):
        f[name] = rng.random(nv, dtype=np.float32) - np.float32(0.5)
    f["cbx"] += np.float32(0.5)
    return f


def main():
    import torch
    ap = T.parser(reps=20)
    ap.set_defaults(cells=256)
    ap.add_argument("--no-route", action="store_true", help="leave (e) out (runs under a profiler)")
    args = ap.parse_args()
    n = args.cells
    cells = n ** 3
    V = importlib.import_module("old-vpic_amd")
    engines = {}
    for name, m in (("full", n), ("small", 2)):
        e = V.Engine(V.make_grid(m, m, m, float(m), float(m), float(m), np.float32(0.95 / np.sqrt(3.0))))
        e.set_vacuum()
        e.set_fields(seeded_fields(V, m))
        engines[name] = (e, torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", 0)))
    q = 2.0 ** -24
    prof_one = ([("z", 0.0, 1.0, n)], [(("cbx",), q)])
    prof_all = ([("z", 0.0, 1.0, n)], [(("e_c",), q), (("b_c",), q), (("e_par_c",), q), (("jdote_c",), q)])
    map2d = ([("x", 0.0, 1.0, n), ("z", 0.0, 1.0, n)], [(("cbx",), q)])
    shapes = {"a profile z, cbx": prof_one, "b profile z, e_c b_c e_par_c jdote_c": prof_all, "c map x-z, cbx": map2d}

    def calls(e):
        c = {}
        for name, (axes, values) in shapes.items():
            c[name] = lambda axes=axes, values=values: e.cell_distribution(axes, values)   # (the small grid keeps the bins: the same clearing and copies)
        c["d energy_f"] = e.energy_f
        return c

    full, small = calls(engines["full"][0]), calls(engines["small"][0])
    for group in (full, small):
        for fn in group.values():
            for _ in range(3):
                fn()
    ms, ms0 = {k: [] for k in full}, {k: [] for k in full}
    for _ in range(args.reps):
        for k in full:
            ms[k].append(T.timed(engines["full"][1], full[k])[:2])
            ms0[k].append(T.timed(engines["small"][1], small[k])[:2])
    e = engines["full"][0]
    extras, results = {}, {}
    for name, (axes, values) in shapes.items():
        results[name] = e.cell_distribution(axes, values)
        s = e.cell_distribution_stats()
        extras[name] = f"  seen {s[0]} kept {s[1]} counted {s[2]} through global memory {s[3]} refused {list(s[4:4 + len(values)])}"
    route = []
    if not args.no_route:
        sy, sz = n + 2, (n + 2) ** 2
        for _ in range(2):
            t0 = time.perf_counter()
            f = e.get_fields()
            t1 = time.perf_counter()
            iz, iy, ix = np.meshgrid(np.arange(1, n + 1), np.arange(1, n + 1), np.arange(1, n + 1), indexing="ij")
            v = (ix + sy * iy + sz * iz).ravel()

            def four(a, s1, s2):
                a = np.ascontiguousarray(a)
                return (np.float32(0.25) * ((a[v + s1 + s2] + a[v]) + (a[v + s1] + a[v + s2]))).astype(np.float64)

            def two(a, s):
                a = np.ascontiguousarray(a)
                return (np.float32(0.5) * (a[v + s] + a[v])).astype(np.float64)

            ex, ey, ez = four(f["ex"], sy, sz), four(f["ey"], sz, 1), four(f["ez"], 1, sy)
            jx, jy, jz = four(f["jfx"], sy, sz), four(f["jfy"], sz, 1), four(f["jfz"], 1, sy)
            bx, by, bz = two(f["cbx"], 1), two(f["cby"], sy), two(f["cbz"], sz)
            b = np.sqrt((bx * bx + by * by) + bz * bz)
            vals = (np.sqrt((ex * ex + ey * ey) + ez * ez), b, ((ex * bx + ey * by) + ez * bz) / b, (jx * ex + jy * ey) + jz * ez)
            want = [w.reshape(n, n * n).sum(axis=1) for w in vals]
            t2 = time.perf_counter()
            got = results["b profile z, e_c b_c e_par_c jdote_c"].sums
            worst = [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, want)]
            route.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, worst))
            del f, v, ix, iy, iz, vals
    for eng, _ in engines.values():
        eng.close()

    lines = [f"cell distributions over a grid of {n}^3 = {cells} cells, {args.reps} alternating repeats", f"device: {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call);",
             "  kernel: that median minus the median of the same call on a 2 x 2 x 2 grid (the same clearing, copies and wait, one workgroup)"]
    more, med, kern = T.call_lines(ms, ms0, "kernel", extras)
    lines += more
    ka, kb, kc, kd = (kern[k] for k in full)
    per_byte = {"a": ka / 4, "b": kb / 36, "c": kc / 4, "d": kd / 24}
    lines.append(f"bytes read: (a) 4 B per cell = {4 * cells / 1e9:.3f} GB -> {4 * cells / ka / 1e6:.0f} GB/s; (b) 36 B -> {36 * cells / kb / 1e6:.0f} GB/s; "
                 f"(c) 4 B -> {4 * cells / kc / 1e6:.0f} GB/s; (d) energy_f 24 B -> {24 * cells / kd / 1e6:.0f} GB/s")
    lines.append(f"(b) / (d): kernels {kb / kd:.2f}, calls {med['b profile z, e_c b_c e_par_c jdote_c'] / med['d energy_f']:.2f}; "
                 f"per byte read {per_byte['b'] / per_byte['d']:.2f}")
    if route:
        down, host, worst = route[-1]
        lines.append(f"  (e get_fields + numpy, the four sums of (b), the second of two): get_fields {down:.0f} ms + numpy {host:.0f} ms "
                     f"(the first: {route[0][0]:.0f} + {route[0][1]:.0f}); largest |device sum - numpy's float sum| over the bins, relative to the "
                     f"largest bin: {', '.join(f'{w:.1e}' for w in worst)}")
        lines.append(f"(e) / (b) = {(down + host) / med['b profile z, e_c b_c e_par_c jdote_c']:.0f}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
