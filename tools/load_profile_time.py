"""What loading a species on the device from per-cell tables costs (vpic_hip_species_load_profile, csrc/load.hip) beside the
synthetic loader and beside the route it replaces.  One species of BASELINE configs[1] (128^3 cells, 67 M particles) in ONE
process; the calls alternate:
  (a) load_maxwellian, 32 per cell                          (b) load_profile with scalar tables and the same 32 per cell
  (c) load_profile of a z profile of equal weights: counts from 0 to 128 per cell (a triangle over the middle half of the
      box, 32 per cell on average: the same 67 M particles), a drift that turns with z, uth = 0.6
  (d) the same with tags, in a second species (a replacing call without tags into a species that has them clears them)
Every call is timed with events on the engine's stream around it and with the host clock; three warm-up calls each, then
the median of the repeats with their range.
  (e) the route replaced: the numpy build of the same particles (tests/load_ref.py, the restatement of the rule: Philox, the
      normals, the boost) plus set_particles, on the host clock, three repeats.  The build is timed on the two densest
      z planes of (c) and scaled per particle to the species; set_particles is timed whole, on 67 M records.
Bytes a call writes per particle: 32 (the 16-byte position record and four floats), 48 with tags.
No figure is fixed in advance: nobody has measured this pass.
    python tools/load_profile_time.py [--out profiles/load_profile_time.txt] [--reps 20] [--skip-host]        (GPU box)"""
import importlib
import time

import numpy as np

import diag_timing as T


def main():
    import torch
    ap = T.parser(reps=20)
    ap.add_argument("--skip-host", action="store_true", help="leave (e) out (a profiler run)")
    args = ap.parse_args()
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc
    V = importlib.import_module("old-vpic_amd")
    e = V.Engine(V.make_grid(n, n, n, float(n), float(n), float(n), np.float32(0.95 / np.sqrt(3.0))))
    e.set_vacuum()
    sp = e.new_species(-1.0, np_ + 4096, np_ // 8)
    tagged = e.new_species(-1.0, np_ + 4096, np_ // 8)          # (d) in a species of its own: one that loses its tags has them cleared
    stream = torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", 0))
    F = np.float32
    k = np.arange(n)
    # a triangle of height 4 ppc over the middle half of the box: ppc per cell on average
    count = np.clip(4 * ppc - (16 * ppc // n) * np.abs(k - n // 2), 0, 4 * ppc).astype(np.int32).reshape(n, 1, 1)
    assert int(count.sum()) * n * n == np_, "the profile holds as many particles as the uniform load"
    phi = np.pi * k / n
    ud = (F(0.2) * np.cos(phi).astype(F).reshape(n, 1, 1), F(0.2) * np.sin(phi).astype(F).reshape(n, 1, 1), None)
    hot = (F(0.6),) * 3
    loaded = {}

    def profile(name, *a, **kw):
        loaded[name] = e.load_profile(tagged if name == "d" else sp, *a, **kw)

    calls = {"a load_maxwellian": lambda: e.load_maxwellian(sp, ppc, 1, -1.0 / ppc, (0.2, 0.0, 0.0), T.VTH),
             "b load_profile, scalar tables": lambda: profile("b", ppc, F(-1.0 / ppc), (F(0.2), F(0), F(0)), (F(T.VTH),) * 3, seed=1),
             "c load_profile, z profile 0 .. %d per cell, turning drift, uth 0.6" % (4 * ppc): lambda: profile("c", count, F(-1.0 / ppc), ud, hot, seed=1),
             "d the same with tags": lambda: profile("d", count, F(-1.0 / ppc), ud, hot, seed=1, tags=1)}
    ms, _ = T.alternate(stream, args.reps, calls)
    assert loaded == dict(b=np_, c=np_, d=np_), loaded

    host = None
    if not args.skip_host:
        import load_ref as R
        planes = slice(n // 2 - 1, n // 2 + 1)
        build, up = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            slab = R.load((n, n, 2), count[planes], F(-1.0 / ppc), tuple(None if t is None else t[planes] for t in ud), hot, seed=1,
                          global_dims=(n, n, n), offset=(0, 0, n // 2 - 1), tag0=1)[0]
            build.append((time.perf_counter() - t0) * 1e3 * np_ / len(slab))
        p = np.resize(slab, np_)                                # 67 M host records (3.2 GB), as the route would hold them
        p["i"] = np.sort(p["i"])
        for _ in range(3):
            t0 = time.perf_counter()
            e.set_particles(sp, p)
            e.sync()
            up.append((time.perf_counter() - t0) * 1e3)
        host = (float(np.median(build)), float(np.median(up)), len(slab))
    e.close()

    lines = [f"loading one species: {n}^3 cells, {np_} particles, {args.reps} alternating repeats", f"device: {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call)"]
    more, med, _ = T.call_lines(ms)
    lines += more
    a, b, c, d = (med[key] for key in calls)
    lines.append(f"(b) / (a) = {b / a:.2f}   (c) / (a) = {c / a:.2f}   (d) / (c) = {d / c:.2f}   bytes written per particle: (a) (b) (c) 32, (d) 48: 48 / 32 = 1.50")
    lines.append(f"bytes written per second: (a) {32.0 * np_ / (a * 1e-3) / 1e9:.0f} GB/s  (b) {32.0 * np_ / (b * 1e-3) / 1e9:.0f} GB/s  "
                 f"(c) {32.0 * np_ / (c * 1e-3) / 1e9:.0f} GB/s  (d) {48.0 * np_ / (d * 1e-3) / 1e9:.0f} GB/s")
    if host:
        lines.append(f"  (e) the route replaced, host clock, medians of 3: the numpy build (tests/load_ref.py; {host[2]} particles of two z planes timed, scaled "
                     f"to the species) {host[0] / 1e3:.0f} s, set_particles of {np_} records {host[1]:.0f} ms; set_particles alone / (c) = {host[1] / c:.0f}, "
                     f"with the build / (c) = {(host[0] + host[1]) / c:.0f}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
