"""What the energy spectrum of a species costs (vpic_hip_energy_spectrum, csrc/spectrum.hip) beside the two things a user
had before it.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread 0.02 c) in
tile order, in ONE process:
  (a) energy_p: the closest existing full pass over a species (32 B per particle and the interpolator)
  (b) energy_spectrum with the production deck's parameters (nex = 6, emax = 300, nbin = 800): 16 B per particle
  (c) get_particles and the numpy restatement of tests/test_spectrum_ref.py: the only route there was
(a) and (b) alternate, timed with events on the engine's stream around each call (every call ends in a
synchronisation of that stream, so the host clock around it is given too); medians and the spread over the repeats.
    python tools/spectrum_time.py [--out profiles/spectrum_time.txt] [--reps 20]        (GPU box)"""
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
    ap.add_argument("--no-route-c", action="store_true", help="leave (c) out (runs under a profiler)")
    args = ap.parse_args()
    import torch
    from test_spectrum_ref import deck_params, spectrum_ref
    V = importlib.import_module("old-vpic_amd")
    n, ppc, vth = args.cells, args.ppc, 0.02
    e = V.Engine(V.make_grid(n, n, n, float(n), float(n), float(n), np.float32(0.95 / np.sqrt(3.0))))
    e.set_vacuum()
    e.set_sort_order("engine")
    np_ = n ** 3 * ppc
    sp = e.new_species(-1.0, np_ + 4096, np_ // 8)
    e.load_maxwellian(sp, ppc, 1, -1.0 / ppc, (0.2, 0.0, 0.0), vth)
    e.load_interpolator()
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    prm = deck_params(vth)
    stream = torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", 0))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    calls = {
        "a energy_p": lambda: e.energy_p(sp),
        "b energy_spectrum (bands and log bins)": lambda: e.energy_spectrum(sp, **prm),
        "b' linear bands only": lambda: e.energy_spectrum(sp, n_lin=prm["n_lin"], d_lin=prm["d_lin"]),
        "b'' log bins only": lambda: e.energy_spectrum(sp, n_log=prm["n_log"], log_lo=prm["log_lo"], d_log=prm["d_log"]),
    }
    for fn in calls.values():                                # warm-up: code objects, the scratch buffers
        for _ in range(3):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                               # alternating
        for k, fn in calls.items():
            ms[k].append(timed(fn)[:2])
    lin, log = e.energy_spectrum(sp, **prm)
    counted, misses = e.energy_spectrum_stats()
    route_c = []
    for _ in range(1 if args.no_route_c else 3):
        t0 = time.perf_counter()
        p = e.get_particles(sp)
        t1 = time.perf_counter()
        want = spectrum_ref(np.stack([p["ux"], p["uy"], p["uz"]], axis=1), p["i"], e.nv, prm)
        route_c.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    same = bool(np.array_equal(want[0], lin) and np.array_equal(want[1], log))
    e.close()

    lines = [f"energy spectrum of one species: {n}^3 cells x {ppc} per cell = {np_} particles, tile order, {args.reps} alternating repeats",
             f"device: {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call)"]
    med = {}
    for k, v in ms.items():
        ev, host = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        med[k] = float(np.median(ev))
        lines.append(f"  ({k}): {np.median(ev):.3f} [{ev.min():.3f} .. {ev.max():.3f}]  (host {np.median(host):.3f})")
    a, b = med["a energy_p"], med["b energy_spectrum (bands and log bins)"]
    lines.append(f"  (c get_particles + numpy restatement, 3 repeats): download {np.median([c[0] for c in route_c]):.0f} ms + numpy {np.median([c[1] for c in route_c]):.0f} ms")
    lines.append(f"(b) / (a) = {b / a:.2f}   (expected <= 1, allowed up to 1.5)")
    lines.append(f"(c) / (b) = {(np.median([c[0] + c[1] for c in route_c])) / b:.0f}")
    lines.append(f"bytes the algorithm needs: (a) 32 B per particle + 80 B per voxel = {(32 * np_ + 80 * (n + 2) ** 3) / 1e9:.3f} GB -> {(32 * np_ + 80 * (n + 2) ** 3) / a / 1e6:.0f} GB/s;"
                 f" (b) 16 B per particle = {16 * np_ / 1e9:.3f} GB -> {16 * np_ / b / 1e6:.0f} GB/s (whole call: counters cleared, read back and waited for)")
    lines.append(f"particles counted {counted}, window misses {misses}; counts equal the numpy restatement: {same}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert same


if __name__ == "__main__":
    main()
