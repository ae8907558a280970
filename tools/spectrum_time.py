"""What the energy spectrum of a species costs (vpic_hip_energy_spectrum, csrc/spectrum.hip) beside the two things a user
had before it.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread 0.02 c) in
tile order, in ONE process:
  (a) energy_p: the closest existing full pass over a species (32 B per particle and the interpolator)
  (b) energy_spectrum with the production deck's parameters (nex = 6, emax = 300, nbin = 800): 16 B per particle
  (c) get_particles and the numpy restatement of tests/test_spectrum_ref.py: the only route there was
(a) and (b) alternate, timed with events on the engine's stream around each call (every call ends in a
synchronisation of that stream, so the host clock around it is given too); medians and the spread over the repeats.
    python tools/spectrum_time.py [--out profiles/spectrum_time.txt] [--reps 20]        (GPU box)"""
import numpy as np

import diag_timing as T


def main():
    ap = T.parser(reps=20)
    ap.add_argument("--no-route-c", action="store_true", help="leave (c) out (runs under a profiler)")
    args = ap.parse_args()
    from test_spectrum_ref import deck_params, spectrum_ref
    n, ppc, vth = args.cells, args.ppc, T.VTH
    np_ = n ** 3 * ppc
    V, e, sp, _, stream = T.species(args)
    prm = deck_params(vth)

    calls = {
        "a energy_p": lambda: e.energy_p(sp),
        "b energy_spectrum (bands and log bins)": lambda: e.energy_spectrum(sp, **prm),
        "b' linear bands only": lambda: e.energy_spectrum(sp, n_lin=prm["n_lin"], d_lin=prm["d_lin"]),
        "b'' log bins only": lambda: e.energy_spectrum(sp, n_log=prm["n_log"], log_lo=prm["log_lo"], d_log=prm["d_log"]),
    }
    ms, _ = T.alternate(stream, args.reps, calls)
    lin, log = e.energy_spectrum(sp, **prm)
    counted, misses = e.energy_spectrum_stats()
    route_c, want = T.host_route(e, sp, 1 if args.no_route_c else 3,
                                 lambda p: spectrum_ref(np.stack([p["ux"], p["uy"], p["uz"]], axis=1), p["i"], e.nv, prm))
    same = bool(np.array_equal(want[0], lin) and np.array_equal(want[1], log))
    e.close()

    lines = T.header("energy spectrum", args)
    lines.append("milliseconds per call: median [min .. max] between events on the engine's stream; (median of the host clock around the call)")
    more, med, _ = T.call_lines(ms)
    lines += more
    a, b = med["a energy_p"], med["b energy_spectrum (bands and log bins)"]
    lines.append(f"  (c get_particles + numpy restatement, 3 repeats): download {np.median([c[0] for c in route_c]):.0f} ms + numpy {np.median([c[1] for c in route_c]):.0f} ms")
    lines.append(f"(b) / (a) = {b / a:.2f}   (expected <= 1, allowed up to 1.5)")
    lines.append(f"(c) / (b) = {(np.median([c[0] + c[1] for c in route_c])) / b:.0f}")
    lines.append(f"bytes the algorithm needs: (a) 32 B per particle + 80 B per voxel = {(32 * np_ + 80 * (n + 2) ** 3) / 1e9:.3f} GB -> {(32 * np_ + 80 * (n + 2) ** 3) / a / 1e6:.0f} GB/s;"
                 f" (b) 16 B per particle = {16 * np_ / 1e9:.3f} GB -> {16 * np_ / b / 1e6:.0f} GB/s (whole call: counters cleared, read back and waited for)")
    lines.append(f"particles counted {counted}, window misses {misses}; counts equal the numpy restatement: {same}")
    T.finish(lines, args.out)
    assert same


if __name__ == "__main__":
    main()
