"""What the absorbing walls that tally and record (vpic_hip_wall_*, csrc/particles.hip: boundary_classify_kernel) cost a round
of the particle boundary exchange.  One species of BASELINE configs[1] (128^3 cells, 32 per cell, drift 0.2 c, thermal spread
0.02 c: 67 M particles) in tile order, in a box whose x faces absorb; every repeat pushes the species once (not timed: it
makes the round's movers, some 60 k of them) and times

  legacy    one vpic_hip_boundary_p_pack round                                      (what vpic_hip_step runs)
  resident  one vpic_hip_exchange_pack + vpic_hip_exchange_finish after _exchange_begin and an asynchronous push

in three settings that alternate in ONE run: no wall registered, VPIC_ABSORB_PARTICLES registered to tally, and registered to
tally and record.  Events on the engine's stream around the call; the median of the repeats with their range.

The no-wall round is also timed on the PARENT commit's library (--parent-lib: a libvpic_hip.so built from the parent, loaded
through VPIC_HIP_LIB), in processes of its own that alternate with processes of this commit's library making exactly the same
calls (no vpic_hip_wall_* call at all: between the timed rounds of the three-setting run stand the small copies and waits of
vpic_hip_set_wall and vpic_hip_wall_records, which the parent cannot make), --runs of each: the figure to hold is that
this commit's no-wall round lies within the spread of the parent's own repeats.  No threshold is fixed: nobody has measured
these before.
    python tools/wall_time.py --parent-lib /path/to/parent/libvpic_hip.so [--out profiles/wall_time.txt] [--reps 20] [--runs 3]   (GPU box)"""
import json
import os
import subprocess
import sys

import numpy as np

import diag_timing as T

SETTINGS = ("no wall", "tally", "tally and records")


def child(args):
    """one process: {path: {setting: [event ms] * reps}, "movers": ...} as one JSON line"""
    import importlib
    import torch
    V = importlib.import_module("old-vpic_amd")
    L = V.layout
    n, ppc = args.cells, args.ppc
    np_ = n ** 3 * ppc
    e = V.Engine(V.make_grid(n, n, n, float(n), float(n), float(n), np.float32(0.95 / np.sqrt(3.0)),
                             pbc=[L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0]))
    e.set_vacuum()
    e.set_sort_order("engine")
    sp = e.new_species(-1.0, np_ + 4096, np_ // 8)
    e.load_maxwellian(sp, ppc, 1, -1.0 / ppc, (0.2, 0.0, 0.0), T.VTH)
    e.load_interpolator()
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    stream = torch.cuda.ExternalStream(e.stream(), device=torch.device("cuda", 0))
    walls = hasattr(V.lib(), "vpic_hip_wall_setup") and not args.plain
    settings = SETTINGS if walls else SETTINGS[:1]
    if walls:
        e.wall_setup(2.0 ** -30 / ppc, 2.0 ** -24 / ppc, np_ // 8)

    def setting(name):
        if walls:
            e.set_wall(L.ABSORB_PARTICLES, record=name == "tally and records", tally=name != "no wall")
            e.wall_records(clear=True, cap=0)                        # (the cursor restarts: the buffer never fills)

    out = {"legacy": {k: [] for k in settings}, "resident": {k: [] for k in settings}, "movers": [], "absorbed": 0}
    for rep in range(args.reps + 3):                                 # three warm-up repeats
        for name in settings:
            setting(name)
            e.advance_p(sp)
            e.sync()
            nm = e.nm(sp)
            ms = T.timed(stream, e.boundary_p_pack)[0]
            assert e.nm(sp) == 0
            if rep >= 3:
                out["legacy"][name].append(ms)
                out["movers"].append(nm)
    for rep in range(args.reps + 3):
        for name in settings:
            setting(name)
            e.exchange_begin()
            e.advance_p_async(sp)
            e.sync()

            def round_():
                e.exchange_pack([0] * 6, [0] * 6, 1 << 30)
                e.exchange_finish([])
            ms = T.timed(stream, round_)[0]
            assert e.exchange_flags == 0 and e.nm(sp) == 0
            if rep >= 3:
                out["resident"][name].append(ms)
    if walls:
        out["absorbed"] = int(e.wall_tally().count.sum())
    out["device"] = torch.cuda.get_device_name(0)
    e.close()
    print("WALL_TIME " + json.dumps(out))


def run_child(args, lib, plain):
    env = dict(os.environ)
    if lib:
        env["VPIC_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--cells", str(args.cells), "--ppc", str(args.ppc)]
    if plain:
        cmd.append("--plain")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("WALL_TIME ")][-1][len("WALL_TIME "):])


def stat(v):
    v = np.asarray(v)
    return f"{np.median(v):.4f} [{v.min():.4f} .. {v.max():.4f}]"


def main():
    ap = T.parser(reps=20)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--plain", action="store_true")                  # (a child that never calls vpic_hip_wall_*: what the parent's library can do)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        return child(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: the parent commit's libvpic_hip.so"
    parent, plain, this = [], [], []
    for _ in range(args.runs):                                       # the processes alternate
        parent.append(run_child(args, os.path.abspath(args.parent_lib), True))
        plain.append(run_child(args, None, True))
    for _ in range(args.runs):
        this.append(run_child(args, None, False))
    lines = [f"absorbing walls that tally and record, one round of the particle boundary exchange of one species: {args.cells}^3 cells x {args.ppc} per cell = "
             f"{args.cells ** 3 * args.ppc} particles, tile order, x faces absorbing; {int(np.median(this[0]['movers']))} movers per round (median); "
             f"{args.reps} alternating repeats per process, {args.runs} processes of the parent commit's library alternating with {args.runs} of this commit's that make the same calls, then {args.runs} of this commit's with the three settings in turn",
             f"device: {this[0]['device']}",
             "milliseconds per round between events on the engine's stream: median [min .. max]"]
    for path in ("legacy", "resident"):
        lines.append(f"{path} round ({'boundary_p_pack' if path == 'legacy' else 'exchange_pack + exchange_finish'}):")
        for k, r in enumerate(parent):
            lines.append(f"  parent commit, process {k}, no wall (it has none): {stat(r[path]['no wall'])}")
        for k, r in enumerate(plain):
            lines.append(f"  this commit,   process {k}, no wall, the same calls as the parent's process: {stat(r[path]['no wall'])}")
        for k, r in enumerate(this):
            for name in SETTINGS:
                lines.append(f"  this commit,   process {k}, the three settings in turn, {name}: {stat(r[path][name])}")
        pm = [float(np.median(r[path]["no wall"])) for r in parent]
        tm = [float(np.median(r[path]["no wall"])) for r in plain]
        inside = min(pm) <= float(np.median(tm)) <= max(pm)
        lines.append(f"  no wall: parent medians {min(pm):.4f} .. {max(pm):.4f} (spread of its own repeats), this commit's medians {min(tm):.4f} .. {max(tm):.4f}, "
                     f"median of them {np.median(tm):.4f}: {'within' if inside else 'OUTSIDE'} the parent's spread")
        base = float(np.median([np.median(r[path]["no wall"]) for r in this]))
        for name in SETTINGS[1:]:
            m = float(np.median([np.median(r[path][name]) for r in this]))
            lines.append(f"  {name}: {m:.4f}, {m - base:+.4f} ms on the no-wall round ({m / base:.3f} x)")
    lines.append(f"particles the walls counted in one process of this commit: {this[0]['absorbed']}")
    T.finish(lines, args.out)


if __name__ == "__main__":
    main()
