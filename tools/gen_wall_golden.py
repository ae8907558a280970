#!/usr/bin/env python3
"""tests/golden/wall_probe.npz: what the REFERENCE makes of tests/decks/wall_probe.cxx -- the absorb_tally and link_boundary
handlers it ships (src/boundary/absorb_tally.c, link.c) on the x faces of a small box.

The deck is built against the reference with the existing recipe (make -C oracle deck DECK=... OUT=wall_probe; nothing
under oracle/ changes) and run on the CPU in a scratch directory.  Stored, data the reference wrote and nothing else:

  steps    int64[13, 6]   per printed step: step, nabs[0], nabs[1], n_out, np of "light", np of "heavy"
  header   bytes          the first line of link.0
  lines    bytes[n]       the other lines of link.0, sorted

The file is written with fixed time stamps, so that the same run gives the same bytes (tests/test_wall_golden.py).

  python tools/gen_wall_golden.py [--out tests/golden/wall_probe.npz]"""
import argparse
import io
import os
import re
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "decks", "wall_probe.cxx")
STEP = re.compile(r"wall_probe: step (\d+) nabs (-?\d+) (-?\d+) n_out (\d+) np (\d+) (\d+)")


def parse_steps(stdout):
    """int64[n, 6] of the deck's printed lines"""
    return np.array([[int(v) for v in m] for m in STEP.findall(stdout)], np.int64).reshape(-1, 6)


def parse_link(path):
    """(header line, the other lines sorted) of a link file, as bytes with their newlines"""
    with open(path, "rb") as f:
        rows = f.read().splitlines(keepends=True)
    return rows[0], np.array(sorted(rows[1:]), dtype="S")


def run_reference(workdir):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "deck", "DECK=" + DECK, "OUT=wall_probe"],
                          stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "oracle", "_ref", "wall_probe.exe")
    r = subprocess.run([exe, "-tpp=1"], cwd=workdir, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    header, lines = parse_link(os.path.join(workdir, "link.0"))
    return dict(steps=parse_steps(r.stdout), header=np.frombuffer(header, np.uint8), lines=lines)


def fixture_bytes(arrays):
    """an .npz of the arrays with fixed time stamps, uncompressed members in name order"""
    out = io.BytesIO()
    with zipfile.ZipFile(out, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue())
    return out.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wall_probe.npz"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        data = fixture_bytes(run_reference(d))
    with open(a.out, "wb") as f:
        f.write(data)
    g = np.load(a.out)
    print("%s: %d bytes, %d steps, %d link lines, last step %s" % (a.out, len(data), len(g["steps"]), len(g["lines"]), g["steps"][-1].tolist()))


if __name__ == "__main__":
    sys.exit(main())
