"""TEST INFRASTRUCTURE: the chain of oracle/field_chain.py run by the COMPILED REFERENCE (oracle/_ref/libvpic_ref.so)
for every grid x wall layout x damp of that file, vacuum, and with three materials on two of the grids.  Per run the
fixture holds a SHA-256 of the seeded inputs, one SHA-256 per stage over the bytes of the array the stage wrote (every
named component, padding excluded) and the doubles the chain returns (rms div E error, rms div B error, the tang-E /
norm-B error, six field energies).  Digests and scalars only: the arrays themselves would be hundreds of MB.
-> tests/golden/field_walls.npz.  Needs the reference tree (python oracle/gen_field_walls.py); written with fixed zip
timestamps, so that a second run gives the same file byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import field_chain as FC  # noqa: E402


def main():
    api = FC.ref_api()
    keys, in_sha, st_sha, scalars = [], [], [], []
    cache = {}
    for dims, fbc, damp, materials in FC.cpu_runs():
        if (dims, materials) not in cache:
            cache.clear()
            cache[(dims, materials)] = FC.inputs(dims, materials=materials)
        inp = cache[(dims, materials)]
        d, s, finite, _ = FC.record(api, dims, fbc, damp, materials, inp)
        key = FC.run_key(dims, fbc, damp, materials)
        assert finite, key + ": the reference itself is not finite here"
        keys.append(key)
        in_sha.append(np.frombuffer(FC.inputs_digest(inp), np.uint8))
        st_sha.append(d)
        scalars.append(s)
    out = dict(keys=np.array(keys), stage_names=np.array(FC.STAGE_NAMES), inputs_sha256=np.stack(in_sha),
               stage_sha256=np.stack(st_sha), scalars=np.stack(scalars))
    dst = os.path.join(ROOT, "tests", "golden", "field_walls.npz")
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arr, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(keys), "runs of", len(FC.STAGE_NAMES), "stages")


if __name__ == "__main__":
    main()
