"""The oracle (oracle/vpic_oracle.c) against the compiled reference on the chain of oracle/field_chain.py: every kind of
field wall (PEC, symmetric, PMC, absorbing) on every face, one axis at a time, mixed with a different kind at each end,
and on all six faces, on twelve grids (axes one cell thick in every position, extents across a wavefront and a tile, planes
of several blocks), with and without damping, vacuum and three materials.  tests/golden/field_walls.npz
(oracle/gen_field_walls.py) holds the reference's SHA-256 per stage and the doubles it returned.  CPU-only.

Per-voxel stages: the same bytes (equal digests).  The three error sums and the six energies: rel 1e-12, the project's
figure for double sums in another order than the reference's per-pipeline partial sums (test_oracle_golden.py)."""
import functools
import os

import numpy as np
import pytest

from oracle import field_chain as FC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_walls.npz")


@functools.lru_cache(maxsize=1)
def fixture():
    assert os.path.exists(FIXTURE), "tests/golden/field_walls.npz is missing (python oracle/gen_field_walls.py)"
    g = np.load(FIXTURE)
    assert list(g["stage_names"]) == FC.STAGE_NAMES, "the chain's stages changed, regenerate tests/golden/field_walls.npz"
    return {k: i for i, k in enumerate(g["keys"])}, g["inputs_sha256"], g["stage_sha256"], g["scalars"]


@functools.lru_cache(maxsize=2)
def inputs(dims, materials):
    return FC.inputs(dims, materials=materials)


def test_fixture_holds_every_run():
    index = fixture()[0]
    keys = [FC.run_key(*r) for r in FC.cpu_runs()]
    assert len(keys) == len(set(keys)) == 532 and set(keys) == set(index)
    assert len(FC.WALLS) == 19 and len(FC.GRIDS) == 12
    # every (kind, face) pair is among the layouts; the mixed ones have a different kind at the two ends of every axis
    for kind in (FC.P, FC.S, FC.M, FC.A):
        for face in range(6):
            assert any(w[face] == kind and w[(face + 3) % 6] == kind for w in FC.ONE_AXIS_WALLS)
    assert all(w[axis] != w[axis + 3] for w in FC.MIXED_WALLS for axis in range(3))


@pytest.mark.parametrize("fbc", FC.WALLS, ids=FC.wall_name)
@pytest.mark.parametrize("dims", FC.GRIDS, ids=FC.grid_name)
def test_oracle_walks_the_chain_as_the_reference_does(orc, dims, fbc):
    index, in_sha, st_sha, scalars = fixture()
    api = FC.orc_api()
    for materials in ((False, True) if dims in FC.MATERIAL_GRIDS else (False,)):
        inp = inputs(dims, materials)
        for damp in FC.DAMPS:
            key = FC.run_key(dims, fbc, damp, materials)
            assert key in index, key + ": not in tests/golden/field_walls.npz, regenerate"
            r = index[key]
            assert FC.inputs_digest(inp) == in_sha[r].tobytes(), key + ": the seeded stream changed, regenerate tests/golden/field_walls.npz"
            d, s, finite, _ = FC.record(api, dims, fbc, damp, materials, inp)
            assert finite, key + ": an oracle output is not finite"
            for k, name in enumerate(FC.STAGE_NAMES):
                assert d[k].tobytes() == st_sha[r][k].tobytes(), (key, name)
            assert np.all(np.abs(s - scalars[r]) <= 1e-12 * np.abs(scalars[r])), (key, s, scalars[r])
