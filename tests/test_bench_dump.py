"""bench.py --dump-outputs on a stand-in engine (no GPU): every file has the same shape and, up to float rounding, the same
values whatever the order of the particle array (the float atomics' order on the device), and all of them stay within
64 MB."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class FakeEngine:
    """What dump_outputs reads of an Engine, over host arrays: 2 species with ppc particles in every cell, in an array order
    drawn from `order_seed`; its hydro moments are per-voxel sums over the particles."""

    def __init__(self, nx, ny, nz, ppc, order_seed):
        L = importlib.import_module("old-vpic_amd.layout")
        E = importlib.import_module("old-vpic_amd.engine")
        self.L = L
        self.grid = E.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), 0.5)
        self.nv = L.nv(nx, ny, nz)
        self.f = np.zeros(self.nv, L.field_t)
        for k, c in enumerate(("ex", "cby", "jfz")):
            self.f[c] = np.random.default_rng(k).standard_normal(self.nv)
        x, y, z = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1), indexing="ij")
        cells = L.voxel(x.ravel(), y.ravel(), z.ravel(), nx, ny, nz)
        self.species = []
        for sp in range(2):
            p = np.zeros(len(cells) * ppc, L.particle_t)
            p["i"] = np.repeat(cells, ppc)
            rng = np.random.default_rng(10 + sp)
            for n in ("dx", "dy", "dz", "ux", "uy", "uz"):
                p[n] = rng.uniform(-1, 1, len(p))
            p["q"] = -1.0
            self.species.append(p[np.random.default_rng(order_seed + sp).permutation(len(p))])
        self.h = None

    def get_fields(self):
        return self.f.copy()

    def np(self, sp):
        return len(self.species[sp])

    def energy_p(self, sp):
        return float(np.sum(self.species[sp]["ux"].astype(np.float64) ** 2))

    def clear_hydro(self):
        self.h = np.zeros(self.nv, self.L.hydro_t)

    def accumulate_hydro_p(self, sp):
        p = self.species[sp]
        for h, c in (("rho", "q"), ("px", "ux"), ("py", "uy"), ("pz", "uz")):
            self.h[h] += np.bincount(p["i"], weights=p[c], minlength=self.nv).astype(np.float32)

    def synchronize_hydro(self):
        pass

    def get_hydro(self):
        return self.h.copy()


@pytest.mark.parametrize("dims", [(9, 8, 6, 3), (64, 64, 32, 40)])
def test_dump_outputs_do_not_depend_on_the_particle_order(tmp_path, dims):
    bench = importlib.import_module("bench")
    deck = dict(species=[None, None])
    for k, seed in enumerate((1, 2)):
        bench.dump_outputs(FakeEngine(*dims, order_seed=seed), deck, str(tmp_path / str(k)))
    names = sorted(os.listdir(tmp_path / "0"))
    assert names == ["fields.npy", "hydro0.npy", "hydro1.npy", "species_summary.npy"]
    nx, ny, nz, ppc = dims
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "0" / name), np.load(tmp_path / "1" / name)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and a.size > 0, name
        total += a.nbytes
        if name == "fields.npy":
            assert a.shape == (min(nx * ny * nz, len(a)), len(bench.DUMP_FIELDS)) and np.array_equal(a, b)
        elif name.startswith("hydro"):
            assert a.shape == (len(np.load(tmp_path / "0" / "fields.npy")), len(bench.DUMP_HYDRO))
            assert np.any(a != 0)
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5 * np.abs(a).max())
        else:
            np.testing.assert_allclose(a, b, rtol=1e-12)
    assert total <= 64 << 20
