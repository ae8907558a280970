"""The three histogram calls share result buffers (csrc/engine.h, HistResult): `distribution` writes its counts where
`distribution_sums` writes its own, each of the three calls keeps statistics of its own, and a later, larger descriptor grows
the buffers under what an earlier call left.  One engine, 4 x 4 x 4 cells, 512 particles: `distribution`, then
`distribution_sums` and `cell_distribution` with other descriptors, and every call's statistics and the first call's
counts are still what they were -- once with the sums in LDS, once with a sums descriptor above the LDS budget, which
grows both of the species' buffers."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from species_states import package  # noqa: E402

pytestmark = pytest.mark.gpu

N_CELLS, PPC = 4, 8
UX_UZ = [("ux", 0.1, 0.025, 16), ("uz", -0.4, 0.05, 16)]                 # 256 bins: in LDS; the faster half of the drift 0.1
VALUES = [(("one",), 1.0), (("ux", "ux"), 1e-6)]
CELLS = ([("z", 0.0, 1.0, N_CELLS)], [(("one",), 1.0)])
# bins * (1 + 2 * 2 values) against the 8192 words of the LDS budget (include/vpic_hip.h)
SUMS_AXES = {"lds": [("ke", 0.0, 0.001, 64)], "global": [("ke", 0.0, 0.00005, 2048)]}


def test_calls_keep_their_own_statistics_and_counts():
    V = package()
    e = V.Engine(V.make_grid(N_CELLS, N_CELLS, N_CELLS, float(N_CELLS), float(N_CELLS), float(N_CELLS), np.float32(0.4)))
    n = N_CELLS ** 3 * PPC
    sp = e.new_species(-1.0, n + 64, 64)
    e.load_maxwellian(sp, PPC, 3, -1.0 / PPC, (0.1, 0.0, 0.0), 0.08)
    assert e.np(sp) == n
    for path, axes in SUMS_AXES.items():
        first = e.distribution(sp, UX_UZ)
        first_stats = e.distribution_stats()
        assert first_stats[0] == n and 0 < first_stats[2] == int(first.sum()) and first_stats[3] == 0, path
        sums = e.distribution_sums(sp, axes, VALUES)
        sums_stats = e.distribution_sums_stats()
        assert sums_stats[0] == n and 0 < sums_stats[2] == int(sums.counts.sum()), path
        assert sums_stats[3] == (0 if path == "lds" else sums_stats[2]), path            # the path meant
        assert np.array_equal(sums.isums[0], sums.counts.astype(np.int64)) and sums.isums[1].sum() > 0, path
        cells = e.cell_distribution(*CELLS)
        cell_stats = e.cell_distribution_stats()
        assert cell_stats[:4] == (N_CELLS ** 3,) * 3 + (0,) and list(cells.counts) == [N_CELLS ** 2] * N_CELLS, path
        assert len({first_stats[:3], sums_stats[:3], cell_stats[:3]}) == 3, path        # three calls that can be told apart
        print(f"{path}: distribution {first_stats}, sums {sums_stats}, cells {cell_stats}")
        assert e.distribution_stats() == first_stats, path
        assert e.distribution_sums_stats() == sums_stats, path
        assert e.cell_distribution_stats() == cell_stats, path
        again = e.distribution(sp, UX_UZ)
        assert again.tobytes() == first.tobytes() and again.shape == first.shape, path
        assert e.distribution_stats() == first_stats and e.distribution_sums_stats() == sums_stats, path
    e.close()
