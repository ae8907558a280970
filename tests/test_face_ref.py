"""The reference world of tests/face_ref.py held to what the golden fixtures already pin on the compiled reference: the
oracle's one-domain synchronize_*_local functions.  CPU only.

  * a 1 x 1 x 1 world run piece by piece IS the _local function (every word, ghosts included, and the same err);
  * on exact inputs every cut world of tests/test_gpu_faces.py equals the gathered one-domain result on every owned word
    (summed families and the averaged ones), and the ghost planes of the copied kinds equal the neighbour's owned plane;
  * every message is exactly `count` floats, `count` is the closed form, and every float of it is written;
  * every input of every case is pairwise different, and the exact ones make err order-free."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import face_ref as R  # noqa: E402
from oracle import pyorc  # noqa: E402

LOCAL = {"jf": lambda a, g: pyorc.synchronize_jf_local(a, g), "rho": lambda a, g: pyorc.synchronize_rho_local(a, g),
         "msg2": lambda a, g: pyorc.synchronize_tang_e_norm_b_local(a, g), "hydro": lambda a, g: pyorc.synchronize_hydro_local(a, g)}
SIZES = [(5, 3, 2), (1, 4, 3), (3, 1, 2), (2, 3, 1), (1, 1, 1), (17, 16, 2)]
ONE_WALLS = [None] + [{a: w} for a in range(3) for w in R.WALLS] + [{0: "pec", 1: "absorb", 2: "symmetric"}]


@pytest.mark.parametrize("walls", ONE_WALLS, ids=lambda w: "-".join(v + "xyz"[k] for k, v in sorted(w.items())) if w else "periodic")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "%dx%dx%d" % n)
def test_one_domain_world_is_the_local_function(n, walls):
    w = R.World((1, 1, 1), n, walls, "general", seed=3)
    d = w.domains[0]
    for fam, local in LOCAL.items():
        w.reset()
        ref = w.array(fam, 0).copy()
        err_ref = local(ref, d.g)
        err = w.run(fam)[0]
        assert not w.msgs, "a one-domain world sends nothing"
        assert np.array_equal(R.words(w.array(fam, 0)), R.words(ref)), (fam, n, walls)
        assert not np.array_equal(R.words(ref), R.words(d.f0 if R.FAMILIES[fam].array == "f" else d.h0)), (fam, "nothing moved")
        if fam == "msg2":
            assert err == err_ref and (err > 0) == (len(walls or {}) < 3), (err, err_ref)


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_cut_world_equals_the_gathered_one_domain_result(gp, n, walls):
    w = R.World(gp, n, walls, "exact", seed=5)
    args, kw = w.one_domain_grid()
    g1 = pyorc.make_grid(*args, **kw)
    for fam, local in LOCAL.items():
        w.reset()
        one = R.gather(w, fam)
        assert np.any(R.words(one)), fam
        local(one, g1)
        w.run(fam)
        assert R.owned_equal(w, fam, one) == 0, (fam, gp, n, walls)


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_ghost_planes_of_the_copied_kinds_are_the_neighbours_planes(gp, n, walls):
    w = R.World(gp, n, walls, "general", seed=6)
    for fam in ("tang_b", "msg0", "msg1"):
        w.reset()
        w.run(fam)
        seen = 0
        for (sender, d) in w.msgs:
            s, r = w.domains[sender], w.domains[w.domains[sender].fbc[d]]
            for comp, src, dst in R.copied_planes(fam, n, d):
                got = R.view3(r.f, comp, n)[R.slab(dst)].view(np.uint32)
                ref = R.view3(s.f0, comp, n)[R.slab(src)].view(np.uint32)
                assert got.size and np.array_equal(got, ref), (fam, sender, d, comp)
                seen += got.size
        assert seen == sum(len(m) for m in w.msgs.values()), (fam, "a float of a message is no ghost word")
        # ... and nothing but ghost words changed: every owned word is the input
        for dom in w.domains:
            for comp in R.FIELD_FLOATS:
                ext = R.extent(n, *R.MESH[comp])
                assert np.array_equal(R.view3(dom.f, comp, n)[R.slab(ext)], R.view3(dom.f0, comp, n)[R.slab(ext)]), (fam, dom.rank, comp)


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_message_sizes_and_coverage(gp, n, walls):
    w = R.World(gp, n, walls, "general", seed=7)
    for fam, F in R.FAMILIES.items():
        for dom in w.domains:
            for d in range(6):
                assert F.count(dom.g, d) == R.closed_count(fam, n, d), (fam, d)
                msg = R.pack(F, w.array(fam, dom.rank), dom.g, d)             # (asserts: count floats, all written, none behind)
                assert len(msg) == R.closed_count(fam, n, d)
                R.assert_distinct(msg.view(np.uint32), (fam, d))              # no voxel is packed twice


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_inputs_are_pairwise_different(gp, n, walls):
    for inputs, seed in (("general", 1), ("exact", 2)):
        w = R.World(gp, n, walls, inputs, seed)
        for name in ("f0", "h0"):
            v = np.concatenate([R.float_words(getattr(d, name)) for d in w.domains])
            R.assert_distinct(v, (inputs, name))
            x = v.view(np.float32).astype(np.float64)
            if inputs == "general":
                assert np.all(np.isfinite(x)) and np.abs(x).min() >= 1e-6 and np.abs(x).max() <= 1e3
                assert np.abs(x).min() < 1e-4 and np.abs(x).max() > 10
            else:
                assert np.all(x * 64 == np.rint(x * 64)) and np.abs(x).max() * 64 == len(x) and (x > 0).any() and (x < 0).any()


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_exact_inputs_make_err_order_free(gp, n, walls):
    """every err the oracle returns on exact inputs is the sum of its squared differences in integers"""
    w = R.World(gp, n, walls, "exact", seed=5)
    F = R.FAMILIES["msg2"]
    checked = 0
    for p in w.schedule("msg2"):
        dom = w.domains[p.rank]
        want = None
        if p.op == "self" and dom.fbc[p.arg] == p.rank and dom.fbc[p.arg + 3] == p.rank:
            lo, hi = R.pack(F, dom.f, dom.g, p.arg), R.pack(F, dom.f, dom.g, p.arg + 3)
            want = R.exact_err(lo, hi, n, p.arg) + R.exact_err(hi, lo, n, p.arg + 3)
            assert want < 2.0 ** 35
        elif p.op == "unpack":
            before = R.pack(F, dom.f, dom.g, (p.arg + 3) % 6)                 # the plane the message lands on
            want = R.exact_err(w.msgs[(p.src, p.arg)], before, n, p.arg)
        err = w.apply("msg2", p)
        if want is None:
            assert err == 0.0
        else:
            assert err == want and err > 0, (p, err, want)
            checked += 1
    assert checked
