"""The face messages a domain exchanges with ANOTHER domain (include/vpic_hip.h: vpic_hip_pack_tang_b / _pack_jf / _pack_rho /
_pack_face_message kinds 0, 1, 2 / _pack_hydro, their unpacks, the _local_adjust_* and _synchronize_*_self pieces and the five
count functions) held word for word to the reference world of tests/face_ref.py, which is the oracle's restatement of
remote.c, local.c and hydro.c and is itself held to the pinned one-domain functions by tests/test_face_ref.py.

One process; a world is a few small engines on the one device, a message a torch byte tensor of 4 * count bytes with a guard
of 1024 bytes behind it, all 0xFF before the pack, that one engine packs and its neighbour unpacks.  After EVERY piece call
(tests/face_ref.py: World.schedule, the order of old-vpic_amd/domain.py) every word of the whole array of every domain --
the 16 float components and the material ids of field_t, all 16 words of hydro_t, ghosts and corners included -- equals
the reference world's at the same point, every message equals the reference's float for float, and every byte behind it is
still 0xFF.  All comparisons are `==` on raw 32-bit words: the pieces copy, add with weights 1 and 1, average with weights
1/2 and 1/2 or double, and each of those has one correctly rounded result, so there is nothing for a tolerance to cover.

The one sum whose order differs is the err of kind 2 (the device adds its squared differences, non-negative doubles, with
atomics).  On exact inputs (face_ref: every partial sum is representable) it must equal the oracle's; on general inputs
both sums are within (n - 1) 2^-53, relative, of the true sum of the n squared differences, so they differ by at most
2 (n - 1) 2^-53 err."""
import ctypes as C
import importlib
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

pytestmark = pytest.mark.gpu
L = R.L
GUARD = 1024                   # bytes of guard pattern behind every message
STAGES = ["tang_b", "jf", "rho", "msg0", "msg1", "msg2", "hydro"]


@pytest.fixture(scope="module")
def V():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


class Msg:
    """count floats on the device and GUARD bytes behind them, all 0xFF"""

    def __init__(self, count):
        import torch
        self.count, self.nbytes = int(count), 4 * int(count)
        self.t = torch.full((self.nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr()

    def read(self):
        """(the message as uint32 words, the guard bytes) -- after the engine that wrote has synchronised"""
        b = self.t.cpu().numpy()
        return b[:self.nbytes].view(np.uint32).copy(), b[self.nbytes:].copy()

    def untouched(self):
        return bool(np.all(self.t.cpu().numpy() == 0xFF))


class Dev:
    """one engine per domain of the reference world `w`"""

    def __init__(self, V, w):
        self.w, self.engines, self.msgs = w, [], {}
        try:
            for d in w.domains:
                self.engines.append(V.Engine(V.make_grid(*d.args, **d.kw)))
        except Exception:
            self.close()
            raise

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload(self, fam):
        """the reference world's current arrays of the family onto the engines"""
        self.msgs = {}
        for e, d in zip(self.engines, self.w.domains):
            if R.FAMILIES[fam].array == "f":
                e.set_fields(d.f)
            else:
                e.set_hydro(d.h)

    def array(self, fam, rank):
        e = self.engines[rank]
        return e.get_fields() if R.FAMILIES[fam].array == "f" else e.get_hydro()

    def calls(self, fam, rank):
        """(count, pack, unpack, adjust, self) of the family on the engine of `rank`; unpack and self return err or None"""
        e = self.engines[rank]
        if fam.startswith("msg"):
            k = int(fam[3])
            return (lambda d: e.message_count(k, d), lambda d, p: e.pack_message(k, d, p), lambda d, p: e.unpack_message(k, d, p),
                    e.local_adjust_tang_e_norm_b if k == 2 else None, e.synchronize_tang_e_norm_b_self if k == 2 else None)
        return {"tang_b": (e.face_count, e.pack_tang_b, e.unpack_tang_b, None, None),
                "jf": (e.face_count, e.pack_jf, e.unpack_jf, e.local_adjust_jf, e.synchronize_jf_self),
                "rho": (e.rho_count, e.pack_rho, e.unpack_rho, e.local_adjust_rho, e.synchronize_rho_self),
                "hydro": (e.hydro_count, e.pack_hydro, e.unpack_hydro, e.local_adjust_hydro, e.synchronize_hydro_self)}[fam]

    def apply(self, fam, p):
        """the piece on the device, synchronised; returns its err (0.0 where the piece has none)"""
        e = self.engines[p.rank]
        count, pack, unpack, adjust, self_ = self.calls(fam, p.rank)
        err = None
        if p.op == "adjust":
            adjust()
        elif p.op == "self":
            err = self_(p.arg)
        elif p.op == "pack":
            m = self.msgs[(p.rank, p.arg)] = Msg(count(p.arg))
            pack(p.arg, m.ptr)
        else:
            err = unpack(p.arg, self.msgs[(p.src, p.arg)].ptr)
        e.sync()
        return float(err or 0.0)


def same_words(got, ref, what):
    g, r = R.words(got), R.words(ref)
    assert g.shape == r.shape, what
    bad = np.flatnonzero(g != r)
    if len(bad):
        per = got.dtype.itemsize // 4
        v, k = divmod(int(bad[0]), per)
        raise AssertionError((what, "%d words differ, first at voxel %d word %d: got %08x, reference %08x" % (len(bad), v, k, g[bad[0]], r[bad[0]])))


def err_terms(w, p):
    """how many squared differences piece p of kind 2 adds"""
    d = w.domains[p.rank]
    if p.op == "unpack":
        return R.squared_terms(w.n, p.arg)
    if p.op == "self" and d.fbc[p.arg] == p.rank and d.fbc[p.arg + 3] == p.rank:
        return 2 * R.squared_terms(w.n, p.arg)
    return 0


def run_stage(dev, w, fam, exact_err=False):
    """one stage from freshly uploaded arrays, compared after every piece; returns the number of pieces that had an err"""
    w.reset()
    dev.upload(fam)
    for rank, d in enumerate(w.domains):
        same_words(dev.array(fam, rank), w.array(fam, rank), (fam, "upload", rank))
    with_err = 0
    for p in w.schedule(fam):
        err_ref = w.apply(fam, p)
        err_dev = dev.apply(fam, p)
        if p.op == "pack":
            ref = w.msgs[(p.rank, p.arg)].view(np.uint32)
            m = dev.msgs[(p.rank, p.arg)]
            assert m.count == len(ref) == R.closed_count(fam, w.n, p.arg), (fam, p, m.count, len(ref))
            got, guard = m.read()
            assert np.array_equal(got, ref), (fam, p, "message", int(np.count_nonzero(got != ref)), "of", len(ref), "floats differ")
            assert np.all(guard == 0xFF), (fam, p, "written behind 4 * count")
        for rank in range(len(w.domains)):
            same_words(dev.array(fam, rank), w.array(fam, rank), (fam, tuple(p), "array of rank", rank))
        n = err_terms(w, p) if fam == "msg2" else 0
        if n == 0:
            assert err_dev == 0.0 and err_ref == 0.0, (fam, p, err_dev, err_ref)
        else:
            with_err += 1
            assert err_ref > 0, (fam, p)
            if exact_err:
                assert err_dev == err_ref, (fam, p, err_dev, err_ref)
            else:
                assert abs(err_dev - err_ref) <= 2 * (n - 1) * 2.0 ** -53 * err_ref, (fam, p, err_dev, err_ref, n)
    return with_err


def check_counts(dev, w):
    for e, d in zip(dev.engines, w.domains):
        for k in range(6):
            assert e.face_count(k) == pyorc.tang_b_count(d.g, k) == R.closed_count("jf", w.n, k)
            assert e.rho_count(k) == pyorc.rho_count(d.g, k) == R.closed_count("rho", w.n, k)
            assert e.hydro_count(k) == pyorc.hydro_count(d.g, k) == R.closed_count("hydro", w.n, k)
            for kind in range(3):
                assert e.message_count(kind, k) == pyorc.msg_count(d.g, kind, k) == R.closed_count("msg%d" % kind, w.n, k)


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_every_piece_equals_the_reference_world(V, gp, n, walls):
    """stages 1 to 6 on general inputs: tang_b; jf; rho; kinds 0 and 1; kind 2 with err; hydro"""
    w = R.World(gp, n, walls, "general", seed=11)
    with Dev(V, w) as dev:
        check_counts(dev, w)
        for e, d in zip(dev.engines, w.domains):
            e.set_hydro(d.h0)
        for fam in STAGES:
            if fam == "hydro":                                 # the field stages left hydro alone ...
                last = [d.f.copy() for d in w.domains]
                for rank, d in enumerate(w.domains):
                    same_words(dev.engines[rank].get_hydro(), d.h0, ("hydro after the field stages", rank))
            with_err = run_stage(dev, w, fam)
            assert (with_err > 0) == (fam == "msg2"), fam
        for rank in range(len(w.domains)):                     # ... and the hydro stage the fields
            same_words(dev.engines[rank].get_fields(), last[rank], ("fields after the hydro stage", rank))


@pytest.mark.parametrize("gp,n,walls", R.CASES, ids=R.CASE_IDS)
def test_err_equals_the_oracles_on_exact_inputs(V, gp, n, walls):
    w = R.World(gp, n, walls, "exact", seed=5)
    with Dev(V, w) as dev:
        assert run_stage(dev, w, "msg2", exact_err=True) > 0


# ---- device against device: the cut world gathered == the plain one-domain call (pinned by tests/test_gpu_field_walls.py) ------
@pytest.mark.parametrize("gp,n,walls", R.FAMILY_WORLDS, ids=[R.case_id(*c) for c in R.FAMILY_WORLDS])
def test_cut_world_on_the_device_equals_one_domain_on_the_device(V, gp, n, walls):
    w = R.World(gp, n, walls, "exact", seed=5)
    args, kw = w.one_domain_grid()
    plain = {"jf": lambda e: e.synchronize_jf(), "rho": lambda e: e.synchronize_rho(),
             "msg2": lambda e: e.synchronize_tang_e_norm_b(), "hydro": lambda e: e.synchronize_hydro()}
    with Dev(V, w) as dev:
        one = V.Engine(V.make_grid(*args, **kw))
        try:
            for fam, call in plain.items():
                w.reset()
                dev.upload(fam)
                for p in w.schedule(fam):
                    dev.apply(fam, p)
                got = [dev.array(fam, rank) for rank in range(len(w.domains))]
                start = R.gather(w, fam)                                       # (of the inputs: the reference arrays are untouched)
                if R.FAMILIES[fam].array == "f":
                    one.set_fields(start)
                    call(one)
                    res = one.get_fields()
                else:
                    one.set_hydro(start)
                    call(one)
                    res = one.get_hydro()
                assert not np.array_equal(R.words(res), R.words(start)), (fam, "the one-domain call moved nothing")
                assert R.owned_equal(w, fam, res, got) == 0, (fam, gp, n, walls)
        finally:
            one.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_touch_nothing(V):
    """every pack / unpack entry point with dir -1 and 6, kind -1 and 3, a null buffer, a null err for kind 2; every _self
    piece with axis -1 and 3: an error return with vpic_hip_last_error set, every array bit for bit as it was, the message
    buffer untouched, and the engine usable afterwards.  The count functions: vpic_hip_face_count answers 0, the others -1."""
    w = R.World((1, 1, 1), (5, 3, 2), None, "general", seed=13)
    d = w.domains[0]
    lib = V.lib()
    with Dev(V, w) as dev:
        e = dev.engines[0]
        e.set_fields(d.f)
        e.set_hydro(d.h)
        h = e._h
        m = Msg(max(R.closed_count(f, w.n, k) for f in R.FAMILIES for k in range(6)))
        buf, err = C.c_void_p(m.ptr), C.c_double(-1.0)
        calls = []
        for name in ("pack_tang_b", "unpack_tang_b", "pack_jf", "unpack_jf", "pack_rho", "unpack_rho", "pack_hydro", "unpack_hydro"):
            fn = getattr(lib, "vpic_hip_" + name)
            calls += [(name, k, lambda fn=fn, k=k: fn(h, k, buf)) for k in (-1, 6)]
            calls += [(name, "null buffer", lambda fn=fn: fn(h, 0, None))]
        for kind, k in ((-1, 0), (3, 0), (0, -1), (0, 6), (1, -1), (1, 6), (2, -1), (2, 6)):
            calls += [("pack_face_message", (kind, k), lambda kind=kind, k=k: lib.vpic_hip_pack_face_message(h, kind, k, buf)),
                      ("unpack_face_message", (kind, k), lambda kind=kind, k=k: lib.vpic_hip_unpack_face_message(h, kind, k, buf, C.byref(err)))]
        for kind in range(3):
            calls += [("pack_face_message", (kind, "null buffer"), lambda kind=kind: lib.vpic_hip_pack_face_message(h, kind, 0, None)),
                      ("unpack_face_message", (kind, "null buffer"), lambda kind=kind: lib.vpic_hip_unpack_face_message(h, kind, 0, None, C.byref(err)))]
        calls += [("unpack_face_message", "kind 2, null err", lambda: lib.vpic_hip_unpack_face_message(h, 2, 0, buf, None))]
        for axis in (-1, 3):
            calls += [("synchronize_jf_self", axis, lambda a=axis: lib.vpic_hip_synchronize_jf_self(h, a)),
                      ("synchronize_rho_self", axis, lambda a=axis: lib.vpic_hip_synchronize_rho_self(h, a)),
                      ("synchronize_hydro_self", axis, lambda a=axis: lib.vpic_hip_synchronize_hydro_self(h, a)),
                      ("synchronize_tang_e_norm_b_self", axis, lambda a=axis: lib.vpic_hip_synchronize_tang_e_norm_b_self(h, a, C.byref(err)))]
        calls += [("synchronize_tang_e_norm_b_self", "null err", lambda: lib.vpic_hip_synchronize_tang_e_norm_b_self(h, 0, None))]
        for name, arg, call in calls:
            rc = call()
            e.sync()
            assert rc != 0, (name, arg, "accepted")
            assert b"ad " in lib.vpic_hip_last_error(), (name, arg, lib.vpic_hip_last_error())
            assert err.value == -1.0, (name, arg, "err written")
            same_words(e.get_fields(), d.f, (name, arg, "fields"))
            same_words(e.get_hydro(), d.h, (name, arg, "hydro"))
            assert m.untouched(), (name, arg, "buffer written")
        for k in (-1, 6):
            assert e.face_count(k) == 0                       # (the ABI as it is)
            assert e.rho_count(k) == -1 and e.hydro_count(k) == -1
            assert all(e.message_count(kind, k) == -1 for kind in range(3))
        assert all(e.message_count(kind, 0) == -1 for kind in (-1, 3))
        # the engine is as usable as before: a valid pack and unpack of every family still answer the reference
        for fam in STAGES:
            w.reset()
            dev.upload(fam)
            for k in (0, 4):
                for p in (R.Piece("pack", 0, k, None), R.Piece("unpack", 0, k, 0)):
                    err_ref, err_dev = w.apply(fam, p), dev.apply(fam, p)
                    got, guard = dev.msgs[(0, k)].read()
                    assert np.array_equal(got, w.msgs[(0, k)].view(np.uint32)) and np.all(guard == 0xFF), (fam, p)
                    same_words(dev.array(fam, 0), w.array(fam, 0), (fam, tuple(p), "after the refused calls"))
                    assert (err_ref > 0) == (fam == "msg2" and p.op == "unpack") and abs(err_dev - err_ref) <= 2.0 ** -40 * err_ref, (fam, p)
