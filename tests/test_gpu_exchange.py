"""The device-resident particle exchange (include/vpic_hip.h: vpic_hip_exchange_begin / _pack / _pack_species / _inject /
_finish, the phased push around them, and the host-count path _boundary_p_pack / _inject) held record by record to the
reference world of tests/exchange_ref.py, which is the oracle's restatement of boundary_p.c.

One process, two engines on the one device (the two domains of a world); a message is a torch byte tensor on the device
that one engine packs and the other injects.  Every message is filled with 0xFF before it is packed and has a guard region
of the same pattern behind it (as floats the pattern is a NaN, as a species id it is -1, which the injection skips).
Particles and injector records have no identity but their bits -- arrivals come in untagged -- so everything is compared as
multisets of raw words; the CPU file tests/test_exchange_ref.py proves that the inputs of every case are pairwise different
and contain what the case is named after.

The float accumulator is held to the project's stated bound (2e-6 of the largest entry: test_gpu_tiles.acc_close), the
deterministic one to pyorc.finalize of the exact sums word for word, rhob to the rounding bound of a float sum in another
order (exchange_ref.rhob_bound)."""
import ctypes as C
import functools
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

import det_exact as X  # noqa: E402
import exchange_ref as R  # noqa: E402
import moments_exact as M  # noqa: E402
from oracle import pyorc  # noqa: E402
from test_gpu_tiles import ACC_TOL, acc_close, tile_key  # noqa: E402

pytestmark = pytest.mark.gpu
L = R.L
GUARD = 1024                   # bytes of guard pattern behind every message
WIDE = 1 << 20                 # a mover capacity no list of these tests reaches
ORDERS = ["voxel", "tile"]
KNOBS = ("VPIC_HIP_WINDOW", "VPIC_HIP_TAIL_SORT_MIN")


def package():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


@pytest.fixture(scope="module")
def V():
    return package()


class knobs:
    """environment knobs the engine reads when it is created, restored on the way out"""

    def __init__(self, order, **more):
        self.want = dict(more)
        if order == "tile":
            self.want["VPIC_HIP_WINDOW"] = "tile"            # grids thinner than a tile take the tile order only when told to

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.want)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- messages ----------------------------------------------------------------------------------------------------------------
class Msg:
    """{int32 header[4]; injector payload[cap]} on the device, and GUARD bytes behind it, all 0xFF"""

    def __init__(self, cap):
        import torch
        self.cap, self.nbytes = int(cap), 16 + 48 * int(cap)
        self.t = torch.full((self.nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr()

    def read(self):
        """(header int32[4], payload injector_t[cap], the guard bytes) -- after the engine that wrote has synchronised"""
        b = self.t.cpu().numpy()
        return b[:16].view(np.int32).copy(), b[16:self.nbytes].view(L.particle_injector_t).copy(), b[self.nbytes:].copy()

    def write(self, header, records):
        import torch
        r = np.ascontiguousarray(records, L.particle_injector_t)
        assert len(r) <= self.cap
        b = np.full(self.nbytes + GUARD, 0xFF, np.uint8)
        b[:16] = np.asarray(header, np.int32).view(np.uint8)
        b[16:16 + 48 * len(r)] = r.view(np.uint8)
        self.t.copy_(torch.from_numpy(b))
        torch.cuda.synchronize()
        return self

    def check(self, count, wanted, ref, what):
        """header {count, wanted, 0, 0}; payload [0, count) is the multiset `ref` (or, when ref holds more, a sub-multiset of
        it); every byte behind record `count` -- the rest of the payload and the guard -- still 0xFF"""
        header, payload, guard = self.read()
        assert list(header) == [count, wanted, 0, 0], (what, list(header), count, wanted)
        if len(ref) == count:
            assert R.same_multiset(payload[:count], ref, R.INJ_WORDS), what
        else:
            assert R.sub_multiset(payload[:count], ref, R.INJ_WORDS), what
        assert np.all(payload[count:].view(np.uint8) == 0xFF), (what, "payload written behind the count")
        assert np.all(guard == 0xFF), (what, "written at or behind 16 + 48 cap")
        return payload[:count]

    def untouched(self):
        return bool(np.all(self.t.cpu().numpy() == 0xFF))


def device_records(records):
    """injector records in a device tensor (the caller keeps it alive); returns (tensor, pointer)"""
    import torch
    r = np.ascontiguousarray(records, L.particle_injector_t)
    t = torch.from_numpy(r.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


# ---- the engines of a world ----------------------------------------------------------------------------------------------------
class Dev:
    """One engine per domain of the reference world `w`, holding the same species with the same particles.  order: "voxel"
    (the reference's) or "tile" (the engine's), or None to leave the arrays as uploaded; mode "float" / "deterministic"."""

    def __init__(self, V, w, order="voxel", mode="float", q_ref=X.Q0, max_np=None, max_nm=None):
        self.w, self.order, self.engines = w, order, []
        for d in w.domains:
            e = V.Engine(V.make_grid(*d.args, **d.kw))
            self.engines.append(e)
            e.set_interpolator(d.fi)
            if order == "tile":
                e.set_sort_order("engine")
            if mode == "deterministic":
                e.set_accumulation("deterministic", q_ref)
            for k, s in enumerate(d.species):
                sp = e.new_species(s["q_m"], max_np or len(s["p"]), max_nm or len(s["pm"]))
                assert sp == k
                if s["np"]:
                    e.set_particles(sp, s["p"][:s["np"]])
                    if order:
                        e.sort_p(sp)
                        assert e.species_order(sp) == order

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def n_species(self, rank):
        return len(self.w.domains[rank].species)

    def begin(self, clear=False):
        for e in self.engines:
            if clear:
                e.clear_accumulators()
            e.exchange_begin()

    def push(self):
        for rank, e in enumerate(self.engines):
            for sp in range(self.n_species(rank)):
                e.advance_p_async(sp)

    def pack(self, rank, caps, mover_cap=WIDE, species=None):
        """a fresh message per face with caps[f] > 0 (None for the others), packed and synchronised"""
        e = self.engines[rank]
        msgs = [Msg(c) if c > 0 else None for c in caps]
        e.exchange_pack([m.ptr if m else 0 for m in msgs], [m.cap if m else 0 for m in msgs], mover_cap, species)
        e.sync()
        return msgs

    def deliver(self, rank, msgs):
        for f, m in enumerate(msgs):
            if m is not None and self.w.domains[rank].shared(f):
                to = self.w.destination(rank, f)[0]
                self.engines[to].exchange_inject(m.ptr, m.cap)

    def finish(self, msgs_by_rank=None):
        """exchange_finish on every engine (with the messages it SENT, so that their headers come back); returns the flags"""
        flags, self.headers = [], []
        for rank, e in enumerate(self.engines):
            mine = [m for m in (msgs_by_rank[rank] if msgs_by_rank else []) if m is not None]
            self.headers.append(e.exchange_finish([m.ptr for m in mine]))
            flags.append(e.exchange_flags)
        return flags

    def live(self, rank, sp):
        """(particles, their slots) of the live particles, in array order"""
        r = self.engines[rank].select(sp, index=True)
        return r.particles, r.index

    def movers(self, rank, sp):
        """the movers on the list as (particle, displacement left) records"""
        e = self.engines[rank]
        pm = e.get_movers(sp)
        p, idx = self.live(rank, sp)
        slot = np.full(e.capacity(sp)[0] + 1, -1, np.int64)
        slot[idx] = np.arange(len(idx))
        assert np.all(pm["i"] >= 0) and np.all(pm["i"] < len(slot)) and np.all(slot[pm["i"]] >= 0), "a mover names a dead slot"
        at = pm.copy()
        at["i"] = slot[pm["i"]]
        return R.mover_pairs(p, at)


def ref_caps(per_face, slack=3):
    return [len(r) + slack if len(r) or slack else 0 for r in per_face]


def ref_leavers(w, rank, k):
    """(the movers of species k as (particle, displacement) records, the face each sits on) -- before the reference packs"""
    d = w.domains[rank]
    return R.mover_pairs(d.species[k]["p"], d.movers(k)), R.faces_of_movers(d, k)


def species_equal(dev, w, what, tags=False):
    """every species of every domain holds the reference's live particles, as multisets"""
    for rank, d in enumerate(w.domains):
        for k in range(len(d.species)):
            got, _ = dev.live(rank, k)
            assert dev.engines[rank].np(k) == len(got) == d.species[k]["np"], (what, rank, k, dev.engines[rank].np(k), len(got), d.species[k]["np"])
            assert R.same_multiset(got, d.live(k), R.P_TAGGED if tags else R.P_WORDS), (what, rank, k)


def whole_step(dev, w, max_rounds=6, check_rounds=True):
    """One step of world and engines the way a multi-GPU driver runs it: push every species, then rounds of
    pack -> inject with ONE finish at the end.  Round by round the messages must be the reference's.  Returns the number of
    rounds the reference needed."""
    for d in w.domains:
        for k in range(len(d.species)):
            w.push(d.rank, k)
    dev.begin(clear=True)
    dev.push()
    all_msgs = [[] for _ in w.domains]
    rounds = 0
    for r in range(max_rounds):
        per_face = [w.pack(d.rank) for d in w.domains]
        if not any(len(x) for pf in per_face for x in pf):
            break
        rounds += 1
        msgs = [dev.pack(d.rank, [len(x) + 2 for x in per_face[d.rank]]) for d in w.domains]
        for d in w.domains:
            for f in range(6):
                if not d.shared(f):                                    # (wraps onto the domain, reflects or absorbs: offered, never written)
                    assert msgs[d.rank][f].untouched(), ("round", r, "rank", d.rank, "face", f)
                    msgs[d.rank][f] = None
                elif check_rounds:
                    n = len(per_face[d.rank][f])
                    msgs[d.rank][f].check(n, n, per_face[d.rank][f], ("round", r, "rank", d.rank, "face", f))
            all_msgs[d.rank] += msgs[d.rank]
        for d in w.domains:
            dev.deliver(d.rank, msgs[d.rank])
            for f in range(6):
                if len(per_face[d.rank][f]):
                    w.inject(w.destination(d.rank, f)[0], per_face[d.rank][f])
    else:
        raise AssertionError("the reference still has movers after %d rounds" % max_rounds)
    flags = dev.finish(all_msgs)
    assert flags == [0] * len(w.domains), flags
    for rank, d in enumerate(w.domains):
        for k in range(len(d.species)):
            assert dev.engines[rank].nm(k) == 0
    return rounds


# ---- the first round of the hot case, played once per (grid, order, mode) and looked at by several tests -------------------------
class Played:
    pass


@functools.lru_cache(maxsize=None)
def played(dims, order, mode):
    """Four hot species per domain in the world whose six faces are shared.
    A: begin, push, pack, finish -- the messages and what stays behind;
    B: clear the accumulators, begin, inject the messages, finish -- the arrivals and their deposits.
    Everything observed is recorded; the tests assert.  The engines are left open for test_the_later_rounds, which closes
    them."""
    V = package()
    o = Played()
    scale = pyorc.fixed_scale(X.Q0) if mode == "deterministic" else None
    w = o.w = R.four_species_world("all_shared", dims, scale=scale)
    with knobs(order):
        dev = o.dev = Dev(V, w, order, mode)
    nd, ns = len(w.domains), 4
    for d in w.domains:
        for k in range(ns):
            w.push(d.rank, k)
    o.leavers = [[ref_leavers(w, r, k) for k in range(ns)] for r in range(nd)]
    o.before = [[dev.live(r, k) for k in range(ns)] for r in range(nd)]
    o.extent0 = [[dev.engines[r].capacity(k)[0] for k in range(ns)] for r in range(nd)]
    # A
    dev.begin(clear=True)
    dev.push()
    o.sent = [w.pack(r) for r in range(nd)]
    o.survivors = [[w.domains[r].live(k).copy() for k in range(ns)] for r in range(nd)]
    o.msgs = [dev.pack(r, ref_caps(o.sent[r])) for r in range(nd)]
    o.flags_a = dev.finish(o.msgs)
    o.headers_a = dev.headers
    o.stayed = [[dev.live(r, k) for k in range(ns)] for r in range(nd)]
    o.state_a = [[dict(capacity=dev.engines[r].capacity(k), stats=dev.engines[r].species_stats(k), np=dev.engines[r].np(k),
                       nm=dev.engines[r].nm(k), order=dev.engines[r].species_order(k),
                       tpart=dev.engines[r].get_tile_partition(k) if order == "tile" else None) for k in range(ns)] for r in range(nd)]
    # B (the accumulators start empty again, in the world too: what they hold afterwards is the arrivals' deposits alone)
    dev.begin(clear=True)
    for d in w.domains:
        d.a[:] = 0
        d.a64[:] = 0
    for r in range(nd):
        dev.deliver(r, o.msgs[r])
        for f in range(6):
            if len(o.sent[r][f]):
                w.inject(w.destination(r, f)[0], o.sent[r][f])
    o.flags_b = dev.finish()
    o.arrived = [[dev.live(r, k) for k in range(ns)] for r in range(nd)]
    o.state_b = [[dict(capacity=dev.engines[r].capacity(k), np=dev.engines[r].np(k), nm=dev.engines[r].nm(k)) for k in range(ns)] for r in range(nd)]
    o.movers_b = [[dev.movers(r, k) for k in range(ns)] for r in range(nd)]
    o.ref_movers_b = [[R.mover_pairs(w.domains[r].species[k]["p"], w.domains[r].movers(k)) for k in range(ns)] for r in range(nd)]
    o.ref_np_b = [[w.domains[r].species[k]["np"] for k in range(ns)] for r in range(nd)]
    o.ref_live_b = [[w.domains[r].live(k).copy() for k in range(ns)] for r in range(nd)]
    o.acc = [dev.engines[r].get_accumulator() for r in range(nd)]
    o.ref_acc = [w.domains[r].a[:w.domains[r].og.nv].copy() for r in range(nd)]
    o.ref_words = [w.finalized(r) for r in range(nd)] if scale else None
    o.ref_a64 = [w.domains[r].a64.copy() for r in range(nd)]
    return o


PLAYS = [(dims, order) for dims in R.GRIDS for order in ORDERS]
IDS = ["%dx%dx%d-%s" % (d + (o,)) for d, o in PLAYS]


@pytest.mark.parametrize("dims,order", PLAYS, ids=IDS)
def test_message_contents(dims, order):
    """After begin, advance_p_async, pack, finish: every face's header is {count, wanted, 0, 0} with both equal to the
    reference's count -- in the message and in what finish returns -- its payload [0, count) is the reference's injectors of
    that face bit for bit as a multiset (remapped voxel, mirrored coordinate, displacement left, species id), and no byte is
    written behind the count."""
    o = played(dims, order, "float")
    assert o.flags_a == [0, 0]
    for r in range(2):
        assert [m is not None for m in o.msgs[r]] == [True] * 6
        for f in range(6):
            n = len(o.sent[r][f])
            assert n > 0
            o.msgs[r][f].check(n, n, o.sent[r][f], (dims, order, r, f))
        assert o.headers_a[r] == [[len(o.sent[r][f])] * 2 + [0, 0] for f in range(6)]


@pytest.mark.parametrize("dims,order", PLAYS, ids=IDS)
def test_what_stays_behind(dims, order):
    """The senders' slots are dead exactly at the reference's leavers: the extent is unchanged, dead_slots is the number
    gone, np() counts the live ones, every survivor sits in the slot it had with the words the reference has, the order
    flag survives and the tile partition still bounds every live particle's key."""
    o = played(dims, order, "float")
    for r in range(2):
        for k in range(4):
            st, (p0, i0), (p1, i1) = o.state_a[r][k], o.before[r][k], o.stayed[r][k]
            gone = len(o.leavers[r][k][0])
            assert gone > 0 and st["capacity"][0] == o.extent0[r][k] == len(p0)
            assert st["stats"]["dead_slots"] == gone and st["np"] == len(p0) - gone == len(p1) and st["nm"] == 0
            assert R.same_multiset(p1, o.survivors[r][k], R.P_TAGGED)
            # slot by slot: a survivor has not moved, and carries its tags
            assert np.all(np.isin(i1, i0))
            was = np.full(len(p0), -1, np.int64)
            was[i0] = np.arange(len(p0))
            assert np.array_equal(p1["tag"], p0["tag"][was[i1]]) and np.array_equal(p1["tag2"], p0["tag2"][was[i1]])
            assert np.array_equal(p1["q"].view(np.uint32), p0["q"][was[i1]].view(np.uint32))
            if order == "tile":
                # the partition describes the array as it was SORTED: every slot still lies in the range of the key its
                # particle had before the push (its tile's range when the species is sorted by tile only) -- the exchange
                # has moved nothing
                assert st["order"] == "tile"
                tp, key = st["tpart"], tile_key(p0["i"].astype(np.int64), *dims)
                lo, hi = (key // 64 * 64, key // 64 * 64 + 64) if st["stats"]["by_tile_only"] else (key, key + 1)
                assert np.all(tp[lo] <= i0) and np.all(i0 < tp[hi])
                assert np.all(tp[lo[was[i1]]] <= i1) and np.all(i1 < tp[hi[was[i1]]])


@pytest.mark.parametrize("dims,order", PLAYS, ids=IDS)
def test_arrivals(dims, order):
    """After exchange_inject: the receiver holds the reference's particles as a multiset; the arrivals occupy the slots
    [old extent, new extent) with tags 0; every particle that was there keeps its slot, words and tags; the movers made by
    arrivals that stopped on another face name the arrival's slot -- (particle at the slot, displacement left) pairs equal
    the reference's as a multiset -- and nm() is the reference's."""
    o = played(dims, order, "float")
    assert o.flags_b == [0, 0]
    stopped = 0
    for r in range(2):
        for k in range(4):
            (p1, i1), (p2, i2) = o.stayed[r][k], o.arrived[r][k]
            ext1, ext2 = o.state_a[r][k]["capacity"][0], o.state_b[r][k]["capacity"][0]
            n_new = o.ref_np_b[r][k] - len(o.survivors[r][k])
            assert n_new > 0 and ext2 == ext1 + n_new
            assert o.state_b[r][k]["np"] == o.ref_np_b[r][k] == len(p2)
            assert R.same_multiset(p2, o.ref_live_b[r][k], R.P_WORDS)
            old, new = i2 < ext1, i2 >= ext1
            assert np.array_equal(i2[old], i1) and int(new.sum()) == n_new
            for c in R.P_TAGGED:
                assert np.array_equal(p2[c][old].view("u%d" % p2.dtype[c].itemsize), p1[c].view("u%d" % p1.dtype[c].itemsize)), c
            assert np.all(p2["tag"][new] == 0) and np.all(p2["tag2"][new] == 0)
            assert o.state_b[r][k]["nm"] == len(o.ref_movers_b[r][k]) == len(o.movers_b[r][k])
            assert R.same_multiset(o.movers_b[r][k], o.ref_movers_b[r][k], R.INJ_WORDS)
            stopped += len(o.ref_movers_b[r][k])
    assert stopped > 0


FLOAT_ERRORS = {}


@pytest.mark.parametrize("dims,order", PLAYS, ids=IDS)
def test_deposits_of_the_arrivals_float(dims, order):
    """The receiver's accumulator after the injection (cleared before it: the arrivals' deposits alone, not hidden behind
    the push's), float sums: within the project's stated bound of the reference's -- 2e-6 of the largest entry (include/vpic_hip.h, vpic_hip_set_accumulation; test_gpu_tiles.acc_close).
    Observed error / bound on an MI355X: 0.07 to 0.3 as a rule, largest on (1, 4, 3), whose 12 cells collect the most deposits per
    word: 0.22 to 0.49 there in 100 samples, 0.65 once."""
    o = played(dims, order, "float")
    for r in range(2):
        a, ref = o.acc[r], o.ref_acc[r]
        err = max(float(np.abs(a[c].astype(np.float64) - ref[c]).max()) for c in ("jx", "jy", "jz"))
        top = max(float(np.abs(ref[c]).max()) for c in ("jx", "jy", "jz"))
        FLOAT_ERRORS[(dims, order, r)] = err / (ACC_TOL * top)
        print("accumulator %s %s rank %d: worst error %.3e = %.3f of the bound" % (dims, order, r, err, err / (ACC_TOL * top)))
        assert top > 0
        acc_close(a, ref)


@pytest.mark.parametrize("order", ORDERS)
def test_deposits_of_the_arrivals_deterministic(order):
    """The same in deterministic mode on one grid: every word equal to pyorc.finalize of the exact integer sums of the
    injection."""
    dims = (9, 2, 6)
    o = played(dims, order, "deterministic")
    assert o.flags_a == [0, 0] and o.flags_b == [0, 0]
    for r in range(2):
        for k in range(4):
            assert R.same_multiset(o.arrived[r][k][0], o.ref_live_b[r][k], R.P_WORDS)
        msg = X.describe_bad_words(o.acc[r], o.ref_a64[r], np.zeros(len(o.ref_a64[r]), np.int32), o.w.scale, dims)
        assert msg is None, msg
    close_played(dims, order, "deterministic")


def close_played(dims, order, mode):
    played(dims, order, mode).dev.close()


@pytest.mark.parametrize("dims,order", PLAYS, ids=IDS)
def test_the_later_rounds(dims, order):
    """From where the first round left the engines: rounds of begin / pack / inject / finish until the reference has no
    mover left (a fixed number: the reference's), every message the reference's; then sort_p drops the dead slots -- no
    dead slot, extent equal to the live count -- and every species holds the reference's particles."""
    o = played(dims, order, "float")
    w, dev = o.w, o.dev
    try:
        for r in range(6):
            per_face = [w.pack(d.rank) for d in w.domains]
            if not any(len(x) for pf in per_face for x in pf):
                break
            dev.begin()
            msgs = [dev.pack(d.rank, ref_caps(per_face[d.rank], slack=0)) for d in w.domains]
            for d in w.domains:
                for f in range(6):
                    n = len(per_face[d.rank][f])
                    if n:
                        msgs[d.rank][f].check(n, n, per_face[d.rank][f], ("later round", r, d.rank, f))
                        w.inject(w.destination(d.rank, f)[0], per_face[d.rank][f])
                dev.deliver(d.rank, msgs[d.rank])
            assert dev.finish(msgs) == [0, 0]
        else:
            raise AssertionError("movers left")
        assert r >= 1
        species_equal(dev, w, "after the last round")
        for rank, e in enumerate(dev.engines):
            for k in range(4):
                assert e.nm(k) == 0 and e.species_stats(k)["dead_slots"] > 0
                e.sort_p(k)
                assert e.species_stats(k)["dead_slots"] == 0 and e.capacity(k)[0] == e.np(k) == w.domains[rank].species[k]["np"]
                assert R.same_multiset(e.get_particles(k), w.domains[rank].live(k), R.P_WORDS)
                assert np.all(e.get_particles(k)["i"] > 0)
        # One more step.  The sort has shortened the arrays, so this step's arrivals land on slots that held other particles
        # before, tags and all: they must come in untagged all the same.
        extent = [[e.capacity(k)[0] for k in range(4)] for e in dev.engines]
        whole_step(dev, w)
        species_equal(dev, w, "the step after the sort")
        for rank in range(2):
            for k in range(4):
                p, idx = dev.live(rank, k)
                new = idx >= extent[rank][k]
                assert new.sum() > 64 and np.all(p["tag"][new] == 0) and np.all(p["tag2"][new] == 0), (rank, k)
                assert np.any(p["tag"][~new] != 0) == R.TAGGED[k]
    finally:
        dev.close()


# ---- the pattern cases: 1, 63, 64, 65, 300 movers through one face ---------------------------------------------------------------
@pytest.mark.parametrize("dims", [(4, 4, 4), (1, 4, 3)], ids=["4x4x4", "1x4x3"])
@pytest.mark.parametrize("n", R.PATTERN_COUNTS)
def test_n_movers_through_one_face(V, dims, n):
    """exactly n movers, all through +x (a lone one, a wavefront less one, a full one, one more, more than a workgroup):
    one step, one round; on (1, 4, 3) the low and the high x face share the cell and the voxel remap adds 0"""
    w = R.pattern_world(dims, n)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        assert whole_step(dev, w) == 1
        species_equal(dev, w, "pattern")
        acc_close(dev.engines[1].get_accumulator(), w.domains[1].a[:w.domains[1].og.nv])


# ---- several species --------------------------------------------------------------------------------------------------------------
def test_messages_per_species(V):
    """exchange_pack_species with one mask per species: the four messages of a face hold the reference's records of that
    species each, and together what exchange_pack for all species sends"""
    dims = (5, 3, 2)
    w = R.four_species_world("all_shared", dims)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        for d in w.domains:
            for k in range(4):
                w.push(d.rank, k)
        sent = w.pack(0)
        dev.begin(clear=True)
        dev.push()
        all_msgs = []
        for k in range(4):
            mine = [np.ascontiguousarray(s[s["sp_id"] == k]) for s in sent]
            msgs = dev.pack(0, ref_caps(mine), species=[k])
            for f in range(6):
                assert len(mine[f]) > 0
                msgs[f].check(len(mine[f]), len(mine[f]), mine[f], ("species", k, "face", f))
            all_msgs += msgs
        assert dev.engines[0].exchange_finish([m.ptr for m in all_msgs]) == [[m.read()[0][0]] * 2 + [0, 0] for m in all_msgs]
        assert dev.engines[0].exchange_flags == 0 and all(dev.engines[0].nm(k) == 0 for k in range(4))


def test_an_interleaved_message_lands_each_record_in_its_species(V):
    """One hand-made message: the reference's records of all six faces of round one, species mixed record by record, with
    records of species -1 and of species 4 (= the species count) among them.  Each record lands in its own species, the two
    bad kinds are skipped without any other effect, nm() is the reference's.  Then: a header count above cap injects cap
    records, a negative one none."""
    dims = (4, 4, 4)
    w = R.four_species_world("all_shared", dims)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        for k in range(4):
            w.push(0, k)
        good = R.interleaved(np.concatenate(w.pack(0)))
        assert R.species_in_windows(good) >= 3
        bad = good[:40].copy()
        bad["sp_id"][:20], bad["sp_id"][20:] = -1, 4
        bad["q"] *= np.float32(64.0)                                   # (would show in q_max and in the accumulator)
        mixed = R.interleaved(np.concatenate([good, bad]), seed=4)
        e = dev.engines[1]
        e.clear_accumulators()
        e.exchange_begin()
        m = Msg(len(mixed) + 5).write([len(mixed), len(mixed), 0, 0], mixed)
        e.exchange_inject(m.ptr, m.cap)
        e.exchange_finish([])
        assert e.exchange_flags == 0
        w.inject(1, good)
        for k in range(4):
            got, _ = dev.live(1, k)
            assert e.np(k) == len(got) == w.domains[1].species[k]["np"]
            assert R.same_multiset(got, w.domains[1].live(k), R.P_WORDS), k
            assert e.nm(k) == w.domains[1].species[k]["nm"]
            assert R.same_multiset(dev.movers(1, k), R.mover_pairs(w.domains[1].species[k]["p"], w.domains[1].movers(k)), R.INJ_WORDS)
        acc_close(e.get_accumulator(), w.domains[1].a[:w.domains[1].og.nv])
        # the header's count against the capacity
        w1 = R.four_species_world("all_shared", dims)                  # (fresh records: domain 1's own leavers, sent to domain 0)
        for k in range(4):
            w1.push(1, k)
        more = R.interleaved(np.concatenate(w1.pack(1)), seed=5)
        cap = len(more) - 50
        e0 = dev.engines[0]
        e0.exchange_begin()
        over = Msg(cap).write([len(more), len(more), 0, 0], more[:cap])
        e0.exchange_inject(over.ptr, cap)
        none = Msg(cap).write([-7, -7, 0, 0], more[:cap])
        e0.exchange_inject(none.ptr, cap)
        e0.exchange_finish([])
        assert e0.exchange_flags == 0
        # (domain 0 was never pushed on the device: it holds its initial particles and the first `cap` records)
        w0 = R.four_species_world("all_shared", dims)
        w0.inject(0, more[:cap])
        for k in range(4):
            got, _ = dev.live(0, k)
            assert R.same_multiset(got, w0.domains[0].live(k), R.P_WORDS), k


# ---- rounds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", R.GRIDS, ids=["%dx%dx%d" % d for d in R.GRIDS])
@pytest.mark.parametrize("order", ORDERS)
def test_three_rounds_under_one_finish(V, dims, order):
    """The corner particle leaves through +x, arrives, stops on +y, is sent back, stops on +z, is sent again: three rounds
    of pack -> inject between one begin and one finish, each round's messages the reference's, and it ends bit-equal to
    the reference's (as every other particle does)."""
    w = R.corner_world(dims)
    with knobs(order), Dev(V, w, order) as dev:
        assert whole_step(dev, w) >= 3
        species_equal(dev, w, "corner")
        where = [(r, p[p["q"] == R.CORNER_Q]) for r in range(2) for p in [dev.live(r, 0)[0]]]
        mine = [(r, p) for r, p in where if len(p)]
        assert len(mine) == 1 and len(mine[0][1]) == 1
        ref = w.domains[mine[0][0]].live(0)
        assert R.same_multiset(mine[0][1], ref[ref["q"] == R.CORNER_Q], R.P_WORDS)


@pytest.mark.parametrize("kind", ["tile", "voxel", "tile_with_tail"])
def test_a_phased_push_sends_everything_once(V, kind):
    """advance_p_phase(sp, 1), exchange_pack_species, advance_p_phase(sp, 2), then a later exchange_pack: across its rounds
    the species delivers exactly the reference's multiset per face -- nothing twice, nothing left -- for a species in tile
    order (whose interior tiles wait for phase 2), one that is not, and one with an appended tail."""
    dims = (9, 2, 6)
    w = R.World("slabs", dims)
    order = "voxel" if kind == "voxel" else "tile"
    p = R.hot(51, dims, n=3 * R.N_HOT)
    tail = R.hot(52, dims, n=300, first_tag=10 ** 6)
    w.domains[0].add_species(R.Q_M[0], p, 8 * R.N_HOT)
    w.domains[1].add_species(R.Q_M[0], R.hot(53, dims, n=10, first_tag=2 * 10 ** 6), 8 * R.N_HOT)
    with knobs(order), Dev(V, w, order) as dev:
        e = dev.engines[0]
        if kind == "tile_with_tail":
            e.append_particles(0, tail)
            s = w.domains[0].species[0]
            s["p"][s["np"]:s["np"] + len(tail)] = tail
            s["np"] += len(tail)
        extent = e.capacity(0)[0]
        assert w.push(0, 0) > 64
        sent = w.pack(0)
        assert len(sent[0]) > 0 and len(sent[3]) > 0
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_phase(0, 1)
        first = dev.pack(0, ref_caps(sent), species=[0])
        e.advance_p_phase(0, 2)
        second = dev.pack(0, ref_caps(sent))
        headers = e.exchange_finish([m.ptr for m in first + second if m])
        assert e.exchange_flags == 0 and e.nm(0) == 0
        for f in (0, 3):
            a, b = first[f].read(), second[f].read()
            na, nb = int(a[0][0]), int(b[0][0])
            assert list(a[0]) == [na, na, 0, 0] and list(b[0]) == [nb, nb, 0, 0] and na + nb == len(sent[f])
            assert R.same_multiset(np.concatenate([a[1][:na], b[1][:nb]]), sent[f], R.INJ_WORDS), f
            assert np.all(a[1][na:].view(np.uint8) == 0xFF) and np.all(b[1][nb:].view(np.uint8) == 0xFF)
            assert np.all(a[2] == 0xFF) and np.all(b[2] == 0xFF)
            if kind != "voxel":
                assert na > 0                                          # (the tiles on the shared faces were pushed first)
        assert len(headers) == 12
        for f in (1, 2, 4, 5):                                         # (faces that wrap onto the domain itself: offered, never written)
            assert first[f].untouched() and second[f].untouched()
        got, _ = dev.live(0, 0)
        assert e.capacity(0)[0] == extent and R.same_multiset(got, w.domains[0].live(0), R.P_TAGGED)
        acc_close(e.get_accumulator(), w.domains[0].a[:w.domains[0].og.nv])


# ---- full messages, closed faces, narrow launches -------------------------------------------------------------------------------------
def parked_of(leavers, faces, face, payload):
    """the leavers through `face` whose record is not in the payload (a record keeps momentum, charge and displacement)"""
    mine = leavers[faces == face]
    key = ("ux", "uy", "uz", "q") + R.DISP
    sent = {tuple(r) for r in R.rows(payload, key).tolist()}
    keep = np.array([tuple(r) not in sent for r in np.stack([np.ascontiguousarray(mine[c]).view(np.uint32).astype(np.uint64) for c in key], 1).tolist()], bool)
    return mine[keep]


@pytest.mark.parametrize("small", ["cap 1", "half"])
def test_a_full_message_parks_the_rest(V, small):
    """Face +x gets a cap below what it wants (1, and half), the other faces exactly what they want: flag 2, header
    {cap, wanted}, the payload a sub-multiset of the reference's of size cap; the parked particles are alive and unchanged
    and their movers are on the list with their displacements (nm() == wanted - cap).  A second begin / pack / finish with
    room sends the rest: the union is the reference's multiset and the receiver ends equal to the reference."""
    dims = (4, 4, 4)
    w = R.corner_world(dims)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        e = dev.engines[0]
        w.push(0, 0)
        leavers, faces = ref_leavers(w, 0, 0)
        sent = w.pack(0)
        wanted = len(sent[3])
        cap = 1 if small == "cap 1" else wanted // 2
        assert wanted > 8
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        caps = [len(s) for s in sent]
        caps[3] = cap
        msgs = dev.pack(0, caps)
        headers = e.exchange_finish([m.ptr for m in msgs])
        assert e.exchange_flags & 2 and not e.exchange_flags & ~3
        for f in range(6):
            msgs[f].check(caps[f], len(sent[f]), sent[f], ("full", f))
            assert headers[f] == [caps[f], len(sent[f]), 0, 0]
        parked = parked_of(leavers, faces, 3, msgs[3].read()[1][:cap])
        assert len(parked) == wanted - cap == e.nm(0)
        assert R.same_multiset(dev.movers(0, 0), parked, R.INJ_WORDS)
        got, _ = dev.live(0, 0)
        alive = np.zeros(len(parked), L.particle_t)
        for c in R.P_WORDS:
            alive[c] = parked[c]
        assert R.same_multiset(got, np.concatenate([w.domains[0].live(0), alive]), R.P_WORDS)
        assert e.species_stats(0)["dead_slots"] == len(leavers) - len(parked)
        # the rest
        e.exchange_begin()
        rest = dev.pack(0, [0, 0, 0, wanted, 0, 0])
        assert e.exchange_finish([rest[3].ptr]) == [[wanted - cap] * 2 + [0, 0]] and e.exchange_flags == 0 and e.nm(0) == 0
        second = rest[3].check(wanted - cap, wanted - cap, sent[3], "the rest")
        assert R.same_multiset(np.concatenate([msgs[3].read()[1][:cap], second]), sent[3], R.INJ_WORDS)
        got, _ = dev.live(0, 0)
        assert R.same_multiset(got, w.domains[0].live(0), R.P_TAGGED)
        # the receiver
        r = dev.engines[1]
        r.clear_accumulators()
        r.exchange_begin()
        dev.deliver(0, msgs)
        dev.deliver(0, rest)
        r.exchange_finish([])
        assert r.exchange_flags == 0
        w.inject(1, np.concatenate(sent))
        got, _ = dev.live(1, 0)
        assert R.same_multiset(got, w.domains[1].live(0), R.P_WORDS) and r.nm(0) == w.domains[1].species[0]["nm"]


def closed_face_reference(w):
    """(leavers, their faces, records per face) of domain 0's one species -- called once the engines hold the particles"""
    w.push(0, 0)
    leavers, faces = ref_leavers(w, 0, 0)
    sent = w.pack(0)
    assert all(len(s) > 8 for s in sent)
    return leavers, faces, sent


def test_a_closed_face_parks_its_movers(V):
    """Face +x is given no message in round one: its movers are parked (alive, on the list), the other faces are served as
    if nothing had happened, flag 2 is set."""
    w = R.corner_world((4, 4, 4))
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        e = dev.engines[0]
        leavers, faces, sent = closed_face_reference(w)
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        caps = [len(s) + 3 for s in sent]
        caps[3] = 0
        msgs = dev.pack(0, caps)
        e.exchange_finish([m.ptr for m in msgs if m])
        assert e.exchange_flags == 2
        for f in (0, 1, 2, 4, 5):
            msgs[f].check(len(sent[f]), len(sent[f]), sent[f], ("closed", f))
        parked = leavers[faces == 3]
        assert e.nm(0) == len(parked) == len(sent[3])
        assert R.same_multiset(dev.movers(0, 0), parked, R.INJ_WORDS)
        assert e.species_stats(0)["dead_slots"] == len(leavers) - len(parked)


def test_a_closed_face_opened_in_the_same_step_starts_at_slot_zero(V):
    """The same, and the NEXT exchange_pack of the same begin ... finish gives the face a message: header and payload must be
    the reference's.  (The face's slot counter used to keep the count of the round that parked the movers: the header said
    twice the count and the first payload slots were never written.)"""
    w = R.corner_world((4, 4, 4))
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        e = dev.engines[0]
        leavers, faces, sent = closed_face_reference(w)
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        caps = [len(s) + 3 for s in sent]
        first = dev.pack(0, caps[:3] + [0] + caps[4:])
        second = dev.pack(0, [0, 0, 0, caps[3], 0, 0])
        headers = e.exchange_finish([second[3].ptr])
        n = len(sent[3])
        assert headers == [[n, n, 0, 0]], headers
        second[3].check(n, n, sent[3], "reopened")
        assert e.exchange_flags == 2 and e.nm(0) == 0                  # (round one did park them: the flag says so)
        for f in (0, 1, 2, 4, 5):
            first[f].check(len(sent[f]), len(sent[f]), sent[f], ("closed", f))
        got, _ = dev.live(0, 0)
        assert R.same_multiset(got, w.domains[0].live(0), R.P_TAGGED)


@pytest.mark.parametrize("cap", [None, 60], ids=["room", "full messages too"])
def test_a_narrow_launch_takes_its_movers_in_turns(V, cap):
    """700 movers, mover_cap 100: each begin / pack / finish classifies 100 and keeps the rest at the front of the list --
    nm() is 600, 500, ... and bit 1 is set while movers remain; after ceil(700 / 100) + 1 rounds at the most nothing is left
    and sender, messages and receiver equal the reference.  With messages of 60 on top, each round sends 60 and parks 40
    behind the uncovered ones: nm() is 640, 580, ... and both bits are set; ceil(700 / 60) + 1 rounds at the most."""
    dims, n = (4, 4, 4), 700
    w = R.pattern_world(dims, n)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        e, r = dev.engines
        assert w.push(0, 0) == n
        sent = w.pack(0)[3]
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        per_round = cap or 100
        rounds = -(-n // per_round) + 1
        got = []
        for k in range(rounds):
            left = max(n - per_round * (k + 1), 0)
            covered = min(100, n - per_round * k)
            if covered <= 0:
                break
            if k:
                e.exchange_begin()
            m = dev.pack(0, [0, 0, 0, cap or 128, 0, 0], mover_cap=100)[3]
            header = e.exchange_finish([m.ptr])[0]
            assert e.nm(0) == left, (k, e.nm(0), left)
            want_flags = (1 if n - per_round * k > 100 else 0) | (2 if cap and covered > cap else 0)
            assert e.exchange_flags == want_flags, (k, e.exchange_flags, want_flags)
            assert header == [min(covered, per_round), covered, 0, 0], (k, header)
            got.append(m.check(header[0], header[1], sent, ("narrow", k)))
            if k == 0:
                r.clear_accumulators()
            r.exchange_begin()
            r.exchange_inject(m.ptr, m.cap)
            r.exchange_finish([])
            assert r.exchange_flags == 0
        assert e.nm(0) == 0
        assert R.same_multiset(np.concatenate(got), sent, R.INJ_WORDS)
        w.inject(1, sent)
        species_equal(dev, w, "narrow")


# ---- absorbing faces on the resident path ---------------------------------------------------------------------------------------------
RHOB_ERRORS = {}


@pytest.mark.parametrize("dims", R.GRIDS, ids=["%dx%dx%d" % d for d in R.GRIDS])
@pytest.mark.parametrize("order", ORDERS)
def test_absorbing_faces(V, dims, order):
    """Domain 0 absorbs on -x and on both z faces, wraps in y, shares +x.  Every face is OFFERED a message: the absorbed
    particles are dead, rhob is within the rounding bound of a float sum in another order of the reference's own addends
    (per node gamma_n sum |w|), only the shared face's message is written, and it is the reference's."""
    w = R.absorbing_world(dims)
    with knobs(order), Dev(V, w, order) as dev:
        e, d = dev.engines[0], w.domains[0]
        nm = w.push(0, 0)
        nodes, addends = R.absorbed_addends(d, 0)
        sent = w.pack(0)
        assert len(nodes) >= 64 and len(sent[3]) > 0
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        msgs = dev.pack(0, [len(s) + 8 for s in sent])
        e.exchange_finish([msgs[3].ptr])
        assert e.exchange_flags == 0 and e.nm(0) == 0
        for f in (0, 1, 2, 4, 5):
            assert msgs[f].untouched(), f
        msgs[3].check(len(sent[3]), len(sent[3]), sent[3], "absorbing")
        assert e.species_stats(0)["dead_slots"] == nm and e.np(0) == d.species[0]["np"]
        got, _ = dev.live(0, 0)
        assert R.same_multiset(got, d.live(0), R.P_TAGGED)
        exact, bound = R.rhob_bound(d.og.nv, nodes, addends)
        rhob = e.get_fields()["rhob"].astype(np.float64)
        err = np.abs(rhob - exact)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(bound > 0, err / bound, 0.0)
        RHOB_ERRORS[(dims, order)] = float(frac.max())
        print("rhob %s %s: worst error %.3f of its bound" % (dims, order, frac.max()))
        assert np.all(err <= bound), (float(err.max()), int(np.argmax(err - bound)))
        assert np.all(rhob[bound == 0] == exact[bound == 0])


# ---- charge bookkeeping -----------------------------------------------------------------------------------------------------------------
def bookkeeping_world(case):
    """world "one_face" on (5, 3, 2): domain 0 sends 300 particles of |q| in (0.5, 1.5) through +x; domain 1's species holds
    chargeless particles, nothing, or particles of |q| = 2^-6"""
    dims = (5, 3, 2)
    w = R.World("one_face", dims)
    w.domains[0].add_species(R.Q_M[0], R.through_face(61, 300, dims, 3, q0=-1.0), 1024)
    own = R.hot(62, dims, n=400, u=X.COLD, first_tag=5001)
    own["q"] = {"zero_q": 0.0, "empty": 0.0, "lighter": 2.0 ** -6}[case] * np.where(np.arange(400) % 2, 1.0, -1.0)
    w.domains[1].add_species(R.Q_M[0], own[:0] if case == "empty" else own, 2048)
    return w, dims


@pytest.mark.parametrize("path", ["exchange_inject", "boundary_p_inject"])
@pytest.mark.parametrize("case", ["zero_q", "empty", "lighter"])
def test_arriving_charges_are_booked(V, case, path):
    """Arrivals count towards "the largest |q| that has ever gone into the species" (include/vpic_hip.h).  A deterministic
    engine that was given no q_ref and holds only chargeless particles, nothing at all, or charges of 2^-6 receives charges
    up to 1.5: the injection works, and afterwards accumulate_hydro_p and accumulate_rho_p equal the exact reference of
    tests/moments_exact.py word for word at the scales of the largest charge that went in, and the next advance_p deposits
    the reference's current exactly.  (Before arrivals were booked: "no macro-particle charge is known yet" for the first
    two, the moments at the scale of 2^-6 for the third.)"""
    w, dims = bookkeeping_world(case)
    with knobs(None), Dev(V, w, None, "deterministic", q_ref=0.0) as dev:
        e, d = dev.engines[1], w.domains[1]
        assert w.push(0, 0) == 300
        sent = w.pack(0)[3]
        own_q = M.q_max_of(d.live(0))
        q_first = own_q if own_q > 0 else float(np.abs(sent["q"]).max())     # the charge the accumulator's scale comes from
        w.scale = pyorc.fixed_scale(q_first)
        if path == "exchange_inject":
            s = dev.engines[0]
            s.clear_accumulators()
            s.exchange_begin()
            s.advance_p_async(0)
            msg = dev.pack(0, [0, 0, 0, len(sent) + 3, 0, 0])[3]
            s.exchange_finish([])
            msg.check(len(sent), len(sent), sent, "bookkeeping")
            w.push(1, 0)
            e.clear_accumulators()
            e.exchange_begin()
            e.advance_p_async(0)
            e.exchange_inject(msg.ptr, msg.cap)
            e.exchange_finish([])
            assert e.exchange_flags == 0
        else:
            w.push(1, 0)
            e.clear_accumulators()
            e.advance_p(0)
            keep, ptr = device_records(sent)
            e.boundary_p_inject(ptr, len(sent))
        w.inject(1, sent)
        assert e.nm(0) == d.species[0]["nm"] == 0
        got, _ = dev.live(1, 0)
        assert R.same_multiset(got, d.live(0), R.P_WORDS)
        msg_a = X.describe_bad_words(e.get_accumulator(), d.a64, np.zeros(d.og.nv, np.int32), w.scale, dims)
        assert msg_a is None, msg_a
        # the moments, at the scales of the largest charge that ever went in
        q_top = max(own_q, float(np.abs(sent["q"]).max()))
        ref = M.Reference(d.og, d.live(0), R.Q_M[0], d.fi, q_max=q_top, q_ref=q_first)
        e.clear_hydro()
        e.accumulate_hydro_p(0)
        bad = M.describe_bad_words(e.get_hydro(), ref.hydro_words(), [ref])
        assert bad is None, bad
        e.clear_rhof()
        e.accumulate_rho_p(0)
        bad = M.describe_bad_words(e.get_fields()["rhof"], ref.rho_words(), [ref], rho=True)
        assert bad is None, bad
        # the next push
        d.a64[:] = 0
        nm = w.push(1, 0)
        e.clear_accumulators()
        assert e.advance_p(0) == nm
        msg_a = X.describe_bad_words(e.get_accumulator(), d.a64, np.zeros(d.og.nv, np.int32), w.scale, dims)
        assert msg_a is None, msg_a
        assert np.abs(d.a64).max() > 0


# ---- the tail -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail_sort_min", [1, 1 << 20], ids=["tail regrouped", "tail as it is"])
def test_arrivals_that_leave_again_from_the_tail(V, tail_sort_min):
    """Tile order: the arrivals of step one land behind the sorted particles; some of them leave again in step two, which
    puts dead slots inside the appended tail; the push of step three regroups that tail (VPIC_HIP_TAIL_SORT_MIN below its
    length) or takes it as it is (above).  Every message of every round and every particle bit-equal to the reference."""
    dims = (9, 2, 6)
    w = R.corner_world(dims)
    with knobs("tile", VPIC_HIP_TAIL_SORT_MIN=str(tail_sort_min)), Dev(V, w, "tile") as dev:
        for step in range(3):
            whole_step(dev, w)
            species_equal(dev, w, ("tail", step))
            for rank, e in enumerate(dev.engines):
                assert e.species_order(0) == "tile"
                acc_close(e.get_accumulator(), w.domains[rank].a[:w.domains[rank].og.nv])
                w.domains[rank].a[:] = 0
        e = dev.engines[0]
        assert e.species_stats(0)["dead_slots"] > 0 and e.capacity(0)[0] > e.np(0)


# ---- the host-count path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(5, 3, 2), (1, 4, 3)], ids=["5x3x2", "1x4x3"])
def test_the_legacy_path_agrees(V, dims):
    """boundary_p_pack, boundary_p_counts and get_injectors give, for the same species state, the per-face multisets of the
    resident path (the reference's); their back-filled array is dense and holds the reference's survivors."""
    w = R.corner_world(dims)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        e, d = dev.engines[0], w.domains[0]
        nm = w.push(0, 0)
        sent = w.pack(0)
        e.clear_accumulators()
        assert e.advance_p(0) == nm
        e.boundary_p_pack()
        counts = (C.c_int32 * 6)()
        assert V.lib().vpic_hip_boundary_p_counts(e._h, counts) == 0
        assert list(counts) == [len(s) for s in sent]
        for f in range(6):
            m = Msg(max(counts[f], 1))                               # (a message buffer as a plain device array: records from byte 16)
            e.get_injectors(f, m.ptr + 16)
            e.sync()
            header, payload, guard = m.read()
            assert R.same_multiset(payload[:counts[f]], sent[f], R.INJ_WORDS), f
            assert np.all(header == -1) and np.all(payload[counts[f]:].view(np.uint8) == 0xFF) and np.all(guard == 0xFF)
        assert e.np(0) == e.capacity(0)[0] == d.species[0]["np"] and e.species_stats(0)["dead_slots"] == 0
        got = e.get_particles_range(0, 0, e.np(0))
        assert np.all(got["i"] > 0) and R.same_multiset(got, d.live(0), R.P_TAGGED)


# ---- errors: argument and capacity paths ------------------------------------------------------------------------------------------------------
def small_pair(V, max_np=None, max_nm=None, n=700, world=None):
    w = world or R.pattern_world((4, 4, 4), n)
    return w, Dev(V, w, "voxel", max_np=max_np, max_nm=max_nm)


def raises(V, text):
    return pytest.raises(V.VpicHipError, match=text)


def test_argument_errors(V):
    """exchange_pack before exchange_begin, exchange_inject before it, mover_cap < 1, a null message or cap < 1 for
    exchange_inject, more messages than the limit for exchange_finish (192: the limit itself is served), reflux handlers
    registered: each an error with its message, and the engine goes on working."""
    w, dev = small_pair(V, n=65)
    with knobs("voxel"), dev:
        e = dev.engines[0]
        m = Msg(80)
        with raises(V, "before vpic_hip_exchange_begin"):
            e.exchange_pack([0, 0, 0, m.ptr, 0, 0], [0, 0, 0, 80, 0, 0], WIDE)
        with raises(V, "before vpic_hip_exchange_begin"):
            e.exchange_inject(m.ptr, 80)
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        for bad in (0, -5):
            with raises(V, "Bad mover capacity"):
                e.exchange_pack([0, 0, 0, m.ptr, 0, 0], [0, 0, 0, 80, 0, 0], bad)
        with raises(V, "Bad exchange message"):
            e.exchange_inject(0, 80)
        for bad in (0, -1):
            with raises(V, "Bad exchange message"):
                e.exchange_inject(m.ptr, bad)
        assert m.untouched()
        with raises(V, "Bad message list"):
            e.exchange_finish([m.ptr] * 193)
        with raises(V, "Bad message list"):
            e._ck(V.lib().vpic_hip_exchange_finish(e._h, None, -1, None, None))
        e.exchange_pack([0, 0, 0, m.ptr, 0, 0], [0, 0, 0, 80, 0, 0], WIDE)
        assert e.exchange_finish([m.ptr] * 192) == [[65, 65, 0, 0]] * 192 and e.exchange_flags == 0 and e.nm(0) == 0
        e.set_maxwellian_reflux(-3, [0.1], [0.1])
        e.exchange_begin()
        with raises(V, "custom particle boundary handlers"):
            e.exchange_pack([0, 0, 0, m.ptr, 0, 0], [0, 0, 0, 80, 0, 0], WIDE)


def test_arrivals_beyond_max_np(V):
    """flag 4: 65 arrivals for a species with room for 30 more -- an error that names the remedy; the species is full, not
    overrun (its extent is max_np)"""
    w, dev = small_pair(V, n=65)
    with knobs("voxel"), dev:
        w.push(0, 0)
        sent = w.pack(0)[3]
        r = V.Engine(V.make_grid(*w.domains[1].args, **w.domains[1].kw))
        try:
            r.set_interpolator(w.domains[1].fi)
            own = w.domains[1].live(0)
            sp = r.new_species(R.Q_M[0], len(own) + 30, 64)
            r.set_particles(sp, own)
            r.exchange_begin()
            m = Msg(len(sent)).write([len(sent)] * 2 + [0, 0], sent)
            r.exchange_inject(m.ptr, m.cap)
            with raises(V, "ran out of particle slots"):
                r.exchange_finish([])
            assert r.capacity(sp)[0] == len(own) + 30
        finally:
            r.close()


def test_stopped_arrivals_beyond_max_nm(V):
    """flag 8: arrivals that stop on a face of the receiver, more of them than it has mover slots"""
    dims = (4, 4, 4)
    w = R.corner_world(dims)
    w.push(0, 0)
    sent = np.concatenate(w.pack(0))
    w.inject(1, sent)
    stopped = w.domains[1].species[0]["nm"]
    assert stopped > 4
    r = V.Engine(V.make_grid(*w.domains[1].args, **w.domains[1].kw))
    try:
        r.set_interpolator(w.domains[1].fi)
        sp = r.new_species(R.Q_M[0], 4 * R.N_HOT, 4)
        r.exchange_begin()
        m = Msg(len(sent)).write([len(sent)] * 2 + [0, 0], sent)
        r.exchange_inject(m.ptr, m.cap)
        with raises(V, "ran out of mover slots"):
            r.exchange_finish([])
        assert r.nm(sp) == 4
    finally:
        r.close()


def test_more_parked_movers_than_the_retry_buffer(V):
    """flag 16: 70 000 movers against a message of one -- more than the 65 536 a step may park"""
    n = 70000
    w = R.World("one_face", (4, 4, 4))
    w.domains[0].add_species(R.Q_M[0], R.through_face(71, n, (4, 4, 4), 3), n + 64)
    w.domains[1].add_species(R.Q_M[0], R.hot(72, (4, 4, 4), n=10, u=X.COLD), 64)
    with knobs("voxel"), Dev(V, w, "voxel") as dev:
        e = dev.engines[0]
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(0)
        m = dev.pack(0, [0, 0, 0, 1, 0, 0])[3]
        with raises(V, "found their message full"):
            e.exchange_finish([m.ptr])
        header, payload, guard = m.read()
        assert list(header) == [1, n, 0, 0] and np.all(guard == 0xFF)


def test_report():
    """(prints what the float comparisons of this file measured, as fractions of their bounds)"""
    if FLOAT_ERRORS:
        print("accumulator: worst error %.3f of the 2e-6 bound" % max(FLOAT_ERRORS.values()))
    if RHOB_ERRORS:
        print("rhob: worst error %.3f of the per-node bound" % max(RHOB_ERRORS.values()))
