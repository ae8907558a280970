"""The calls whose signatures Python never declared before the binding took every one of them from the headers
(old-vpic_amd/_lib.py: signatures): a device pointer comes back whole from vpic_hip_device_alloc and goes into the copies as
a plain integer with a size_t beside it, and the pack / unpack calls that had no declared types take a torch buffer's data_ptr()
as it is -- with the same result as the pointer wrapped in ctypes.c_void_p by hand, which is how they had to be called."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DIMS = (8, 6, 4)


@pytest.fixture(scope="module")
def V():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


@pytest.fixture()
def engine(V):
    """a domain all of whose faces are shared with another one, so that every direction has a message"""
    nx, ny, nz = DIMS
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.3), fbc=[1] * 6, pbc=[1] * 6, rank=0))
    yield e
    e.close()


def test_device_alloc_and_the_copies_through_lib(V, engine):
    l, h = V.lib(), engine._h
    dev = l.vpic_hip_device_alloc(h, 4096)
    assert isinstance(dev, int) and dev != 0, l.vpic_hip_last_error()
    assert C.c_void_p(dev).value == dev                      # the whole 64-bit address: the copies below go through it
    try:
        pattern = np.random.default_rng(5).integers(0, 256, 4096, dtype=np.uint8)
        back = np.zeros_like(pattern)
        assert l.vpic_hip_copy_from_host(h, dev, pattern.ctypes.data, pattern.nbytes) == 0, l.vpic_hip_last_error()
        assert l.vpic_hip_copy_to_host(h, back.ctypes.data, dev, back.nbytes) == 0, l.vpic_hip_last_error()
        engine.sync()
        assert np.array_equal(back, pattern)
    finally:
        l.vpic_hip_device_free(h, dev)


def random_words(rng, dtype, n):
    """n records whose float words are small random numbers (the two-byte material indices of a field stay 0)"""
    a = np.zeros(n, dtype)
    for name in dtype.names:
        if dtype[name].base == np.float32:
            a[name] = rng.uniform(-1.0, 1.0, a[name].shape).astype(np.float32)
    return a


@pytest.mark.parametrize("family", ["rho", "hydro", "message"])
def test_pack_and_unpack_take_a_plain_data_ptr(V, engine, family):
    import torch
    e, L = engine, V.layout
    rng = np.random.default_rng(11)
    count, pack, unpack = {"rho": (e.rho_count, e.pack_rho, e.unpack_rho),
                           "hydro": (e.hydro_count, e.pack_hydro, e.unpack_hydro),
                           "message": (lambda d: e.message_count(0, d), lambda d, p: e.pack_message(0, d, p),
                                       lambda d, p: e.unpack_message(0, d, p))}[family]
    if family == "hydro":
        start, put, get = random_words(rng, L.hydro_t, e.nv), e.set_hydro, e.get_hydro
    else:
        start, put, get = random_words(rng, L.field_t, e.nv), e.set_fields, e.get_fields
    for d in range(6):
        n = count(d)
        assert n > 0, (family, d)
        # pack: the same array into two buffers, the pointer once as an integer and once wrapped by hand
        put(start)
        packed = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        pack(d, packed[0].data_ptr())
        pack(d, C.c_void_p(packed[1].data_ptr()))
        e.sync()
        words = [t.cpu().numpy().view(np.uint32) for t in packed]
        assert words[0].any() and np.array_equal(words[0], words[1]), (family, d)
        # unpack: the same message into the same array, likewise
        msg = torch.from_numpy(rng.uniform(-1.0, 1.0, n).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        planes = []
        for ptr in (msg.data_ptr(), C.c_void_p(msg.data_ptr())):
            put(start)
            unpack(d, ptr)
            e.sync()
            planes.append(get())
        assert planes[0].tobytes() == planes[1].tobytes(), (family, d)
        assert planes[0].tobytes() != start.tobytes(), (family, d, "unpack left the array as it was")
