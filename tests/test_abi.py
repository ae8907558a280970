"""CPU-side checks of the C ABI: the library builds, loads, and exports every function the headers
in include/ declare; the Python-side struct mirrors have the reference's sizes; with no GPU the
engine refuses loudly instead of falling back to anything."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vpic_hip_\w+)\s*\(", text)) - {"vpic_hip_engine"})


@pytest.mark.parametrize("header", ["vpic_hip.h", "vpic_hip_dropin.h"])
def test_library_exports_every_declared_symbol(header):
    V = importlib.import_module("old-vpic_amd")
    l = V.lib()
    names = [n for n in declared_functions(header) if not n.endswith("_t")]
    assert len(names) > 10
    missing = [n for n in names if not hasattr(l, n)]
    assert not missing, missing


def test_python_lists_match_headers():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    drop = importlib.import_module("old-vpic_amd.dropin")
    assert sorted(lib_mod.EXPORTS) == [n for n in declared_functions("vpic_hip.h")]
    assert sorted(drop.DROPIN_EXPORTS) == [n for n in declared_functions("vpic_hip_dropin.h")]


HEADERS = ["vpic_hip.h", "vpic_hip_dropin.h"]
# what the compiler says of a type: void, ptr, or i / u / f with its size in bytes
CLASSIFY = """#include <cstdio>
#include <type_traits>
#include "%s"
template <class T> void cls() {
  if constexpr (std::is_void<T>::value) std::printf(" void");
  else if constexpr (std::is_pointer<T>::value) std::printf(" ptr");
  else std::printf(" %%c%%d", std::is_floating_point<T>::value ? 'f' : std::is_signed<T>::value ? 'i' : 'u', (int)sizeof(T));
}
template <class R, class... A> void sig(const char *name, R (*)(A...)) {
  std::printf("%%s", name); cls<R>(); (cls<A>(), ...); std::printf("\\n");
}
int main() {
%s  return 0;
}
"""


def ctypes_class(t):
    """the same of a ctypes class, from its own type code and size"""
    if t is None:
        return "void"
    kind = {"P": "ptr", "z": "ptr", "f": "f", "d": "f", "i": "i", "l": "i", "q": "i", "I": "u", "L": "u", "Q": "u"}[t._type_]
    return kind if kind == "ptr" else kind + str(C.sizeof(t))


@pytest.fixture(scope="module")
def compiled_signatures(tmp_path_factory):
    """{header: {name: [return class, parameter class ...]}} as the host compiler derives them from the header, for every
    function declared_functions() finds: decltype(&name) is unevaluated, so nothing is linked"""
    out = {}
    for header in HEADERS:
        d = tmp_path_factory.mktemp("abi")
        calls = "".join('  sig("%s", static_cast<decltype(&%s)>(nullptr));\n' % (n, n) for n in declared_functions(header))
        (d / "sig.cpp").write_text(CLASSIFY % (header, calls))
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               str(d / "sig.cpp"), "-o", str(d / "sig")])
        lines = subprocess.run([str(d / "sig")], capture_output=True, text=True, check=True).stdout.splitlines()
        out[header] = {line.split()[0]: line.split()[1:] for line in lines}
    return out


@pytest.mark.parametrize("header", HEADERS)
def test_parsed_signatures_match_the_compiler(header, compiled_signatures):
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    table = lib_mod.signatures(header)
    want = compiled_signatures[header]
    assert sorted(want) == declared_functions(header) == sorted(table)
    for name in declared_functions(header):
        res, args = table[name]
        assert [ctypes_class(res)] + [ctypes_class(a) for a in args] == want[name], name
        if res is C.c_char_p:                                  # the one return that is read as a string, not as an address
            assert name == "vpic_hip_last_error"


@pytest.mark.parametrize("header", HEADERS)
def test_every_exported_function_is_bound(header, compiled_signatures):
    V = importlib.import_module("old-vpic_amd")
    l = V.lib()
    bound = 0
    for name in declared_functions(header):
        if not hasattr(l, name):
            continue
        f, want = getattr(l, name), compiled_signatures[header][name]
        assert f.argtypes is not None and len(f.argtypes) == len(want) - 1, name
        assert ctypes_class(f.restype) == want[0], name
        bound += 1
    assert bound > 10


def test_a_type_outside_the_map_is_refused():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    ok = lib_mod.parse_prototypes("int vpic_hip_fine(const float *a, int64_t n);\nvoid *vpic_hip_more(void);\n")
    assert ok == {"vpic_hip_fine": (C.c_int, [C.c_void_p, C.c_int64]), "vpic_hip_more": (C.c_void_p, [])}
    for text, name in (("int vpic_hip_fine(int a);\nint vpic_hip_odd(long double x);\n", "vpic_hip_odd"),
                       ("int vpic_hip_fine(int a);\nshort vpic_hip_short(int a);\n", "vpic_hip_short"),
                       ("int vpic_hip_fine(int a);\nint vpic_hip_by_value(vpic_hip_grid_t g);\n", "vpic_hip_by_value")):
        with pytest.raises(TypeError, match=name):
            lib_mod.parse_prototypes(text)


def test_field_advance_method_table():
    """vpic_hip_ref_field_advance_methods: the 20 slots of field_advance_methods_t in the reference's order
    (field_advance.h:185-302), every one an entry point of this library."""
    V = importlib.import_module("old-vpic_amd")
    drop = importlib.import_module("old-vpic_amd.dropin")
    l = V.lib()
    table = (C.c_void_p * 20).in_dll(l, "vpic_hip_ref_field_advance_methods")
    assert len(drop.FIELD_ADVANCE_SLOTS) == 20
    for k, name in enumerate(drop.FIELD_ADVANCE_SLOTS):
        assert table[k] == C.cast(getattr(l, "vpic_hip_ref_" + name), C.c_void_p).value, name


def test_allocation_slots_and_material_coefficients():
    """new_field / new_material_coefficients / ... (host memory only: no GPU needed): aligned, zeroed, and the
    coefficient records of the reference for the K13 materials, bit for bit."""
    V = importlib.import_module("old-vpic_amd")
    drop = importlib.import_module("old-vpic_amd.dropin")
    L = importlib.import_module("old-vpic_amd.layout")
    import numpy as np
    l = V.lib()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "kernels.npz"))
    nx, ny, nz = [int(v) for v in gold["k1_dims"]]
    g = drop.reference_grid(nx, ny, nz, 6.0, 5.0, 4.0, np.float32(0.3))

    class Material(C.Structure):
        pass
    Material._fields_ = [("id", C.c_uint16)] + [(n, C.c_float) for n in "epsx epsy epsz mux muy muz sigmax sigmay sigmaz zetax zetay zetaz".split()] + \
                        [("next", C.POINTER(Material)), ("name", C.c_char * 8)]
    head = None
    for k, props in enumerate(gold["k13_props"]):             # new_material pushes on the front of the list
        m = Material(k, *[float(v) for v in props], 0, 0, 0)
        m.name = b"m%d" % k
        if head is not None:
            m.next = C.pointer(head)
        head = m
    mc = l.vpic_hip_ref_new_material_coefficients(C.byref(g), C.byref(head))
    table = np.frombuffer((C.c_char * (3 * L.material_coefficient_t.itemsize)).from_address(mc), L.material_coefficient_t)
    want = gold["k13per_mc"]
    for n in want.dtype.names:
        assert np.array_equal(table[n].view(np.uint32), want[n].view(np.uint32)), n
    l.vpic_hip_ref_delete_material_coefficients(C.c_void_p(mc))
    nv = (nx + 2) * (ny + 2) * (nz + 2)
    for name, rec in (("field", L.field_t), ("hydro", L.hydro_t), ("interpolator", L.interpolator_t), ("accumulators", L.accumulator_t)):
        ptr = getattr(l, "vpic_hip_ref_new_" + name)(C.byref(g))
        assert ptr % 128 == 0
        assert not np.frombuffer((C.c_char * (nv * rec.itemsize)).from_address(ptr), np.uint8).any()
        getattr(l, "vpic_hip_ref_delete_" + name)(C.c_void_p(ptr))


def test_struct_mirrors():
    drop = importlib.import_module("old-vpic_amd.dropin")
    eng = importlib.import_module("old-vpic_amd.engine")
    assert C.sizeof(drop.RefGrid) == 240          # grid_t, src/grid/grid.h:112-167
    assert drop.RefGrid.neighbor.offset == 200 and drop.RefGrid.bc.offset == 84
    assert C.sizeof(eng.GridDesc) == 4 * (4 + 6 + 3 + 12 + 1)


# mirror (old-vpic_amd.<module>.<name>) -> the header's struct and, where a mirror's field is named otherwise, {field: C member}
MIRRORS = {"engine.GridDesc": ("vpic_hip_grid_t", {}), "engine.SpectrumParams": ("vpic_hip_spectrum_t", {}),
           "engine.DistAxis": ("vpic_hip_dist_axis_t", {}), "engine.DistRange": ("vpic_hip_dist_range_t", {}),
           "engine.DistDesc": ("vpic_hip_dist_t", {}), "engine.DistValue": ("vpic_hip_dist_value_t", {}),
           "engine.SelectDesc": ("vpic_hip_select_t", {}), "engine.CollisionDesc": ("vpic_hip_collision_t", {}),
           "dropin.RefGrid": ("vpic_grid_t", {}),
           "layout.particle_t": ("vpic_particle_t", {}), "layout.particle_mover_t": ("vpic_particle_mover_t", {}),
           "layout.particle_injector_t": ("vpic_particle_injector_t", {}), "layout.interpolator_t": ("vpic_interpolator_t", {}),
           "layout.accumulator_t": ("vpic_accumulator_t", {}), "layout.hydro_t": ("vpic_hydro_t", {}),
           "layout.field_t": ("vpic_field_t", {}), "layout.material_coefficient_t": ("vpic_material_coefficient_t", {}),
           "layout.wall_tally_t": ("vpic_hip_wall_tally_t", {}), "layout.wall_record_t": ("vpic_hip_wall_record_t", {}),
           "layout.load_t": ("vpic_hip_load_t", {})}


def mirror_layout(m):
    """(size, {field: offset}) of a ctypes.Structure class or a numpy dtype"""
    if isinstance(m, type) and issubclass(m, C.Structure):
        return C.sizeof(m), {name: getattr(m, name).offset for name, *_ in m._fields_}
    return m.itemsize, {name: m.fields[name][1] for name in m.names}


def test_struct_mirrors_against_the_compiler(tmp_path):
    """every mirror -- the ctypes.Structure classes of engine.py and dropin.py, the numpy dtypes of layout.py (none may be
    added without a row above) -- has the size of the header's struct and every field at the offset of its member, as a C
    program generated from the table prints them"""
    mods = {n: importlib.import_module("old-vpic_amd." + n) for n in ("engine", "dropin", "layout")}
    import numpy as np
    for mod_name, mod in mods.items():
        for name, obj in vars(mod).items():
            if (isinstance(obj, type) and issubclass(obj, C.Structure) and obj.__module__ == mod.__name__) or isinstance(obj, np.dtype):
                assert mod_name + "." + name in MIRRORS, name
    layouts = {key: mirror_layout(getattr(mods[key.split(".")[0]], key.split(".")[1])) for key in MIRRORS}
    body = ""
    for key, (ctype, names) in MIRRORS.items():
        body += '  printf("%s %%zu\\n", sizeof(%s));\n' % (key, ctype)
        for field in layouts[key][1]:
            body += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (key, field, ctype, names.get(field, field))
    src = '#include <stdio.h>\n#include "vpic_hip_dropin.h"\nint main(void) {\n%s  return 0;\n}\n' % body
    exe = str(tmp_path / "vpic_hip_struct_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    want = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert len(want) == sum(1 + len(fields) for _, fields in layouts.values())
    for key, (size, fields) in layouts.items():
        assert size == int(want[key]), key
        for field, offset in fields.items():
            assert offset == int(want[key + "." + field]), (key, field)


def test_headers_compile_as_c(tmp_path):
    src = '#include "vpic_hip_dropin.h"\nint main(void){return sizeof(vpic_grid_t)==240?0:1;}\n'
    exe = str(tmp_path / "vpic_hip_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    subprocess.check_call([exe])


def test_no_gpu_means_loud_failure():
    V = importlib.import_module("old-vpic_amd")
    if V.lib().vpic_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(V.VpicHipError, match="no CPU fallback"):
        V.Engine(V.make_grid(4, 4, 4, 4.0, 4.0, 4.0, 0.3))


def test_reference_production_deck_compiles_against_the_hip_host(tmp_path):
    """The reference's reconnection deck (decks/trecon-part/turbulence.cxx with its tracer.cxx / energy.cxx /
    config.h, 1.8 k lines, UNCHANGED) compiles and links against old-vpic_amd/host: every name it uses --
    DumpParameters, FileIO, global_header, field_dump / hydro_dump, the L3 calls of its tracer macros,
    mp_elapsed, turnstiles, dump_restart ... -- exists with the reference's signature.  Build check only
    (the deck lives in the reference tree, which is not on the GPU box; oracle/decks/sheet4.cxx is the
    deck of that family that RUNS in the GPU tests)."""
    import os, subprocess
    deck = "/root/reference/decks/trecon-part/turbulence.cxx"
    if not os.path.exists(deck) or not os.path.exists("/opt/conda/include/mpi.h"):
        pytest.skip("reference tree or MPI headers not present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    __import__("importlib").import_module("old-vpic_amd").build()
    out = str(tmp_path / "trecon")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "old-vpic_amd", "host"), "deck", "MPI=1", "DECK=" + deck, "OUT=" + out])
    assert os.path.getsize(out + ".hip.exe") > 0


def test_push_launch_plan_beyond_two_to_the_thirty():
    """advance_p addresses particles by 32-bit byte offsets inside a launch, so a species beyond 2^30 particles is pushed in
    segments (vpic_hip_push_plan: host arithmetic, no GPU needed): they tile [0, np) without gaps or overlap, start on
    workgroup chunk boundaries, and no byte offset inside one reaches 2^32."""
    import ctypes as C
    V = importlib.import_module("old-vpic_amd")
    lib = V.lib()
    for npart, iters in ((2 ** 30 + 4096, 6), (2 ** 30, 12), (2 ** 31 - 8192, 64), (1000, 1), (2 ** 30 + 1, 7)):
        start, count, grid = (C.c_int64 * 4)(), (C.c_int32 * 4)(), (C.c_uint32 * 4)()
        n = lib.vpic_hip_push_plan(C.c_int64(npart), iters, start, count, grid, 4)
        assert n >= 1
        chunk = 256 * iters
        at = 0
        for k in range(n):
            assert start[k] == at and start[k] % chunk == 0
            assert 0 < count[k] <= 2 ** 30
            last = count[k] - 1 if count[k] % 64 == 0 else count[k] + 62                  # highest index a lane of the last pass addresses
            assert last * 4 < 2 ** 32                                                     # 32-bit byte offsets
            assert grid[k] * chunk >= count[k] and grid[k] % 8 == 0 and (grid[k] - 8) * chunk < count[k]
            at += count[k]
        assert at == npart
        assert (n == 1) == (npart <= 2 ** 30 and (npart % 64 == 0 or npart <= 2 ** 30 - 64))
    assert lib.vpic_hip_push_plan(C.c_int64(-1), 6, start, count, grid, 4) < 0
