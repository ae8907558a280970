"""Loader of libvpic_hip.so -- the HIP engine's C ABI (include/vpic_hip.h, include/vpic_hip_dropin.h).

The headers are the one statement of the ABI: signatures() reads every prototype out of them and lib() gives each function
the library exports its restype and argtypes from there.  Nothing here, in engine.py or in dropin.py restates a signature.

There is no CPU fallback: if the library is missing it is built with hipcc; if that fails, or no
HIP device is present when an engine is created, the error is raised to the caller.
"""
import ctypes as C
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libvpic_hip.so")
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
_lib = None

# the closed map of the ABI's scalar types; whatever carries a * or [..], and a typedef'd function pointer, is a c_void_p
_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "uint32_t": C.c_uint32, "unsigned": C.c_uint32, "int64_t": C.c_int64,
            "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every `ret vpic_hip_name(args);` in the text of a header.  A type outside the map
    raises a TypeError that names the function: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    fn_ptrs = set(re.findall(r"typedef[^;{}]*\(\s*\*\s*(\w+)\s*\)", text))

    def ctype(decl, fn, ret=False):
        words = [w for w in re.sub(r"\*|\[\w*\]", " ", decl).split() if w != "const"]
        if "*" in decl or "[" in decl:
            return C.c_char_p if ret and words == ["char"] else C.c_void_p
        if not ret and len(words) == 2:
            words.pop()                                              # the parameter's name
        if ret and words == ["void"]:
            return None
        if len(words) == 1 and words[0] in fn_ptrs:
            return C.c_void_p
        if len(words) != 1 or words[0] not in _SCALARS:
            raise TypeError(f"{fn}: no ctypes class for `{' '.join(decl.split())}`")
        return _SCALARS[words[0]]

    table = {}
    for ret, fn, args in re.findall(r"([^;{}()]*?)\b(vpic_hip_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() == "void" else args.split(",")
        table[fn] = (ctype(ret, fn, ret=True), [ctype(a, fn) for a in args])
    return table


def signatures(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return parse_prototypes(f.read())


SIGNATURES = {h: signatures(h) for h in ("vpic_hip.h", "vpic_hip_dropin.h")}
EXPORTS = sorted(SIGNATURES["vpic_hip.h"])


def build(force=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j4"])
    if not os.path.exists(SO):
        raise RuntimeError("building libvpic_hip.so failed")
    return SO


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE)]
    return any(os.path.getmtime(s) > t for s in srcs)


def _bind(L):
    """The one place that declares signatures.  A function the loaded library lacks is skipped: an older build of the ABI
    under VPIC_HIP_LIB still binds (tools/wall_time.py times one)."""
    for table in SIGNATURES.values():
        for name, (res, args) in table.items():
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = res, args


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if _stale() and os.path.exists("/opt/rocm/bin/hipcc") and not os.environ.get("VPIC_HIP_NO_REBUILD"):
        build()
    try:
        # torch ships its own libamdhip64 (same SONAME): when both live in one process the HIP
        # runtime must be loaded once, so let torch load it first.
        import torch  # noqa: F401
    except Exception:
        pass
    # VPIC_HIP_LIB: load another build of the same ABI (A/B timing of kernel variants on one GPU box)
    L = C.CDLL(os.environ.get("VPIC_HIP_LIB", SO))
    _bind(L)
    _lib = L
    return L
