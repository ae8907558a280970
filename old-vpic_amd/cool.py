"""The descriptor and the result of Engine.cool (include/vpic_hip.h: vpic_hip_species_cool).  tests/test_cool_ref.py holds
the descriptor's size and every member's offset against the compiler's."""
import collections
import ctypes as C


class CoolDesc(C.Structure):
    """vpic_hip_cool_t (include/vpic_hip.h)"""
    _fields_ = [("sync", C.c_double), ("ic", C.c_double), ("quantum", C.c_double), ("flags", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(CoolDesc) == 32
COOL_DRY = 1                                                                                   # VPIC_HIP_COOL_DRY
CoolResult = collections.namedtuple("CoolResult", "isum energy cell_isums stats")
