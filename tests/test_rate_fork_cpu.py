"""CPU: the side-stream entry points of the coders' rate branch (tdvc_rate_branch / tdvc_rate_join, ABI 19) are declared, bound and laid
out as the header says, and what they can decide on the host they decide without a device."""
import ctypes as C
import os
import re

from tdvc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tdvc_hip.h")).read(), flags=re.S)
    for sym in ("tdvc_rate_branch", "tdvc_rate_join"):
        assert re.search(rf"\bint {sym}\s*\(", header), f"{sym} is not declared in include/tdvc_hip.h"
        assert sym in L.SIGNATURES and hasattr(L.lib(), sym)
    assert "tdvc_rate_chain" in header and L.lib().tdvc_abi_version() >= 19
    assert L.SIGNATURES["tdvc_rate_branch"] == (C.c_int, [C.POINTER(L.RateChainDesc), C.c_void_p])
    assert L.SIGNATURES["tdvc_rate_join"] == (C.c_int, [C.c_void_p, C.c_int])
    for name, value in (("TDVC_RATE_MAX_CONVS", L.RATE_MAX_CONVS), ("TDVC_RATE_BRANCHES", L.RATE_BRANCHES)):
        assert re.search(rf"#define {name} {value}\b", header)


def test_the_chain_descriptor_has_the_headers_layout():
    # the numbers csrc/lib.cpp static_asserts on the header
    assert C.sizeof(L.RateChainDesc) == 224 and L.RateChainDesc.bits.offset == 208
    assert L.RateChainDesc.z.offset == 16 and L.RateChainDesc.y.offset == 128 and L.RateChainDesc._fields_[-1][0] == "split"


def test_a_join_with_nothing_pending_is_a_no_op_without_a_device():
    lib = L.lib()
    for which in range(L.RATE_BRANCHES):
        assert lib.tdvc_rate_join(None, which) == 0
        assert lib.tdvc_rate_join(None, which) == 0           # twice
        assert lib.tdvc_rate_join(0x1000, which) == 0         # a stream that never forked
    assert lib.tdvc_rate_join(None, L.RATE_BRANCHES) != 0 and b"slot" in lib.tdvc_last_error()
    assert lib.tdvc_rate_join(None, -1) != 0


def test_a_bad_chain_is_refused_before_anything_touches_a_device():
    lib = L.lib()
    assert lib.tdvc_rate_branch(None, None) != 0 and b"null" in lib.tdvc_last_error()
    convs = (L.ConvDesc * 1)()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    fm = L.FMapDesc(p, 1, 1, 1, 8, 8, 8, L.F32)

    def chain(nconvs=1, eb_after=1, which=0):
        return L.RateChainDesc(convs, nconvs, eb_after, fm, fm, p, p, 1, 1, p, fm, fm, p, which, 0)
    for bad in (chain(nconvs=0), chain(nconvs=L.RATE_MAX_CONVS + 1), chain(eb_after=0), chain(eb_after=2), chain(which=-1),
                chain(which=L.RATE_BRANCHES)):
        assert lib.tdvc_rate_branch(bad, None) != 0 and lib.tdvc_last_error().startswith(b"tdvc_rate_branch:")
