"""Fused rotate, multiply-plain and add outside the kernels: the route table (tests/cpp/test_route_rotate_mac.cpp) and the C ABI's
three new names -- exported, bound, declared -- with the route operation's number."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
NAMES = ("abc_hip_rotate_mac_plain", "abc_hip_apply_galois_mac_plain", "abc_hip_diag_matvec")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", RT, "test_route_rotate_mac"], stdout=subprocess.DEVNULL)
    return RT


def test_route_table_of_rotate_mac(built):
    """route_rotate_mac over every ring 2^10..2^16, scheme, level and switch: fused exactly under the documented rule, the strings,
    and every route that existed gives the string it gave"""
    p = subprocess.run([os.path.join(built, "test_route_rotate_mac")], capture_output=True, text=True, timeout=120)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_c_abi_symbols_of_rotate_mac_plain(capi):
    """the three calls are exported, bound and declared; the route operation has its number and its name"""
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 9
        assert re.search(r"\bint " + name + r"\(abc_hip_ctx \*ctx,", header)
    for method in ("rotate_mac_plain", "apply_galois_mac_plain", "diag_matvec"):
        assert callable(getattr(capi.Context, method))
    m = re.search(r"#define ABC_HIP_ROUTE_ROTATE_MAC_PLAIN (\d+)", header)
    assert m and int(m.group(1)) == 7 == capi.Context.ROUTE_OPS["rotate_mac_plain"]
    route_hpp = open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    assert "kRouteRotateMacPlain = 7" in route_hpp
    # the numbers that existed keep their operations
    assert {k: v for k, v in capi.Context.ROUTE_OPS.items() if v < 6} == {
        "mul_relin": 0, "keyswitch": 1, "relinearize": 1, "rotate": 2, "rescale": 3, "multiply": 4, "rotate_add": 5}
