"""The BFV plaintext-weighted sum with one inverse transform, outside the kernels: the route table and the grouping
(tests/cpp/test_route_bfv_plain_sum.cpp) and the C ABI's three new names -- exported, bound, declared, documented -- with the two
route operations' numbers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
NAMES = {"abc_hip_bfv_plain_to_ntt": 4, "abc_hip_bfv_multiply_plain_sum": 10, "abc_hip_bfv_diag_matvec_bsgs": 10}


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", RT, "test_route_bfv_plain_sum"], stdout=subprocess.DEVNULL)
    return RT


def test_route_table_of_bfv_plain_sum(built):
    """route_bfv_plain_sum on both sides of every condition; arena polynomials and groups; the matvec's string"""
    p = subprocess.run([os.path.join(built, "test_route_bfv_plain_sum")], capture_output=True, text=True, timeout=120)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_c_abi_symbols_of_bfv_plain_sum(capi):
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    for name, nargs in NAMES.items():
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
        assert re.search(r"\bint " + name + r"\(abc_hip_ctx \*ctx, ", header)
    comment = lambda name: header.split("int %s(" % name)[0].rsplit("/*", 1)[1]  # noqa: E731
    assert "Evaluator::transform_to_ntt(plain)" in comment("abc_hip_bfv_plain_to_ntt")
    for replaced in ("Evaluator::multiply_plain", ":159,:196", "Evaluator::add", ":92,:114"):
        assert replaced in comment("abc_hip_bfv_multiply_plain_sum")
    for said in ("rotate_rows", ":55,:60", ":159,:196", ":92,:114", "ALREADY ROTATED"):
        assert said in comment("abc_hip_bfv_diag_matvec_bsgs"), said
    for macro, number, key in (("ABC_HIP_ROUTE_BFV_PLAIN_SUM", 14, "bfv_plain_sum"), ("ABC_HIP_ROUTE_BFV_MATVEC_BSGS", 15, "bfv_matvec_bsgs")):
        m = re.search(r"#define %s (\d+)" % macro, header)
        assert m and int(m.group(1)) == number == capi.Context.ROUTE_OPS[key]
    assert re.search(r"#define ABC_HIP_CT_COEFF 0\b", header) and re.search(r"#define ABC_HIP_CT_NTT 1\b", header)
    assert "kRouteBfvPlainSum = 14, kRouteBfvMatvecBsgs = 15" in open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    assert not {6, 8, 9, 11} & set(capi.Context.ROUTE_OPS.values())  # stay unassigned: the unknown operations of the host tests
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "abc_hip_bfv_multiply_plain_sum" in open(os.path.join(ROOT, doc)).read(), doc
