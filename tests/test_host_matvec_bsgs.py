"""The plaintext multiply-accumulate sum and the baby-step giant-step matvec, outside the kernels: the route table
(tests/cpp/test_route_matvec_bsgs.cpp) and the C ABI's three new names -- exported, bound, declared, documented -- with the route
operation's number and the switch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
NAMES = {"abc_hip_multiply_plain_sum": 10, "abc_hip_rotate_plain": 6, "abc_hip_diag_matvec_bsgs": 11}


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", RT, "test_route_matvec_bsgs"], stdout=subprocess.DEVNULL)
    return RT


def test_route_table_of_matvec_bsgs(built):
    """route_matvec_bsgs over every ring 2^10..2^16, chain, level and switch; the groups; every other route as it was"""
    p = subprocess.run([os.path.join(built, "test_route_matvec_bsgs")], capture_output=True, text=True, timeout=120)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_c_abi_symbols_of_plain_sum_and_bsgs(capi):
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    for name, nargs in NAMES.items():
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
        assert re.search(r"\bint " + name + r"\(abc_hip_ctx \*ctx, ", header)
    comment = lambda name: header.split("int %s(" % name)[0].rsplit("/*", 1)[1]  # noqa: E731
    for replaced in ("Evaluator::multiply_plain", ":159,:196", "Evaluator::add", ":92,:114"):
        assert replaced in comment("abc_hip_multiply_plain_sum")
    assert ":55,:60" in comment("abc_hip_rotate_plain")
    for said in ("rotate_rows", ":55,:60", ":159,:196", ":92,:114", "rot_plain(diag, -g)", "ALREADY ROTATED"):
        assert said in comment("abc_hip_diag_matvec_bsgs"), said
    m = re.search(r"#define ABC_HIP_ROUTE_DIAG_MATVEC_BSGS (\d+)", header)
    assert m and int(m.group(1)) == 13 == capi.Context.ROUTE_OPS["diag_matvec_bsgs"]
    assert "kRouteDiagMatvecBsgs = 13" in open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    assert not {6, 8, 9, 11} & set(capi.Context.ROUTE_OPS.values())  # stay unassigned: the unknown operations of the host tests
    for doc in ("README.md", "DESIGN.md"):
        assert "ABC_HIP_NO_PLAIN_MAC_SUM" in open(os.path.join(ROOT, doc)).read(), doc
    assert "abc_hip_diag_matvec_bsgs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
