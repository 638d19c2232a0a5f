"""Sums of ciphertext products with one relinearisation, outside the kernels: the route table (tests/cpp/test_route_mul_sum.cpp), the
interpreter's peephole on a recording fake backend (tests/cpp/test_runtime_mul_sum.cpp), the C ABI's two new names -- exported,
bound, declared, documented -- with the route operation's number, and, on the GPU, lazy relinearisation behind the plugin surface with
HipSchemeConfig::lazyRelinearize on and off (tests/cpp/test_hip_mul_sum_runtime.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
NAMES = ("abc_hip_multiply_sum", "abc_hip_mul_sum_relin")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", RT, "test_route_mul_sum", "test_runtime_mul_sum"], stdout=subprocess.DEVNULL)
    return RT


def _run(built, name, timeout=120):
    p = subprocess.run([os.path.join(built, name)], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_route_table_of_mul_sum(built):
    """route_mul_sum over every ring 2^10..2^16, scheme, chain, level and switch; the groups; every other route as it was"""
    _run(built, "test_route_mul_sum")


def test_interpreter_peephole_for_sums_of_products(built):
    """one mulSum per run of products when offered and asked for; every other shape, and every other backend, as before"""
    _run(built, "test_runtime_mul_sum")


def test_c_abi_symbols_of_mul_sum(capi):
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 7
        assert re.search(r"\bint " + name + r"\(abc_hip_ctx \*ctx, const uint64_t \*const \*h_a,", header)
    for replaced in ("Evaluator::multiply", "Evaluator::add", "Evaluator::relinearize_inplace"):
        assert replaced in header.split("int abc_hip_multiply_sum(")[0].rsplit("/*", 1)[1]
    m = re.search(r"#define ABC_HIP_ROUTE_MUL_SUM_RELIN (\d+)", header)
    assert m and int(m.group(1)) == 12 == capi.Context.ROUTE_OPS["mul_sum_relin"]
    assert "kRouteMulSumRelin = 12" in open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    assert not {6, 8, 9, 11} & set(capi.Context.ROUTE_OPS.values())  # stay unassigned: the unknown operations of the host tests
    for doc in ("README.md", "DESIGN.md"):
        assert "ABC_HIP_NO_TENSOR_SUM" in open(os.path.join(ROOT, doc)).read(), doc
    assert "lazyRelinearize" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.gpu
def test_lazy_relinearisation_behind_the_plugin_surface(built):
    from abc_amd import capi
    assert os.path.exists(capi.LIB_PATH), "libabc_hip.so missing: python -m abc_amd.build"
    subprocess.check_call(["make", "-C", RT, "test_hip_mul_sum_runtime"], stdout=subprocess.DEVNULL)
    _run(built, "test_hip_mul_sum_runtime", timeout=300)
