"""multiply_plain + rescale as one call, outside the kernels: the route table (tests/cpp/test_route_mulplain_rescale.cpp), the C ABI's new
name -- exported, bound, declared -- with the route operation's number, and, on the GPU, the plugin classes with
HipSchemeConfig::fuseMultiplyPlainRescale on and off (tests/cpp/test_hip_mulplain_rescale_runtime.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
NAME = "abc_hip_multiply_plain_rescale"


def _run(name, timeout=120):
    p = subprocess.run([os.path.join(RT, name)], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_route_table_of_mulplain_rescale():
    """route_mulplain_rescale over every ring 2^10..2^16, fp, mixed and 60-bit chains, every level and switch: fused exactly on the
    LDS-resident rescale, the strings, ops 6, 8 and 9 still unknown, and every route that existed gives the string it gave"""
    subprocess.check_call(["make", "-C", RT, "test_route_mulplain_rescale"], stdout=subprocess.DEVNULL)
    _run("test_route_mulplain_rescale")


def test_c_abi_symbol_of_multiply_plain_rescale(capi):
    """the call is exported, listed and declared; the route operation has its number and its name; the switch is documented"""
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    assert hasattr(lib, NAME), "missing export: " + NAME
    assert NAME in capi.SYMBOLS
    assert re.search(r"\bint " + NAME + r"\(abc_hip_ctx \*ctx, const uint64_t \*d_ct, const uint64_t \*d_plain, size_t plain_stride,\s+"
                     r"uint64_t \*d_out, int size, int nl, size_t count\);", header)
    assert callable(capi.Context.multiply_plain_rescale)
    m = re.search(r"#define ABC_HIP_ROUTE_MULTIPLY_PLAIN_RESCALE (\d+)", header)
    assert m and int(m.group(1)) == 10 == capi.Context.ROUTE_OPS["multiply_plain_rescale"]
    assert "kRouteMulPlainRescale = 10" in open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    assert not {6, 8, 9} & set(capi.Context.ROUTE_OPS.values())  # stay unassigned: the unknown operations of the host tests
    assert "ABC_HIP_NO_MULPLAIN_RESCALE_FUSION" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.gpu
def test_weight_products_behind_the_plugin_surface(capi):
    assert os.path.exists(capi.LIB_PATH), "libabc_hip.so missing: python -m abc_amd.build"
    subprocess.check_call(["make", "-C", RT, "test_hip_mulplain_rescale_runtime"], stdout=subprocess.DEVNULL)
    _run("test_hip_mulplain_rescale_runtime", timeout=300)
