"""The K-term plaintext sum with one rescale, outside the kernels: the route table (tests/cpp/test_route_plain_sum_rescale.cpp) and the
C ABI's two new names -- exported, bound, declared -- with their route operations' numbers and the new switch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")


def _run(name, timeout=120):
    p = subprocess.run([os.path.join(RT, name)], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_route_table_of_plain_sum_rescale():
    """route_plain_sum_rescale and route_matvec_bsgs_rescale over every ring 2^10..2^16, fp, mixed and 60-bit chains, every level and
    switch: fused exactly on the LDS-resident rescale without either switch, both strings, the terms the streaming kernel takes
    first, and every route that existed gives the string it gave"""
    subprocess.check_call(["make", "-C", RT, "test_route_plain_sum_rescale"], stdout=subprocess.DEVNULL)
    _run("test_route_plain_sum_rescale")


def test_c_abi_symbols_of_the_two_calls(capi):
    """the calls are exported, listed and declared; the route operations have their numbers and names; the switch is documented"""
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    route = open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    for name in ("abc_hip_multiply_plain_sum_rescale", "abc_hip_diag_matvec_bsgs_rescale"):
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.SYMBOLS
    assert re.search(r"\bint abc_hip_multiply_plain_sum_rescale\(abc_hip_ctx \*ctx, const uint64_t \*const \*h_ct, const uint64_t \*const \*h_plain, "
                     r"size_t plain_stride,\s+int n_terms, const uint64_t \*d_addend, uint64_t \*d_out, int size, int nl, size_t count\);", header)
    assert re.search(r"\bint abc_hip_diag_matvec_bsgs_rescale\(abc_hip_ctx \*ctx, const uint64_t \*d_in, const uint64_t \*d_diags, size_t diag_stride, "
                     r"const int \*h_baby,\s+int n_baby, const int \*h_giant, int n_giant, uint64_t \*d_out, int nl, size_t count\);", header)
    assert callable(capi.Context.multiply_plain_sum_rescale) and callable(capi.Context.diag_matvec_bsgs_rescale)
    for macro, number, key in (("PLAIN_SUM_RESCALE", 16, "plain_sum_rescale"), ("DIAG_MATVEC_BSGS_RESCALE", 17, "diag_matvec_bsgs_rescale")):
        m = re.search(r"#define ABC_HIP_ROUTE_%s (\d+)" % macro, header)
        assert m and int(m.group(1)) == number == capi.Context.ROUTE_OPS[key]
    assert "kRoutePlainSumRescale = 16, kRouteDiagMatvecBsgsRescale = 17" in route
    assert not {6, 8, 9, 11} & set(capi.Context.ROUTE_OPS.values())  # stay unassigned: the unknown operations of the host tests
    assert "ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION" in open(os.path.join(ROOT, "README.md")).read()
