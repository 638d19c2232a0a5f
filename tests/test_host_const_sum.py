"""Scalar constants and polynomial evaluation, outside the kernels: the route table (tests/cpp/test_route_const_sum.cpp) and the C
ABI's new names -- exported, bound, declared -- with their route operations' numbers and the new switch."""
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


def test_route_table_of_const_sum_and_poly_eval():
    """route_const_mac_sum, route_const_sum_rescale, string 18 and string 19 over every ring 2^10..2^16, fp, mixed and 60-bit chains, every
    level and switch: fused exactly where the LDS-resident rescale runs, the sum has 1 .. 4 terms all at nl and the measured rule or
    ABC_HIP_CONST_SUM_RESCALE_FUSED says so; never for a raised term, five terms, N >= 2^15, NO_FUSED or NO_ISPLIT on a wide chain; the
    new switches change no route that existed"""
    subprocess.check_call(["make", "-C", RT, "test_route_const_sum"], stdout=subprocess.DEVNULL)
    _run("test_route_const_sum")


def test_c_abi_symbols_of_the_new_calls(capi):
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    route = open(os.path.join(ROOT, "abc_amd", "csrc", "abc_route.hpp")).read()
    for name in ("abc_hip_ckks_const_words", "abc_hip_multiply_const_sum", "abc_hip_multiply_const_sum_rescale", "abc_hip_ckks_poly_eval",
                 "abc_hip_ckks_poly_eval_depth"):
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.SYMBOLS
    assert re.search(r"\bint abc_hip_ckks_const_words\(abc_hip_ctx \*ctx, double value, double scale, int nl, uint64_t \*h_words\);", header)
    for name in ("abc_hip_multiply_const_sum", "abc_hip_multiply_const_sum_rescale"):
        assert re.search(r"\bint %s\(abc_hip_ctx \*ctx, const uint64_t \*const \*h_ct, const int \*h_ct_nl, const uint64_t \*h_weights,\s+int n_terms,\s+"
                         r"const uint64_t \*h_const, const uint64_t \*d_addend, uint64_t \*d_out, int size, int nl,\s+size_t count\);" % name, header), name
    assert re.search(r"\bint abc_hip_ckks_poly_eval\(abc_hip_ctx \*ctx, const uint64_t \*d_x, double x_scale, const double \*h_coeffs, int degree, double out_scale,\s+"
                     r"uint64_t \*d_out, int nl, size_t count\);", header)
    for method in ("const_words", "multiply_const_sum", "multiply_const_sum_rescale", "multiply_const", "add_const", "poly_eval", "poly_eval_depth"):
        assert callable(getattr(capi.Context, method))
    for macro, number, key in (("CONST_SUM_RESCALE", 18, "const_sum_rescale"), ("POLY_EVAL", 19, "poly_eval")):
        m = re.search(r"#define ABC_HIP_ROUTE_%s (\d+)" % macro, header)
        assert m and int(m.group(1)) == number == capi.Context.ROUTE_OPS[key]
    assert "kRouteConstSumRescale = 18, kRoutePolyEval = 19" in route
    assert not {6, 8, 9, 11} & set(capi.Context.ROUTE_OPS.values())  # stay unassigned: the unknown operations of the host tests
    assert "ABC_HIP_NO_CONST_MAC_SUM" in open(os.path.join(ROOT, "README.md")).read()
