"""CKKS plain operations whose public value is one number, behind the plugin classes (tests/cpp/test_hip_const_operands_runtime.cpp):
with HipSchemeConfig::constOperands on, the scalar travels as per-limb words (abc_hip_multiply_const_sum_rescale /
abc_hip_multiply_const_sum) -- word for word with dyadic scalars, the same decoded values with others; off -- the default -- the
encoded path.  The option and its note are in INTEGRATION.md."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")


def test_the_option_is_declared_off_by_default_and_documented():
    hpp = open(os.path.join(RT, "HipCiphertextFactory.hpp")).read()
    assert "bool constOperands = false;" in hpp and "constOperandCalls()" in hpp
    assert "constOperands" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.gpu
def test_const_operands_behind_the_plugin_surface(capi):
    assert os.path.exists(capi.LIB_PATH), "libabc_hip.so missing: python -m abc_amd.build"
    subprocess.check_call(["make", "-C", RT, "test_hip_const_operands_runtime"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(RT, "test_hip_const_operands_runtime")], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout
