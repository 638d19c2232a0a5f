"""The BFV plaintext-weighted sum behind the plugin surface: the interpreter's peephole on a recording fake backend
(tests/cpp/test_runtime_plain_sum.cpp, runs anywhere) and, on the GPU, HipSchemeConfig::fusePlainSum on against off word for word,
eagerly and as a recorded circuit (tests/cpp/test_hip_plain_sum_runtime.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")


def _run(name, timeout=120):
    subprocess.check_call(["make", "-C", RT, name], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(RT, name)], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_interpreter_peephole_for_sums_of_plain_products():
    """one plainSum per run when offered and asked for, operands in the order written; every other shape and backend as before"""
    _run("test_runtime_plain_sum")


def test_the_option_is_documented():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "fusePlainSum" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(RT, "PlainSumCapable.hpp"))


@pytest.mark.gpu
def test_plain_sum_behind_the_plugin_surface():
    from abc_amd import capi
    assert os.path.exists(capi.LIB_PATH), "libabc_hip.so missing: python -m abc_amd.build"
    _run("test_hip_plain_sum_runtime", timeout=300)
