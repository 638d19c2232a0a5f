"""Fused rotate-and-add outside the kernels: the route table (tests/cpp/test_route_rotate_add.cpp), the interpreter's peephole on a
recording fake backend (tests/cpp/test_runtime_rotate_add.cpp) and, on the GPU, the vectorizer's trees behind the plugin surface with
HipSchemeConfig::fuseRotateAdd on and off (tests/cpp/test_hip_rotate_add_runtime.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
DRIVERS = ("test_route_rotate_add", "test_runtime_rotate_add", "test_hip_rotate_add_runtime")


@pytest.fixture(scope="module")
def built():
    from abc_amd import capi
    assert os.path.exists(capi.LIB_PATH), "libabc_hip.so missing: python -m abc_amd.build"
    subprocess.check_call(["make", "-C", RT] + list(DRIVERS), stdout=subprocess.DEVNULL)
    return RT


def _run(built, name, timeout=60):
    p = subprocess.run([os.path.join(built, name)], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout


def test_route_table_of_rotate_add(built):
    """route_rotate_add over every shape and switch test_route.cpp names: fused exactly under the documented rule, the strings"""
    _run(built, "test_route_rotate_add")


def test_interpreter_peephole_on_a_recording_backend(built):
    """`lhs +++ rotate(v, k)` is one fused call where the ciphertext offers RotateAddCapable; other shapes and malformed rotate
    calls issue the operations, and throw the texts, they always did"""
    _run(built, "test_runtime_rotate_add")


def test_c_abi_symbols_of_rotate_add(capi):
    """the three calls are exported, bound and declared; route op 5 has its name"""
    lib = capi.lib()
    for name in ("abc_hip_rotate_add", "abc_hip_apply_galois_add", "abc_hip_rotate_sum"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.Context.ROUTE_OPS["rotate_add"] == 5
    header = open(os.path.join(ROOT, "include", "abc_hip.h")).read()
    assert "#define ABC_HIP_ROUTE_ROTATE_ADD 5" in header


@pytest.mark.gpu
def test_rotate_add_trees_behind_the_plugin_surface(built):
    _run(built, "test_hip_rotate_add_runtime", timeout=300)
