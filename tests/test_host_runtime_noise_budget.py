"""HipCiphertext::noiseBits / noiseBitsBatch behind the plugin surface (tests/cpp/test_hip_noise_budget.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = os.path.join(ROOT, "abc_amd", "runtime")
DRIVER = os.path.join(RT, "test_hip_noise_budget")


@pytest.fixture(scope="module")
def built():
    from abc_amd import capi
    assert os.path.exists(capi.LIB_PATH), "libabc_hip.so missing: python -m abc_amd.build"
    subprocess.check_call(["make", "-C", RT, "test_hip_noise_budget"], stdout=subprocess.DEVNULL)
    return DRIVER


def test_noise_budget_driver_builds(built):
    assert os.access(built, os.X_OK)


@pytest.mark.gpu
def test_noise_budget_behind_the_plugin_surface(built):
    p = subprocess.run([built], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " 0 failed" in p.stdout
