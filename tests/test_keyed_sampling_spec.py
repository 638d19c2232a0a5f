"""The keyed sampling spec on the CPU: the Python restatement (tests/keyed_spec.py) against RFC 8439's
test vector, and the library's host twin (abc_hip_keyed_small_host, abc_amd/csrc/abc_sample.hpp) against the restatement.
No GPU: the device side of the same checks is tests/test_gpu_keyed_sampling.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyed_spec as ks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32))
ALL_ONES = (1 << 64) - 1
# RFC 8439 section 2.3.2: nonce 00:00:00:09 00:00:00:4a 00:00:00:00, block count 1, in the spec's state layout
RFC_COUNTER, RFC_STREAM = 0x0900000000000001, 0x4A000000
WRAP_NONCE = 0xFFFFFFFFFFFFFFFE


def test_block_function_matches_rfc8439():
    b = ks.blocks(KEY, RFC_STREAM, RFC_COUNTER, 1)[0]
    assert b.astype("<u4").tobytes()[:8] == bytes.fromhex("10f1e7e4d13b5915")
    assert b[0] == 0xE4E7F110 and b[15] == 0x4E3C50A2  # first and last word of the RFC's serialised state
    w = ks.words(KEY, RFC_STREAM, 8 * RFC_COUNTER, 8)
    assert int(w[0]) == 0x15593BD1E4E7F110
    assert ks.ternary(w).tolist() == [1, 1, 0, 0, -1, -1, -1, 1]
    assert ks.cbd(w).tolist() == [-4, -1, -1, -5, -3, -2, -2, 2]


def test_words_are_addressed_by_number():
    """word W of a stream is word W mod 8 of block W div 8, whatever the window it is read through"""
    whole = ks.words(KEY, 5, 0, 64)
    assert np.array_equal(ks.words(KEY, 5, 13, 30), whole[13:43])
    assert not np.array_equal(ks.words(KEY, 6, 0, 64), whole)


@pytest.mark.parametrize("n,count,nonce", [(1024, 3, 7), (4096, 4, WRAP_NONCE)])
def test_host_twin_matches_restatement(capi, n, count, nonce):
    got = capi.keyed_small_host(KEY, nonce, n, count)
    want = ks.encrypt_small(KEY, nonce, n, count)
    assert got.shape == want.shape == (count, 3, n)
    assert np.array_equal(got, want)
    assert set(np.unique(got[:, 0])) == {-1, 0, 1}
    assert np.abs(got[:, 1:].astype(int)).max() <= 21
    # ciphertext i of a batch is ciphertext 0 of the call with nonce + i: the stream id wraps modulo 2^64
    assert np.array_equal(capi.keyed_small_host(KEY, (nonce + count - 1) % 2 ** 64, n, 1)[0], got[count - 1])


def test_host_twin_rejects_bad_sizes(capi):
    with pytest.raises(capi.AbcHipError):
        capi.keyed_small_host(KEY, 0, 12, 1)
    with pytest.raises(ValueError):
        capi.keyed_small_host(KEY[:31], 0, 1024, 1)
    assert capi.keyed_small_host(KEY, 0, 1024, 0).shape == (0, 3, 1024)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/cpp/test_keyed_sampling.cpp: the host twin as a stand-alone program, under AddressSanitizer and UBSan where the
    toolchain has their runtimes"""
    out = str(tmp_path_factory.mktemp("keyed") / "test_keyed_sampling")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "abc_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "test_keyed_sampling.cpp"), "-o", out]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return out


def test_standalone_host_twin(driver):
    n, count = 1024, 2
    p = subprocess.run([driver, "small", KEY.hex(), str(WRAP_NONCE + 1), str(n), str(count)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.array([int(v) for v in p.stdout.split()], dtype=np.int8).reshape(count, 3, n)
    assert np.array_equal(got, ks.encrypt_small(KEY, WRAP_NONCE + 1, n, count))


def test_edge_words(driver, capi):
    """ternary and uniform_q at the words where a shortcut would show: against Python's integers, for three prime widths"""
    primes = capi.create_primes(4096, [36, 50, 60])
    assert [q.bit_length() for q in primes] == [36, 50, 60]
    cases = []
    for q in primes:
        for lo in (ALL_ONES, 0, q - 1, q, 1):
            for hi in (ALL_ONES, 0, q - 1, 1):
                cases.append((lo, hi, q))
    args = [str(v) for c in cases for v in c]
    p = subprocess.run([driver, "edge"] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [line.split() for line in p.stdout.splitlines()]
    assert len(rows) == len(cases)
    for (lo, hi, q), (t_lo, t_hi, u) in zip(cases, rows):
        want = ((hi << 64) + lo) % q
        assert int(u) == want == ks.uniform_q(lo, hi, q), (lo, hi, q)
        assert int(t_lo) == lo % 3 - 1 == int(ks.ternary([lo])[0]), lo
        assert int(t_hi) == hi % 3 - 1 == int(ks.ternary([hi])[0]), hi
    assert int(ks.ternary([ALL_ONES])[0]) == -1  # no rejection: the all-ones word is a draw like any other
