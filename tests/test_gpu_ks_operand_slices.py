"""The per-chunk slice of a key switch's operands (KsOperands::slice, abc_context.hpp) in the call shape where the operand's stride
is not the width of a ciphertext: abc_hip_relinearize of size-3 ciphertexts -- target c2 and addend (c0, c1) both 3 * nl * N words
apart, the output 2 * nl * N, add_c1 set -- in ragged chunks: three ciphertexts with ABC_HIP_CHUNK=2, a chunk of two and one of
one.  Word for word against the CPU oracle, every row, once with ABC_HIP_LANES=2 and once with 1 (up to eight ciphertexts a call
stays on one lane either way; the two settings differ in the scratch plan_chunks lays out).

One case per sequence that goes through for_each_chunk, at the smallest shape that selects it; the route string is asserted so that
a case which falls to another sequence fails.  bsplit_big and generic chunk by a GiB budget no small shape splits: their chunks go
through the same slice().  Inputs are residues, not encryptions (fuzz_parity.random_ct: uniform words plus the edge values).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_parity import random_ct  # noqa: E402

pytestmark = pytest.mark.gpu

COUNT, NL = 3, 2
CASES = {
    # name: (scheme, N, widths of the two data primes + the special prime, route of abc_hip_relinearize)
    "lds_fp": ("ckks", 1 << 12, [40, 40, 40], "lds_fp"),
    "lds_int": ("ckks", 1 << 12, [58, 40, 40], "lds_int guard=1 lazy=0"),
    "split14": ("ckks", 1 << 14, [50, 40, 50], "split14 front=lean pack=1 main=split4"),
    "isplit14": ("ckks", 1 << 14, [55, 40, 50], "isplit14 guard=0 fpmask=0x2"),
    "bsplit14": ("bfv", 1 << 14, [48, 48, 49], "bsplit14 pass0=per_target"),
    "gsplit15": ("ckks", 1 << 15, [50, 40, 50], "gsplit15"),
    "isplit15": ("ckks", 1 << 15, [55, 40, 50], "isplit15 guard=0 fpmask=0x2"),
}


@pytest.fixture(scope="module")
def references(oracle_mod):
    """per case, computed once and shared by both lane settings: (primes, t, relinearisation key, size-3 inputs, expected outputs)"""
    cache = {}

    def get(name):
        if name not in cache:
            scheme, n, bits, _ = CASES[name]
            primes = oracle_mod.create_primes(n, bits)
            bfv = scheme == "bfv"
            t = oracle_mod.plain_modulus_batching(n, 20) if bfv else 0
            o = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t) if bfv else oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
            o.keygen(0xABC00700 + len(cache), elts=[])  # the relinearisation key is all this needs
            rng = np.random.default_rng(n + len(name))
            t3 = random_ct(rng, primes, NL, n, COUNT, size=3)
            want = np.stack([o.relinearize(x) for x in t3])
            for a in (t3, want):
                a.setflags(write=False)
            cache[name] = (primes, t, o.relin_key(), t3, want)
        return cache[name]

    return get


@pytest.mark.parametrize("lanes", [2, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_relinearize_size3_ragged_chunks(name, lanes, references, capi, monkeypatch):
    scheme, n, _, route = CASES[name]
    primes, t, relin, t3, want = references(name)
    monkeypatch.setenv("ABC_HIP_CHUNK", "2")  # read when the context is created
    monkeypatch.setenv("ABC_HIP_LANES", str(lanes))
    g = capi.Context(capi.BFV, n, primes, t) if scheme == "bfv" else capi.Context(capi.CKKS, n, primes)
    try:
        g.load_keys(relin=relin)
        assert g.route("relinearize", NL, COUNT) == route
        got = g.relinearize(t3)
        assert got.shape == want.shape
        for row in range(COUNT):
            bad = np.argwhere(got[row] != want[row])
            assert not len(bad), "%s lanes=%d row %d: %d/%d words differ, first at %s" % (
                name, lanes, row, len(bad), want[row].size, tuple(bad[0]))
    finally:
        g.close()
