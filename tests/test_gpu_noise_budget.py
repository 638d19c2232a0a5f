"""abc_hip_noise_budget (Decryptor::invariant_noise_budget, src/runtime/SealCiphertext.cpp:80-83) through the C ABI against the
CPU oracle, and against the big-integer definition (tests/test_noise_budget_reference.py) wherever that is cheap (always where
N <= 8192).  The budget is an exact
integer: every comparison is equality, for every ciphertext of a batch.  Both sides hold the same keys through the shared seeded
sampling spec.

Oracle.noise_budget accumulates the lifted value in long double (oracle/orc_keys.c): where Q is more than 64 bits wider than the
noise, Q - value cancels to nothing and the coefficients with NEGATIVE noise drop out of its maximum.  That usually leaves the bit
length unchanged, but not always: on BFVDefault(32768), keygen seed 0xABC00001, slot values default_rng(32768), the fresh
ciphertext under encryption seed 1 has its largest coefficient (28 bits) on the negative side and a 27-bit one on the positive
side; the big-integer definition and the device give 796, the oracle 797.  The big-integer value is the definition, so that case
encrypts under seed 3 instead (FRESH_SEEDS); every case of this file was checked on the CPU to have oracle == definition, and the
ring test compares with the definition on every ring, not only where N <= 8192.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_noise_budget_reference import exact_noise_budget  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xABC00001
RINGS = ["bfv4096", "bfv8192", "bfv16384", "bfv32768", "config5"]
FRESH_SEEDS = {"bfv32768": (3, 2)}  # encryption seeds of the ring test's two fresh ciphertexts; (1, 2) elsewhere (see above)


def _params(om, name):
    if name == "config5":  # BASELINE config 5: N = 2^16, explicit primes (SEAL's default table stops at 2^15)
        n = 65536
        return n, om.create_primes(n, [55] * 8 + [56]), om.plain_modulus_batching(n, 20)
    if name == "wide16384":  # primes above 2^50: outside the fp64 fast path
        n = 16384
        return n, om.create_primes(n, [60, 40, 40, 40, 60]), om.plain_modulus_batching(n, 20)
    n = int(name[3:])
    return n, om.default_bfv_primes(n), om.plain_modulus_batching(n, 20)


@pytest.fixture(scope="module")
def pair(oracle_mod, capi):
    """name -> (oracle context, device context) with identical keys; built on first use, kept for the module"""
    made = {}

    def get(name):
        if name not in made:
            n, primes, t = _params(oracle_mod, name)
            o = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)
            o.keygen(SEED)
            g = capi.Context(capi.BFV, n, primes, t)
            g.keygen(SEED)
            made[name] = (o, g)
        return made[name]

    yield get
    for _, g in made.values():
        g.close()


def _fresh(o, rng, seed):
    return o.encrypt(o.encode(rng.integers(0, 1025, size=o.n).astype(np.int64)), seed)


def _qbits(o):
    Q = 1
    for q in o.primes[:o.L]:
        Q *= q
    return Q.bit_length()


def _check(name, o, g, cts, exact=False):
    """one batched device call over cts (same size) against the oracle, entry by entry; returns the budgets"""
    got = g.noise_budget(np.stack(cts))
    want = [o.noise_budget(c) for c in cts]
    print("%s: device %s oracle %s" % (name, list(map(int, got)), want))
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (len(cts),)
    assert [int(x) for x in got] == want, name
    if exact:
        ex = [exact_noise_budget(o, c) for c in cts]
        print("%s: big-integer definition %s" % (name, ex))
        assert [int(x) for x in got] == ex, name + " (big-integer definition)"
    return want


@pytest.mark.parametrize("ring", RINGS)
def test_fresh_product_and_relinearised_product(ring, pair):
    o, g = pair(ring)
    rng = np.random.default_rng(o.n)
    exact = True  # cheap enough on every ring, and the oracle's long double needs the cross-check there most
    sa, sb = FRESH_SEEDS.get(ring, (1, 2))
    a, b = _fresh(o, rng, sa), _fresh(o, rng, sb)
    fresh = _check(ring + " fresh", o, g, [a, b], exact)
    m3 = g.multiply(a, b)
    assert m3.shape == (3, o.L, o.n)
    prod = _check(ring + " size-3 product", o, g, [m3], exact)
    r = g.relinearize(m3)
    rel = _check(ring + " relinearised product", o, g, [r], exact)
    assert min(fresh) > prod[0] > 0 and min(fresh) > rel[0] > 0
    one = g.noise_budget(r)  # a single ciphertext comes back as an int
    assert isinstance(one, int) and one == rel[0]
    # an all-zero ciphertext: no noise at all, bitlen(0) = 0; next to a fresh one in the same call
    z = np.zeros_like(a)
    got = g.noise_budget(np.stack([z, a, z]))
    print("%s zero/fresh/zero: %s, bitlen(Q) = %d" % (ring, list(map(int, got)), _qbits(o)))
    assert [int(x) for x in got] == [_qbits(o) - 1, fresh[0], _qbits(o) - 1]
    assert o.noise_budget(z) == _qbits(o) - 1


@pytest.mark.parametrize("ring", ["bfv4096", "bfv8192"])
def test_multiply_chain_down_to_zero(ring, pair):
    o, g = pair(ring)
    rng = np.random.default_rng(7 * o.n)
    acc = _fresh(o, rng, 10)
    seen = _check(ring + " chain depth 0", o, g, [acc], True)
    for depth in range(1, 13):
        acc = g.mul_relin(acc, _fresh(o, rng, 10 + depth))
        seen += _check("%s chain depth %d" % (ring, depth), o, g, [acc], True)
        if seen[-1] == 0:
            break
    assert seen[-1] == 0 and all(a > b for a, b in zip(seen, seen[1:]))
    # one level past the end: the clamp, not a negative number
    acc = g.mul_relin(acc, _fresh(o, rng, 99))
    assert _check(ring + " past the end", o, g, [acc], True) == [0]
    assert g.noise_budget(acc) == 0


def test_batch_of_ciphertexts_at_different_depths(pair):
    o, g = pair("bfv8192")
    rng = np.random.default_rng(11)
    levels = [_fresh(o, rng, 20)]
    for depth in range(1, 6):
        levels.append(g.mul_relin(levels[-1], _fresh(o, rng, 20 + depth)))
    order = [3, 0, 5, 1, 4, 2, 0]
    want = _check("mixed depths %s" % order, o, g, [levels[d] for d in order], True)
    assert len(set(want)) == 6  # six different values in one call, in an order that is not monotone
    assert any(a < b for a, b in zip(want, want[1:])) and any(a > b for a, b in zip(want, want[1:]))


@pytest.mark.parametrize("ring", ["bfv8192", "bfv32768"])
def test_one_noisy_coefficient_in_the_last_block(ring, pair):
    """the same ciphertext with one coefficient of c0 pushed far off: whichever block, wave and lane that coefficient falls into,
    it alone decides the budget"""
    o, g = pair(ring)
    rng = np.random.default_rng(13)
    base = g.mul_relin(_fresh(o, rng, 30), _fresh(o, rng, 31))
    b0 = _check(ring + " base", o, g, [base])[0]
    Q = 1
    for q in o.primes[:o.L]:
        Q *= q
    D = Q // 1000003  # t D mod Q is large whatever t is: far above the noise of the base
    n = o.n
    variants = []
    where = [n - 1, n - 63, n - 64, n - 65, n - 256, n - 257, 255, 0]
    for idx in where:
        v = base.copy()
        for j, q in enumerate(o.primes[:o.L]):
            v[0, j, idx] = np.uint64((int(v[0, j, idx]) + D) % q)
        variants.append(v)
    got = _check("%s one coefficient at %s" % (ring, where), o, g, variants, o.n <= 8192)
    assert all(b < b0 for b in got)
    assert _check(ring + " base again", o, g, [base, variants[0], base]) == [b0, got[0], b0]


def test_wide_chain_outside_the_fp64_path(pair):
    o, g = pair("wide16384")
    rng = np.random.default_rng(17)
    a = _fresh(o, rng, 40)
    d1 = g.mul_relin(a, _fresh(o, rng, 41))
    d2 = g.mul_relin(d1, _fresh(o, rng, 42))
    want = _check("wide chain depths 0, 1, 2", o, g, [a, d1, d2])
    assert want[0] > want[1] > want[2]
    _check("wide chain size-3 product", o, g, [g.multiply(d1, a)])


def test_loaded_secret_key_gives_the_same_value(pair, capi):
    o, g = pair("bfv4096")
    rng = np.random.default_rng(19)
    cts = [_fresh(o, rng, 50), g.mul_relin(_fresh(o, rng, 51), _fresh(o, rng, 52))]
    want = _check("generated keys", o, g, cts, True)
    g2 = capi.Context(capi.BFV, o.n, o.primes, o.t)
    g2.load_keys(sk=o.secret_key())  # abc_hip_load_secret_key: nothing else is needed
    assert _check("loaded secret key", o, g2, cts) == want
    g2.close()


def test_error_paths_leave_the_context_usable(pair, capi, oracle_mod):
    o, g = pair("bfv4096")
    rng = np.random.default_rng(23)
    a = _fresh(o, rng, 60)
    want = o.noise_budget(a)
    for bad, what in ((np.zeros((1, 1, o.L, o.n), dtype=np.uint64), "size 1"),
                      (np.zeros((1, 4, o.L, o.n), dtype=np.uint64), "size 4"),
                      (np.zeros((1, 2, o.L - 1, o.n), dtype=np.uint64), "nl = L - 1")):
        with pytest.raises(capi.AbcHipError):
            g.noise_budget(bad)
        assert g.noise_budget(a) == want, "after " + what
    # count = 0 succeeds and touches nothing
    g.op("noise_budget", None, 2, o.L, None, C.c_size_t(0))
    # no secret key
    g2 = capi.Context(capi.BFV, o.n, o.primes, o.t)
    with pytest.raises(capi.AbcHipError) as e:
        g2.noise_budget(a)
    assert "secret key" in str(e.value)
    g2.keygen(SEED)
    assert g2.noise_budget(a) == want
    g2.close()
    # CKKS: SEAL refuses too
    n = 16384
    primes = oracle_mod.create_primes(n, [50, 40, 40, 40, 50])
    oc = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    oc.keygen(SEED)
    gc = capi.Context(capi.CKKS, n, primes)
    gc.keygen(SEED)
    x = np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in primes[:4]], axis=1)
    with pytest.raises(capi.AbcHipError) as e:
        gc.noise_budget(x)
    assert "CKKS" in str(e.value)
    assert np.array_equal(gc.decrypt(x), oc.decrypt(x))
    gc.close()


def test_decrypt_is_unchanged_around_a_budget_call(pair):
    """decrypt and the budget share the phase helper and the workspace"""
    o, g = pair("bfv16384")
    rng = np.random.default_rng(29)
    a, b, c = _fresh(o, rng, 70), _fresh(o, rng, 71), _fresh(o, rng, 72)
    r = g.mul_relin(a, b)
    m3 = g.multiply(r, c)
    two, three = np.stack([a, r, b]), np.stack([m3, g.multiply(a, b)])
    want2 = np.stack([o.decrypt(x) for x in two])
    want3 = np.stack([o.decrypt(x) for x in three])
    assert np.array_equal(g.decrypt(two), want2) and np.array_equal(g.decrypt(three), want3)
    _check("size 2 batch", o, g, list(two))
    assert np.array_equal(g.decrypt(three), want3)
    _check("size 3 batch", o, g, list(three))
    assert np.array_equal(g.decrypt(two), want2)
    _check("size 2 batch, again", o, g, list(two) + [c] * 5)  # a larger batch: the workspace grows
    assert np.array_equal(g.decrypt(two), want2) and np.array_equal(g.decrypt(three), want3)
