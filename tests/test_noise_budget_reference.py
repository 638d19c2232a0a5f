"""The yardstick of the noise-budget tests, pinned on the CPU before the device is compared with it.

exact_noise_budget() is the definition in Python big integers (SEAL's Decryptor::invariant_noise_budget, which the reference
reaches through SealCiphertext::noiseBits, src/runtime/SealCiphertext.cpp:80-83):
  v = t (c0 + c1 s + c2 s^2) mod Q coefficient-wise, Q the product of the data primes, lifted into (-Q/2, Q/2] (Q odd: no tie);
  m = the largest magnitude; budget = max(0, bitlen(Q) - bitlen(m) - 1), bitlen(0) = 0.
The phase is formed per limb with the oracle's transforms and secret key and Python ints; composition, the product with t, the
centring and the bit length are Python ints throughout.  Oracle.noise_budget (oracle/orc_keys.c, orc_bfv_noise_budget)
accumulates the mixed-radix digits in long double; should the two ever disagree, the big-integer value is the definition.

A disagreement on record (none among the cases below): where Q is more than 64 bits wider than the noise, the oracle's Q - value
cancels to nothing, so coefficients with negative noise drop out of its maximum.  On BFVDefault(32768), keygen seed 0xABC00001,
slot values default_rng(32768).integers(0, 1025), encryption seed 1, the largest coefficient (28 bits) is negative and the largest
positive one has 27 bits: the definition gives 796, the oracle 797.  tests/test_gpu_noise_budget.py uses another encryption seed
for that case.
"""
import numpy as np
import pytest

SEED = 0xABC00001


def phase_limbs(o, ct):
    """c0 + c1 s (+ c2 s^2) per data limb, coefficient form: a list of L lists of N Python ints"""
    ct = np.asarray(ct)
    sk = o.secret_key()  # [K][N], NTT form
    out = []
    for j in range(o.L):
        q = o.primes[j]
        s = [int(x) for x in sk[j]]
        acc = [0] * o.n
        sp = s
        for p in range(1, ct.shape[0]):
            cp = o.ntt(j, ct[p, j])
            acc = [(a + int(c) * w) % q for a, c, w in zip(acc, cp, sp)]
            if p + 1 < ct.shape[0]:
                sp = [(a * b) % q for a, b in zip(sp, s)]
        back = o.intt(j, np.array(acc, dtype=np.uint64))
        out.append([(int(a) + int(b)) % q for a, b in zip(back, ct[0, j])])
    return out


def exact_noise_budget(o, ct):
    qs = o.primes[:o.L]
    Q = 1
    for q in qs:
        Q *= q
    limbs = phase_limbs(o, ct)
    weights = [(Q // q) * pow(Q // q, -1, q) for q in qs]  # CRT: x = sum r_j (Q/q_j) ((Q/q_j)^-1 mod q_j) mod Q
    m = 0
    for k in range(o.n):
        v = sum(limbs[j][k] * weights[j] for j in range(o.L)) % Q
        v = v * o.t % Q
        if v > Q // 2:
            v = Q - v
        m = max(m, v)
    return max(0, Q.bit_length() - m.bit_length() - 1)


def fresh(o, rng, seed):
    return o.encrypt(o.encode(rng.integers(0, 1025, size=o.n).astype(np.int64)), seed)


@pytest.mark.parametrize("n", [4096, 8192])
def test_big_integer_definition_agrees_with_the_oracle(n, oracle_mod):
    o = oracle_mod.Oracle.bfv_default(n)
    o.keygen(SEED)
    rng = np.random.default_rng(n)
    acc = fresh(o, rng, 100)
    b_fresh = exact_noise_budget(o, acc)
    print("N=%d fresh: exact %d oracle %d" % (n, b_fresh, o.noise_budget(acc)))
    assert b_fresh == o.noise_budget(acc)
    relin = []
    for depth in range(1, 13):
        m3 = o.multiply(acc, fresh(o, rng, 100 + depth))
        b3 = exact_noise_budget(o, m3)
        acc = o.relinearize(m3)
        b2 = exact_noise_budget(o, acc)
        print("N=%d depth %d: size 3 exact %d oracle %d, relinearised exact %d oracle %d"
              % (n, depth, b3, o.noise_budget(m3), b2, o.noise_budget(acc)))
        assert b3 == o.noise_budget(m3), "size-3 product, depth %d" % depth
        assert b2 == o.noise_budget(acc), "relinearised product, depth %d" % depth
        relin.append(b2)
        if b2 == 0:
            break
    assert relin[-1] == 0, "the chain did not reach budget 0"
    assert b_fresh > relin[0] > 0
    assert all(a > b for a, b in zip(relin, relin[1:]))
    if n == 4096:
        assert len(relin) == 2  # BFVDefault(4096): the depth-2 product has exactly 0 bits left


def test_all_zero_ciphertext_has_bitlen_q_minus_one(oracle_mod):
    o = oracle_mod.Oracle.bfv_default(4096)
    o.keygen(SEED)
    z = np.zeros((2, o.L, o.n), dtype=np.uint64)
    Q = 1
    for q in o.primes[:o.L]:
        Q *= q
    assert exact_noise_budget(o, z) == Q.bit_length() - 1 == o.noise_budget(z)
