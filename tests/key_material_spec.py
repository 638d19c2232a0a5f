"""Keys and fresh ciphertexts as plain big-integer formulas -- TEST INFRASTRUCTURE ONLY.  No GPU, and of the oracle only its
transforms (o.ntt / o.intt) and, for BFV, its add_plain (whose Delta-scaling is pinned by tests/test_gpu_parity.py and
tests/test_gpu_operand_forms.py).

  divide_round      floor((X + floor(p/2)) / p) on the CRT lift X of every coefficient: SEAL's divide_and_round_q_last as one integer
                    formula (last += p/2; x_j - (last mod q_j - p/2 mod q_j), times p^-1 mod q_j, is (X + p/2 - (X + p/2) mod p) / p)
  fresh_ciphertext  a public-key encryption from its draws u | e0 | e1: c_p = NTT(u) (.) pk[p] + e_p at key
                    level, divided by the special prime, plus the message
  key_equation      a published key-switching key against its definition (KeyGenerator::generate_one_kswitch_key)

What fresh_ciphertext cannot see: e0 and e1 of an encryption are bounded by 21 and are divided by a special prime of at least
2^36, so a wrong e changes an output word only where the sum lands within 42 of a rounding boundary -- with probability below
2^-30 per word.  The errors of an ENCRYPTION are therefore not testable through any entry point (their draws are:
tests/test_gpu_keyed_sampling.py compares them with tests/keyed_spec.py).  u multiplies the public key and changes every word.
The errors of a KEY are published undivided and key_equation holds them exactly."""
import numpy as np


def same(what, got, want):
    """got == want word for word, or an AssertionError that names the first difference"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s: got %s want %s"
                             % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def crt_lift(coeffs, primes):
    """[K][N] residues -> N Python integers in [0, q_0 ... q_{K-1}) (an object array)"""
    primes = [int(q) for q in primes]
    assert len(coeffs) == len(primes)
    big = 1
    for q in primes:
        big *= q
    x = np.zeros(np.shape(coeffs)[1], dtype=object)
    for j, q in enumerate(primes):
        rest = big // q
        x = x + np.asarray(coeffs[j]).astype(object) * (rest * pow(rest, -1, q))
    return x % big


def divide_round(coeffs, primes, drop):
    """coeffs [K][N], coefficient form, limb j modulo primes[j] -> [K-1][N]: floor((X + floor(p/2)) / p) modulo every prime but
    p = primes[drop], X the CRT lift of a coefficient"""
    p = int(primes[drop])
    y = (crt_lift(coeffs, primes) + p // 2) // p
    keep = [int(q) for j, q in enumerate(primes) if j != drop]
    return np.stack([(y % q).astype(np.uint64) for q in keep])


def small_residues(small, q):
    """a signed small polynomial modulo q"""
    return (np.asarray(small).astype(np.int64) % int(q)).astype(np.uint64)


def fresh_ciphertext(o, pk, small, plain):
    """pk [2][K][N] NTT form, small [3][N] int8 (u | e0 | e1), plain as o.encrypt takes it -> the ciphertext [2][L][N]"""
    primes, K, L, n = [int(q) for q in o.primes], o.K, o.L, o.n
    assert np.shape(pk) == (2, K, n) and np.shape(small) == (3, n)
    ckks = (o.scheme == 2)
    u_ntt = [o.ntt(j, small_residues(small[0], q)).astype(object) for j, q in enumerate(primes)]
    ct = np.empty((2, L, n), dtype=np.uint64)
    for p in range(2):
        coef = []
        for j, q in enumerate(primes):
            c = (u_ntt[j] * pk[p][j].astype(object) % q).astype(np.uint64)
            e = small_residues(small[1 + p], q)
            if ckks:  # the error joins in NTT form; the division needs coefficients
                c = ((c.astype(object) + o.ntt(j, e).astype(object)) % q).astype(np.uint64)
                coef.append(o.intt(j, c))
            else:
                coef.append(((o.intt(j, c).astype(object) + e.astype(object)) % q).astype(np.uint64))
        low = divide_round(np.stack(coef), primes, K - 1)
        for j in range(L):
            ct[p][j] = o.ntt(j, low[j]) if ckks else low[j]
    if not ckks:
        return o.add_plain(ct, np.ascontiguousarray(plain, dtype=np.uint64))
    plain = np.asarray(plain, dtype=np.uint64)
    assert plain.shape == (L, n)
    for j in range(L):
        ct[0][j] = ((ct[0][j].astype(object) + plain[j].astype(object)) % primes[j]).astype(np.uint64)
    return ct


def key_equation(o, key, a, e, sk, new_key, what="key"):
    """Every published word of a key is accounted for: key[i][1][j] == a_i[j], and key[i][0][j] + a_i[j] s - [j == i] (q_sp mod q_i)
    new_key == -e_i, exactly.  key [nkeys][2][K][N] and a [nkeys][K][N] in NTT form, e [nkeys][N] signed, sk [K][N] the secret key in
    NTT form, new_key [K][N] in NTT form what the key switches from (None: the public key, an encryption of zero)."""
    primes, K = [int(q) for q in o.primes], o.K
    sko = np.asarray(sk).astype(object)
    e = np.asarray(e).astype(np.int64)
    assert len(key) == len(a) == len(e)
    for i in range(len(key)):
        for j, q in enumerate(primes):
            same("%s a[%d][%d]" % (what, i, j), key[i][1][j], a[i][j])
            v = key[i][0][j].astype(object) + a[i][j].astype(object) * sko[j]
            if new_key is not None and j == i:
                v = v - (primes[K - 1] % primes[i]) * new_key[i].astype(object)
            coeffs = o.intt(j, (v % q).astype(np.uint64))
            same("%s -e[%d] limb %d" % (what, i, j), coeffs, ((-e[i]) % q).astype(np.uint64))
