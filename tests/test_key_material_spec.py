"""The big-integer model of keys and fresh ciphertexts (tests/key_material_spec.py) on the CPU: divide_round against the oracle's
rescale on every word, fresh_ciphertext against the oracle's decryption, key_equation against a key built from its definition --
and the model's sensitivity to the errors tests/test_gpu_key_material.py has to catch with it (a wrong u, a wrong stream, the wrong
public-key component).  What the model cannot see -- the errors e0, e1 of an encryption -- is stated in its docstring.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyed_spec as ks  # noqa: E402
import key_material_spec as km  # noqa: E402

KEY = bytes(range(32))
KEY_SEC, KEY_PUB = bytes(range(64, 96)), bytes(range(160, 192))
WRAP_NONCE = 0xFFFFFFFFFFFFFFFE
SEED = 0x5EED
SCALE = 2.0 ** 40
RESCALE_CHAINS = {"n1024_36_50_60_45": (1024, [36, 50, 60, 45]), "n2048_50_40_50": (2048, [50, 40, 50])}


def _ckks(oracle_mod, n, bits):
    return oracle_mod.Oracle(oracle_mod.CKKS, n, oracle_mod.create_primes(n, bits))


def _edge(rng, primes, nl, n):
    """[nl][N], every limb from the ends and the middle of its range (tests/test_gpu_divide_round.py)"""
    return np.stack([rng.choice(np.array([0, 1, q - 1, q - 2, q // 2, q // 2 + 1], dtype=np.uint64), size=n) for q in primes[:nl]])


def _boundary_limb(rng, o, p, index, n):
    """the limb a rescale drops, built in COEFFICIENT form around the rounding boundary, in NTT form"""
    vals = np.array([0, 1, (p - 3) // 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1], dtype=np.uint64)
    coef = rng.choice(vals, size=n)
    coef[:len(vals)] = vals  # each of them at least once
    return o.ntt(index, coef)


@pytest.mark.parametrize("chain", list(RESCALE_CHAINS))
def test_divide_round_is_the_oracles_rescale(chain, oracle_mod):
    n, bits = RESCALE_CHAINS[chain]
    o = _ckks(oracle_mod, n, bits)
    primes = o.primes
    rng = np.random.default_rng(n)
    for nl in range(o.L, 1, -1):
        rand = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in primes[:nl]])
        bound, rand_bound = _edge(rng, primes, nl, n), rand.copy()
        bound[nl - 1] = _boundary_limb(rng, o, primes[nl - 1], nl - 1, n)
        rand_bound[nl - 1] = _boundary_limb(rng, o, primes[nl - 1], nl - 1, n)
        ct = np.stack([_edge(rng, primes, nl, n), bound, rand, rand_bound])  # rescale takes any number of polynomials
        want = o.rescale(ct)
        assert want.shape == (4, nl - 1, n)
        for s in range(4):
            coef = np.stack([o.intt(j, ct[s][j]) for j in range(nl)])
            got = km.divide_round(coef, primes[:nl], nl - 1)
            km.same("%s nl=%d poly %d" % (chain, nl, s), np.stack([o.ntt(j, got[j]) for j in range(nl - 1)]), want[s])


def test_divide_round_by_hand():
    """q = {5, 7}, p = 3: X = 0 .. 104, floor((X + 1) / 3) modulo 5 and 7"""
    xs = np.arange(105)
    coeffs = np.stack([xs % 5, xs % 7, xs % 3]).astype(np.uint64)
    got = km.divide_round(coeffs, [5, 7, 3], 2)
    assert got.tolist() == [(((xs + 1) // 3) % 5).tolist(), (((xs + 1) // 3) % 7).tolist()]
    got = km.divide_round(coeffs[[2, 0, 1]], [3, 5, 7], 0)  # the dropped prime need not be the last
    assert got.tolist() == [(((xs + 1) // 3) % 5).tolist(), (((xs + 1) // 3) % 7).tolist()]


def _plain(o, seed):
    rng = np.random.default_rng(seed)
    if o.scheme == 2:
        vals = rng.uniform(-1, 1, o.n // 2)
        return vals, o.ckks_encode(vals, SCALE)
    vals = rng.integers(0, o.t, o.n)
    return vals, o.encode(vals)


@pytest.fixture(scope="module")
def keyed_oracles(oracle_mod):
    """name -> oracle with keygen(SEED), no Galois keys"""
    made = {}

    def get(name):
        if name not in made:
            o = {"bfv4096": lambda: oracle_mod.Oracle.bfv_default(4096), "ckks4096": lambda: _ckks(oracle_mod, 4096, [50, 40, 50]),
                 "ckks1024": lambda: _ckks(oracle_mod, 1024, [36, 50, 60])}[name]()
            o.keygen(SEED, elts=[])
            made[name] = o
        return made[name]

    return get


@pytest.mark.parametrize("name", ["bfv4096", "ckks4096"])
def test_fresh_ciphertext_decrypts_under_the_oracle(name, keyed_oracles):
    o = keyed_oracles(name)
    small = ks.encrypt_small(KEY, WRAP_NONCE, o.n, 3)
    for i in range(3):
        vals, plain = _plain(o, 7 + i)
        ct = km.fresh_ciphertext(o, o.public_key(), small[i], plain)
        assert ct.shape == (2, o.L, o.n) and ct.dtype == np.uint64
        for j, q in enumerate(o.primes[:o.L]):
            assert int(ct[:, j].max()) < q
        if o.scheme == 2:
            # |error of a coefficient| <= |e0| + |e1 s| + |u e| + rounding < 21 (2N + 1) + N + 2 < 2^18.5 at N = 2^12; a slot sums N
            # coefficients times roots of unity: below 2^30.5 / scale = 2^-9.5 (tests/test_gpu_keyed_sampling.py, test_encrypt_keyed)
            assert np.abs(o.ckks_decode(o.decrypt(ct), SCALE).real - vals).max() < 2.0 ** -9
        else:
            km.same(name + " oracle decrypt %d" % i, o.decrypt(ct), plain)


def _seeded_small(seed, n):
    """u | e0 | e1 of the seeded sampling spec: splitmix64-seeded xoshiro256**, one word per draw"""
    m = (1 << 64) - 1
    s, x = [], seed & m
    for _ in range(4):
        x = (x + 0x9E3779B97F4A7C15) & m
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        s.append(z ^ (z >> 31))

    def rotl(v, k):
        return ((v << k) | (v >> (64 - k))) & m

    w = np.empty(3 * n, dtype=np.uint64)
    for i in range(3 * n):
        w[i] = (rotl((s[1] * 5) & m, 7) * 9) & m
        t = (s[1] << 17) & m
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]
        s[2] ^= t
        s[3] = rotl(s[3], 45)
    assert int(w[:n].max()) != m  # the one word a ternary draw rejects
    return np.stack([ks.ternary(w[:n]), ks.cbd(w[n:2 * n]), ks.cbd(w[2 * n:])])


@pytest.mark.parametrize("name", ["bfv4096", "ckks1024", "ckks4096"])
def test_fresh_ciphertext_is_the_oracles_encryption(name, keyed_oracles):
    """under the draws of the seeded spec the model is o.encrypt word for word: the same formula reached two ways"""
    o = keyed_oracles(name)
    for seed in (77, 0xFFFFFFFFFFFFFFFF):
        _, plain = _plain(o, seed % 1000)
        km.same("%s seed %d" % (name, seed), km.fresh_ciphertext(o, o.public_key(), _seeded_small(seed, o.n), plain), o.encrypt(plain, seed))


@pytest.mark.parametrize("name", ["bfv4096", "ckks1024"])
def test_model_sees_a_wrong_u_and_a_wrong_key_component(name, keyed_oracles):
    """each of the errors a decryption cannot see changes at least 99 % of the model's words"""
    o = keyed_oracles(name)
    pk = o.public_key()
    _, plain = _plain(o, 3)
    small = ks.encrypt_small(KEY, WRAP_NONCE, o.n, 2)
    base = km.fresh_ciphertext(o, pk, small[0], plain)

    def changed(ct):
        return float(np.mean(ct != base))

    next_stream = small[0].copy()
    next_stream[0] = small[1][0]  # u of stream nonce + 1 for ciphertext 0
    assert changed(km.fresh_ciphertext(o, pk, next_stream, plain)) >= 0.99
    from_e0 = small[0].copy()
    from_e0[0] = small[0][1]  # u read from the slot of e0
    assert changed(km.fresh_ciphertext(o, pk, from_e0, plain)) >= 0.99
    assert changed(km.fresh_ciphertext(o, np.ascontiguousarray(pk[::-1]), small[0], plain)) >= 0.99
    km.same(name + " the model repeats itself", km.fresh_ciphertext(o, pk.copy(), small[0].copy(), plain), base)


def test_key_equation_holds_a_key_built_from_its_definition(oracle_mod):
    """key[i][0][j] = -(a_i[j] s + e_i) + [j == i] (q_sp mod q_i) new_key, key[i][1][j] = a_i[j], assembled here with Python integers:
    key_equation accepts it, and refuses one flipped word of either component, a wrong error and a factor on the wrong limb"""
    o = _ckks(oracle_mod, 1024, [36, 50, 60])
    n, K, L, primes = o.n, o.K, o.L, o.primes
    s = ks.secret(KEY_SEC, n)
    sk = np.stack([o.ntt(j, km.small_residues(s, q)) for j, q in enumerate(primes)])
    new_key = np.stack([(sk[j].astype(object) ** 2 % q).astype(np.uint64) for j, q in enumerate(primes)])
    a = ks.key_uniform(KEY_PUB, 2, n, primes, L)
    e = ks.key_errors(KEY_SEC, 2, n, L)

    def build(nkeys, switched_from):
        key = np.empty((nkeys, 2, K, n), dtype=np.uint64)
        for i in range(nkeys):
            for j, q in enumerate(primes):
                v = -(a[i][j].astype(object) * sk[j].astype(object) + o.ntt(j, km.small_residues(e[i], q)).astype(object))
                if switched_from is not None and j == i:
                    v = v + (primes[K - 1] % q) * switched_from[i].astype(object)
                key[i][0][j], key[i][1][j] = (v % q).astype(np.uint64), a[i][j]
        return key

    key = build(L, new_key)
    km.key_equation(o, key, a, e, sk, new_key)
    km.key_equation(o, build(1, None), a[:1], e[:1], sk, None)  # the public key's form: an encryption of zero
    for comp, i, j, x in ((0, 0, 0, 0), (0, L - 1, K - 1, n - 1), (1, 1, 1, 17)):
        bad = key.copy()
        bad[i][comp][j][x] ^= np.uint64(1)
        with pytest.raises(AssertionError):
            km.key_equation(o, bad, a, e, sk, new_key)
    wrong_e = e.copy()
    wrong_e[1][5] += 1
    with pytest.raises(AssertionError):
        km.key_equation(o, key, a, wrong_e, sk, new_key)
    with pytest.raises(AssertionError):
        km.key_equation(o, key, a, e, sk, np.ascontiguousarray(new_key[::-1]))
    with pytest.raises(AssertionError):
        km.key_equation(o, key, a, e, sk, None)
