"""Self-consistency of the oracle's building blocks (so a golden-vector pass is not an accident)."""
import numpy as np
import pytest


def test_ntt_is_negacyclic_convolution(oracle_mod):
    n = 1024
    primes = oracle_mod.create_primes(n, [40, 41])
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    q = primes[0]
    rng = np.random.default_rng(0)
    a = rng.integers(0, q, n, dtype=np.uint64)
    b = rng.integers(0, q, n, dtype=np.uint64)
    fa, fb = o.ntt(0, a), o.ntt(0, b)
    prod = np.array([(int(x) * int(y)) % q for x, y in zip(fa, fb)], dtype=np.uint64)
    c = o.intt(0, prod)
    # schoolbook negacyclic product
    ref = [0] * n
    ai, bi = [int(v) for v in a], [int(v) for v in b]
    for i in range(n):
        if ai[i] == 0:
            continue
        for j in range(n):
            k = i + j
            v = ai[i] * bi[j]
            if k >= n:
                ref[k - n] -= v
            else:
                ref[k] += v
    assert [int(v) for v in c] == [v % q for v in ref]
    assert np.array_equal(o.intt(0, fa), a)


def test_ntt_root_is_minimal_primitive(oracle_mod):
    n = 4096
    o = oracle_mod.Oracle.bfv_default(n)
    for i, q in enumerate(o.primes):
        psi = int(oracle_mod.lib().orc_ctx_ntt_root(o.h, i))
        assert pow(psi, n, q) == q - 1
        # minimal among all primitive 2N-th roots (odd powers of psi)
        sq, cur, best = psi * psi % q, psi, psi
        for _ in range(n):
            best = min(best, cur)
            cur = cur * sq % q
        assert best == psi


def test_keyswitch_preserves_plaintext(oracle_mod):
    o = oracle_mod.Oracle.bfv_default(4096)
    o.keygen(5)
    vals = list(range(-20, 20))
    ct = o.encrypt(o.encode(oracle_mod.expand_vector(vals, o.n)), 9)
    sq = o.multiply(ct, ct)
    assert list(o.decode(o.decrypt(sq))[:40]) == [v * v for v in vals]          # size-3 decrypt
    assert list(o.decode(o.decrypt(o.relinearize(sq)))[:40]) == [v * v for v in vals]


def test_naf_rotation_equals_composed_rotations(oracle_mod):
    o = oracle_mod.Oracle.bfv_default(4096)
    o.keygen(6)
    vals = list(range(100))
    ct = o.encrypt(o.encode(oracle_mod.expand_vector(vals, o.n)), 10)
    # 7 = 8 - 1 in NAF: no direct key, so the result must match the slot semantics anyway
    d = o.decode(o.decrypt(o.rotate(ct, 7)))
    assert list(d[:93]) == vals[7:]
    assert o.elt_from_step(7) not in o.galois_elts()


def test_ckks_pipeline_accuracy(oracle_mod):
    n = 4096
    primes = oracle_mod.create_primes(n, [50, 40, 40, 50])
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    o.keygen(3)
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1, 1, n // 2), rng.uniform(-1, 1, n // 2)
    s = 2.0 ** 40
    cx, cy = o.encrypt(o.ckks_encode(x, s), 1), o.encrypt(o.ckks_encode(y, s), 2)
    m = o.rescale(o.mul_relin(cx, cy))
    got = o.ckks_decode(o.decrypt(m), s * s / primes[2]).real
    assert np.abs(got - x * y).max() < 1e-6   # CKKS is approximate: tolerance, not bit parity
    r = o.ckks_decode(o.decrypt(o.rotate(cx, 5)), s).real
    assert np.abs(r - np.roll(x, -5)).max() < 1e-5


def test_sampler_spec_is_deterministic(oracle_mod):
    a = oracle_mod.Oracle.bfv_default(4096)
    b = oracle_mod.Oracle.bfv_default(4096)
    a.keygen(11)
    b.keygen(11)
    assert np.array_equal(a.relin_key(), b.relin_key())
    b.keygen(12)
    assert not np.array_equal(a.relin_key(), b.relin_key())


def test_bfv_multiply_does_not_depend_on_the_auxiliary_base(oracle_mod):
    """BEHZ: every step of the multiply computes residues of one fixed integer, so the q-residues of the result must be the
    same whichever auxiliary primes carry the intermediate values.  SEAL draws m_sk and B from the 61-bit primes; the HIP
    backend draws them from the 50-bit ones where that puts every BEHZ transform on its exact-fp64 path.  Here: the oracle
    with ORC_BEHZ_AUX_BITS = 50 / 45 against the oracle with SEAL's base, on ordinary and on adversarial ciphertexts."""
    import os
    rng = np.random.default_rng(61)
    for n in (4096, 8192):
        primes, t = oracle_mod.default_bfv_primes(n), oracle_mod.plain_modulus_batching(n, 20)
        os.environ.pop("ORC_BEHZ_AUX_BITS", None)
        ref = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)
        ref.keygen(3)
        L = len(primes) - 1
        a = ref.encrypt(ref.encode(oracle_mod.expand_vector([3, 3, 1, 4, 5, 9], n)), 1)
        b = ref.encrypt(ref.encode(oracle_mod.expand_vector([0, 1, 2, 1, 10, 21], n)), 2)
        ex = np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in primes[:L]], axis=1)
        for j in range(L):
            ex[0, j, : n // 2] = primes[j] - 1
            ex[1, j, ::2] = 0
        want = [ref.multiply(a, b), ref.multiply(ex, ex), ref.multiply(a, ex)]
        for bits in (50, 45):
            os.environ["ORC_BEHZ_AUX_BITS"] = str(bits)
            try:
                alt = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)
            finally:
                os.environ.pop("ORC_BEHZ_AUX_BITS", None)
            got = [alt.multiply(a, b), alt.multiply(ex, ex), alt.multiply(a, ex)]
            for w, g_ in zip(want, got):
                assert np.array_equal(w, g_), (n, bits)


def test_timed_mul_relin_bfv_default_ring_runs_in_its_arena(oracle_mod):
    """orc_time_mul_relin (bench.py's cpu_baseline leg) bump-allocates every temporary of one multiply from an arena: BFV on
    BFVDefault(16384) needs ~300 limbs of it (the arena is sized from the scheme, and falls back to the heap when short)."""
    o = oracle_mod.Oracle.bfv_default(16384)
    o.keygen(5)
    a = o.encrypt(o.encode(oracle_mod.expand_vector([3, 3, 1, 4, 5, 9], o.n)), 1)
    b = o.encrypt(o.encode(oracle_mod.expand_vector([0, 1, 2, 1, 10, 21], o.n)), 2)
    assert o.time_mul_relin(a, b, 1) > 0.0
    assert list(o.decode(o.decrypt(o.mul_relin(a, b)))[:6]) == [0, 3, 2, 4, 50, 189]


def test_keygen_for_chosen_galois_elements(oracle_mod):
    """Oracle.keygen(seed, elts): the default list gives orc_keygen's keys bit for bit; a sub-list changes no other key, and its first
    key is the default run's first key (both are sampled right after the relin key)."""
    n = 4096
    primes = oracle_mod.create_primes(n, [40, 40, 41])
    full, same, part = (oracle_mod.Oracle(oracle_mod.CKKS, n, primes) for _ in range(3))
    full.keygen(21)
    elts = full.galois_elts()
    assert len(elts) == 2 * (full.logn - 1) and elts[0] == 2 * n - 1  # 3^(N/4) is named twice in the default list: one key
    default_list = [2 * n - 1]
    pos, neg = 3, pow(3, -1, 2 * n)
    for _ in range(full.logn - 1):
        default_list += [pos, neg]
        pos, neg = pos * pos % (2 * n), neg * neg % (2 * n)
    same.keygen(21, elts=default_list)
    assert same.galois_elts() == elts
    sub = [elts[0], full.elt_from_step(8), elts[0], full.elt_from_step(1)]  # a duplicate is skipped
    part.keygen(21, elts=sub)
    assert part.galois_elts() == [sub[0], sub[1], sub[3]]
    for other in (same, part):
        assert np.array_equal(other.secret_key(), full.secret_key())
        assert np.array_equal(other.public_key(), full.public_key())
        assert np.array_equal(other.relin_key(), full.relin_key())
    for e in elts:
        assert np.array_equal(same.galois_key(e), full.galois_key(e)), e
    assert np.array_equal(part.galois_key(sub[0]), full.galois_key(elts[0]))
    # later keys follow other draws of the stream, but they are keys for their element: a rotation decrypts to the rotated slots
    bfv = oracle_mod.Oracle.bfv_default(n)
    bfv.keygen(5, elts=[bfv.elt_from_step(1)])
    ct = bfv.encrypt(bfv.encode(oracle_mod.expand_vector([1, 2, 3, 4], n)), 3)
    assert list(bfv.decode(bfv.decrypt(bfv.rotate(ct, 1)))[:3]) == [2, 3, 4]
    with pytest.raises(RuntimeError):
        bfv.rotate(ct, 2)  # no key for that step
    none = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    none.keygen(21, elts=[])
    assert none.galois_elts() == [] and np.array_equal(none.relin_key(), full.relin_key())


@pytest.mark.parametrize("size", [2, 3])
def test_ckks_plain_ops_are_componentwise_integer_arithmetic(size, oracle_mod):
    """orc_ckks_multiply_plain / _add_plain / _sub_plain against Python integers, below the top level (nl = 2 of L = 3, one prime of
    60 bits): every component times p; only component 0 plus or minus p, the others unchanged"""
    n, nl = 1024, 2
    primes = oracle_mod.create_primes(n, [60, 40, 50, 60])
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    assert nl < o.L
    rng = np.random.default_rng(size)
    ct = np.stack([rng.integers(0, q, size=(size, n), dtype=np.uint64) for q in primes[:nl]], axis=1)
    pl = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in primes[:nl]])
    for j, q in enumerate(primes[:nl]):  # ends of the range, and a - a / a + (q - a)
        ct[:, j, :4] = [0, 1, q - 1, (q - 1) // 2]
        pl[j, :8] = [0, 1, q - 1, (q - 1) // 2, q - 1, 0, 1, q - 2]
        pl[j, 8] = ct[0, j, 8]
        pl[j, 9] = (q - int(ct[0, j, 9])) % q
    got = {"mul": o.multiply_plain(ct, pl), "add": o.add_plain(ct, pl), "sub": o.sub_plain(ct, pl)}
    for j, q in enumerate(primes[:nl]):
        p = [int(v) for v in pl[j]]
        for c in range(size):
            x = [int(v) for v in ct[c, j]]
            assert [int(v) for v in got["mul"][c, j]] == [a * b % q for a, b in zip(x, p)], (c, j)
            assert [int(v) for v in got["add"][c, j]] == ([(a + b) % q for a, b in zip(x, p)] if c == 0 else x), (c, j)
            assert [int(v) for v in got["sub"][c, j]] == ([(a - b) % q for a, b in zip(x, p)] if c == 0 else x), (c, j)
    assert got["sub"][0, 0, 8] == 0 and got["add"][0, 0, 9] == 0
    # BFV keeps its own function
    b = oracle_mod.Oracle.bfv_default(4096)
    cb = np.stack([rng.integers(0, q, size=(2, 4096), dtype=np.uint64) for q in b.primes[:b.L]], axis=1)
    pb = rng.integers(0, b.t, size=4096, dtype=np.uint64)
    back = b.add_plain(b.sub_plain(cb, pb), pb)
    assert np.array_equal(back, cb) and not np.array_equal(b.sub_plain(cb, pb), cb)
