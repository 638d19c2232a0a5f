"""Keys and fresh ciphertexts made on the device (abc_hip_keygen*, abc_hip_encrypt*, abc_amd/csrc/abc_keys.hip), word for word, on
every ring 2^10 .. 2^16 and every chain family.  A ciphertext made with the wrong u, the wrong draw offset, a stream reused across a
batch or the wrong public-key component still decrypts, and the residual of a fresh encryption is the rounding noise of the division
by the special prime, not the sampled errors: only word parity against a reference that contains the draws can tell.  So

  * the seeded entries (abc_hip_keygen, abc_hip_encrypt) are compared with the oracle, which draws the same seeded spec;
  * abc_hip_encrypt_keyed is compared with the big-integer model of tests/key_material_spec.py under the draws of
    tests/keyed_spec.py, also under ABC_HIP_HOST_SAMPLING=1, and abc_hip_keygen_keyed with its definition (key_equation; that the host
    twin makes the same keys is tests/test_gpu_keyed_sampling.py's);
  * the device's use of its own keys (the key words and the mirrors built at keygen: fp64 twin, Shoup quotients) is tied to the
    oracle's use of the same words: o.keyswitch(target, g.get_key(...)) == g.keyswitch(target, ...);
  * loaded keys come back as loaded and are replaced as a whole; the calls that need a key refuse without one and leave the context
    usable.

What no entry point can show -- the errors e0, e1 of an encryption -- is stated in tests/key_material_spec.py; the CPU side of the
model is tests/test_key_material_spec.py."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyed_spec as ks  # noqa: E402
import key_material_spec as km  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
KEY_SEC, KEY_PUB = bytes(range(64, 96)), bytes(range(160, 192))
WRAP_NONCE = 0xFFFFFFFFFFFFFFFE  # nonce + 2 wraps: the stream id changes its high word inside a batch of 3
SEED = 0x4B455953
SCALE = 2.0 ** 30
GRID_THREADS = 8192 * 256  # grid_for's cap (abc_context.hpp): more items than this and a grid-stride loop runs again
FEW_LIMBS = 48  # ABC_HIP_FEW_LIMBS' default: at N = 2^14 the stand-alone transforms of at most this many limbs take the spread form

# id -> (scheme, N, key prime bit sizes or None for BFVDefault(N), key primes K), each chosen for the route it forces
CONTEXTS = {
    "ckks1024": ("ckks", 1 << 10, [36, 50, 60], 3),  # three widths, 60-bit special prime
    "ckks2048": ("ckks", 1 << 11, [50, 40, 50], 3),  # the LB = 11 pass schedule, all fp64
    "bfv4096": ("bfv", 1 << 12, None, 3),  # the shape of test_gpu_parity.py's test_keygen_matches_oracle
    "bfv8192": ("bfv", 1 << 13, None, 5),  # LB = 13, five key primes
    "ckks8192w": ("ckks", 1 << 13, [60, 40, 40, 60], 4),  # mixed: guarded integer ends, fp64 middle
    "ckks16384": ("ckks", 1 << 14, [50, 40, 40, 40, 50], 5),  # spread transforms for a key and one encryption, block form for a batch of 5
    "bfv16384": ("bfv", 1 << 14, None, 9),  # 72 limbs per key: block form
    "ckks32768": ("ckks", 1 << 15, [50, 40, 50], 3),  # strided + block, fp64
    "ckks32768w": ("ckks", 1 << 15, [60, 40, 60], 3),  # strided + block, integer
    "ckks65536": ("ckks", 1 << 16, [50, 40, 50], 3),  # radix-16 strided pass
    "bfv65536": ("bfv", 1 << 16, [49, 49, 50], 3),  # the BFV branch on the biggest ring, t = plain_modulus_batching(65536, 20)
}
# bfv16384: a default key set is half a gigabyte.  The oracle makes the first three Galois keys, a prefix of the device's order
# (tests/test_gpu_hoisted_rotations.py), and those are compared
ORACLE_GALOIS_KEYS = {"bfv16384": 3}


def default_elts(n):
    """GaloisTool::get_elts_all: 2N - 1, then 3^(2^i), 3^-(2^i); an element named twice once"""
    m = 2 * n
    elts, pos, neg = [m - 1], 3, pow(3, -1, m)
    for _ in range(n.bit_length() - 2):
        elts += [pos, neg]
        pos, neg = pos * pos % m, neg * neg % m
    return list(dict.fromkeys(elts))


def _oracle(om, name):
    scheme, n, bits, _ = CONTEXTS[name]
    if bits is None:
        return om.Oracle.bfv_default(n)
    primes = om.create_primes(n, bits)
    if scheme == "ckks":
        return om.Oracle(om.CKKS, n, primes)
    return om.Oracle(om.BFV, n, primes, om.plain_modulus_batching(n, 20))


def _context(capi, o):
    return capi.Context(capi.CKKS if o.scheme == 2 else capi.BFV, o.n, o.primes, o.t)


@contextlib.contextmanager
def host_sampling(g):
    """ABC_HIP_HOST_SAMPLING=1 on context g inside the block, the default again behind it"""
    os.environ["ABC_HIP_HOST_SAMPLING"] = "1"
    g.reload_env()
    try:
        yield
    finally:
        os.environ.pop("ABC_HIP_HOST_SAMPLING", None)
        g.reload_env()


@pytest.fixture(scope="module")
def rings(oracle_mod, capi):
    """name, keys -> (oracle, context).  The oracle has keygen(SEED) (made once); the device has keygen(SEED) for keys="seeded" and
    keygen_keyed(KEY_SEC, KEY_PUB) for keys="keyed", regenerated in place when a test asks for the other kind"""
    made, device_keys = {}, {}

    def get(name, keys):
        if name not in made:
            o = _oracle(oracle_mod, name)
            o.keygen(SEED, elts=default_elts(o.n)[:ORACLE_GALOIS_KEYS[name]] if name in ORACLE_GALOIS_KEYS else None)
            made[name] = (o, _context(capi, o))
        o, g = made[name]
        if device_keys.get(name) != keys:
            device_keys[name] = None
            if keys == "seeded":
                g.keygen(SEED)
            else:
                g.keygen_keyed(KEY_SEC, KEY_PUB)
            device_keys[name] = keys
        return o, g

    yield get
    for _, g in made.values():
        g.close()


def _plains(o, count, seed):
    """count different plaintexts as encrypt takes them: BFV [count][N] random values mod t, CKKS [count][L][N] encoded random slots"""
    rng = np.random.default_rng(seed)
    if o.scheme == 2:
        return np.stack([o.ckks_encode(rng.uniform(-1, 1, o.n // 2), SCALE) for _ in range(count)])
    return rng.integers(0, o.t, (count, o.n), dtype=np.uint64)


def _target(o, seed):
    """one polynomial [L][N] at the top level: of every limb half the positions from the ends and the middle of its range, half random"""
    rng = np.random.default_rng(seed)
    rows = []
    for q in o.primes[:o.L]:
        edge = rng.choice(np.array([0, 1, q - 1, q - 2, q // 2, q // 2 + 1], dtype=np.uint64), size=o.n)
        rows.append(np.where(rng.random(o.n) < 0.5, edge, rng.integers(0, q, size=o.n, dtype=np.uint64)))
    return np.stack(rows)


def _check_shape(name, o, g):
    """what the table says of a context, where an entry point shows it"""
    scheme, n, bits, K = CONTEXTS[name]
    assert (g.n, g.K, g.L, g.scheme) == (n, K, K - 1, 2 if scheme == "ckks" else 1)
    assert g.primes == o.primes and len(set(g.primes)) == K
    if bits is not None:
        assert [q.bit_length() for q in g.primes] == bits
    if scheme == "bfv":
        assert g.t == o.t and g.t % (2 * n) == 1 and g.t.bit_length() == 20
    if name == "ckks16384":  # limbs through one stand-alone transform call: a key's errors, one encryption's, a batch of five's
        assert g.L * g.K <= FEW_LIMBS and 2 * g.K <= FEW_LIMBS < 5 * 2 * g.K
    if name == "bfv16384":
        assert g.L * g.K == 72 > FEW_LIMBS


# ---- the seeded spec: the oracle draws the same words ----
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_seeded_keygen_matches_oracle(name, rings):
    o, g = rings(name, "seeded")
    _check_shape(name, o, g)
    km.same(name + " secret key", g.get_key("sk"), o.secret_key())
    km.same(name + " public key (component, limb, position)", g.get_key("pk"), o.public_key())
    km.same(name + " relin key (digit, component, limb, position)", g.get_key("relin"), o.relin_key())
    elts = default_elts(o.n)
    assert g.galois_elts() == elts
    compared = elts[:ORACLE_GALOIS_KEYS.get(name, len(elts))]
    assert o.galois_elts() == compared
    for e in compared:
        km.same("%s Galois key %d (digit, component, limb, position)" % (name, e), g.get_key("galois", e), o.galois_key(e))


def _encrypt_cases():
    for name in CONTEXTS:
        for count in (1, 5) + ((13,) if name == "ckks16384" else ()):
            yield pytest.param(name, count, id="%s-%d" % (name, count))


@pytest.mark.parametrize("name,count", list(_encrypt_cases()))
def test_seeded_encrypt_matches_oracle(name, count, rings):
    """row i of a batch is the oracle's encryption of plaintext i under seed + i"""
    o, g = rings(name, "seeded")
    _check_shape(name, o, g)
    items = count * 2 * o.K * o.n
    if count == 13:  # k_enc_mul_pk, k_acc_add and k_small_to_rns take a second, ragged pass
        assert GRID_THREADS < items < 2 * GRID_THREADS and items % GRID_THREADS
    else:
        assert items <= GRID_THREADS
    pls = _plains(o, count, 100 + count)
    seed = 0xE0000 + count
    got = g.encrypt(pls, seed)
    assert got.shape == (count, 2, o.L, o.n)
    for i in range(count):
        km.same("%s ciphertext %d of %d (component, limb, position)" % (name, i, count), got[i], o.encrypt(pls[i], seed + i))


# ---- the keyed spec: the model and the definition ----
@pytest.mark.parametrize("name", ["ckks1024", "bfv4096", "ckks2048"])
def test_keyed_encrypt_matches_model(name, rings):
    """ciphertext i == fresh_ciphertext(the device's own public key, the draws of stream nonce + i, plaintext i); the stream id wraps
    inside the batch"""
    o, g = rings(name, "keyed")
    count = 3
    pls = _plains(o, count, 31)
    small = ks.encrypt_small(KEY, WRAP_NONCE, o.n, count)
    pk = g.get_key("pk")
    want = np.stack([km.fresh_ciphertext(o, pk, small[i], pls[i]) for i in range(count)])
    got = g.encrypt_keyed(pls, KEY, WRAP_NONCE)
    for i in range(count):
        km.same("%s ciphertext %d (component, limb, position)" % (name, i), got[i], want[i])
    with host_sampling(g):
        got = g.encrypt_keyed(pls, KEY, WRAP_NONCE)
    for i in range(count):
        km.same("%s host sampling, ciphertext %d (component, limb, position)" % (name, i), got[i], want[i])


@pytest.mark.parametrize("name", ["ckks1024", "bfv4096", "ckks32768"])
def test_keyed_key_equation(name, rings):
    """the secret key is the spec's, and every word of the public key, the relinearisation key and the keys of elements 2N - 1 and 3
    is accounted for by a, s and e of the Python restatement"""
    o, g = rings(name, "keyed")
    n, L, primes = o.n, o.L, o.primes
    sk = g.get_key("sk")
    s = ks.secret(KEY_SEC, n)
    for j, q in enumerate(primes):
        km.same("%s secret key limb %d" % (name, j), o.intt(j, sk[j]), km.small_residues(s, q))
    sko = sk.astype(object)

    def check(what, key, stream, nkeys, new_key):
        assert len(key) == nkeys
        km.key_equation(o, key, ks.key_uniform(KEY_PUB, stream, n, primes, nkeys), ks.key_errors(KEY_SEC, stream, n, nkeys), sk, new_key,
                        name + " " + what)

    check("pk", g.get_key("pk")[None], 1, 1, None)
    check("relin", g.get_key("relin"), 2, L, np.stack([(sko[j] * sko[j] % q).astype(np.uint64) for j, q in enumerate(primes)]))
    for elt in (2 * n - 1, 3):
        assert elt in g.galois_elts()
        check("galois %d" % elt, g.get_key("galois", elt), 2 + elt, L, o.galois_permute(sk, elt, True))


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_device_keys_switch_like_the_oracle(name, rings):
    """the oracle switches with the words the device published; the device with its buffers and the mirrors it built at keygen"""
    o, g = rings(name, "keyed")
    _check_shape(name, o, g)
    target = _target(o, o.n + o.K)
    km.same(name + " key switch, relin key (component, limb, position)", g.keyswitch(target, 0), o.keyswitch(target, g.get_key("relin")))
    km.same(name + " key switch, key of element 3 (component, limb, position)", g.keyswitch(target, 3), o.keyswitch(target, g.get_key("galois", 3)))


# ---- loaded keys ----
@pytest.mark.parametrize("name", ["ckks16384", "bfv8192"])
def test_load_then_get_round_trip(name, oracle_mod, capi):
    first, second = _oracle(oracle_mod, name), _oracle(oracle_mod, name)
    elt = first.elt_from_step(1)
    first.keygen(SEED + 1, elts=[elt])
    second.keygen(SEED + 2, elts=[elt])
    assert not np.array_equal(first.relin_key(), second.relin_key())
    g = _context(capi, first)
    _check_shape(name, first, g)
    rng = np.random.default_rng(5)
    if first.scheme == 2:
        a, b = (np.stack([rng.integers(0, q, size=(2, first.n), dtype=np.uint64) for q in first.primes[:first.L]], axis=1) for _ in range(2))
    else:
        a, b = (first.encrypt(pl, 40 + i) for i, pl in enumerate(_plains(first, 2, 6)))
    try:
        for tag, o in (("first", first), ("second", second)):
            g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={elt: o.galois_key(elt)})
            assert g.galois_elts() == [elt]
            # one use of each key-switching key: their mirrors exist, and after the second load they are the second set's
            km.same("%s %s keys: mul_relin" % (name, tag), g.mul_relin(a, b), o.mul_relin(a, b))
            km.same("%s %s keys: rotate" % (name, tag), g.rotate(a, 1), o.rotate(a, 1))
            km.same("%s %s secret key" % (name, tag), g.get_key("sk"), o.secret_key())
            km.same("%s %s public key" % (name, tag), g.get_key("pk"), o.public_key())
            km.same("%s %s relin key" % (name, tag), g.get_key("relin"), o.relin_key())
            km.same("%s %s Galois key" % (name, tag), g.get_key("galois", elt), o.galois_key(elt))
    finally:
        g.close()


# ---- refusals ----
# Every one is a host-side check that precedes every launch of its call: abc_hip_load_galois_key and get_key (abc_context.hip),
# no_public_key and decrypt (abc_keys.hip), relinearize, abc_hip_mul_relin and rotation_terms (abc_context.hip).
def _refusals(o, g):
    n, L = o.n, o.L
    ct, ct3, plain = np.zeros((2, L, n), np.uint64), np.zeros((3, L, n), np.uint64), np.zeros(n, np.uint64)
    key = np.zeros((L, 2, o.K, n), np.uint64)
    return {
        "encrypt": lambda: g.encrypt(plain, 1),
        "encrypt_keyed": lambda: g.encrypt_keyed(plain, KEY, 0),
        "encrypt_secure": lambda: g.encrypt(plain, None),
        "decrypt": lambda: g.decrypt(ct),
        "mul_relin": lambda: g.mul_relin(ct, ct),
        "relinearize": lambda: g.relinearize(ct3),
        "rotate": lambda: g.rotate(ct, 1),
        "get_sk": lambda: g.get_key("sk"),
        "get_pk": lambda: g.get_key("pk"),
        "get_relin": lambda: g.get_key("relin"),
        "get_galois": lambda: g.get_key("galois", 3),
        "load_even_element": lambda: g.load_keys(galois={4: key}),
        "load_element_above_2n": lambda: g.load_keys(galois={2 * n + 1: key}),
    }


REFUSALS = ["encrypt", "encrypt_keyed", "encrypt_secure", "decrypt", "mul_relin", "relinearize", "rotate", "get_sk", "get_pk", "get_relin",
            "get_galois", "load_even_element", "load_element_above_2n"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(what, oracle_mod, capi):
    """BFVDefault(4096) without keys: the call raises, and the context works afterwards -- keygen, then encrypt and decrypt"""
    o = _oracle(oracle_mod, "bfv4096")
    g = _context(capi, o)
    try:
        calls = _refusals(o, g)
        assert list(calls) == REFUSALS
        with pytest.raises(capi.AbcHipError):
            calls[what]()
        assert g.galois_elts() == []
        g.keygen(SEED)
        pls = _plains(o, 2, 9)
        km.same("round trip after the refused " + what, g.decrypt(g.encrypt(pls, 3)), pls)
    finally:
        g.close()
