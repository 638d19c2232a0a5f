"""The keyed sampling spec on the device: the draws of abc_kernels_sample.hip against the Python
restatement (tests/keyed_spec.py), the keyed / OS-keyed entry points against the host twin (ABC_HIP_HOST_SAMPLING=1), the
oracle's decryption and the key equation.  The CPU side of the same spec: tests/test_keyed_sampling_spec.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyed_spec as ks  # noqa: E402
from key_material_spec import key_equation  # noqa: E402

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
KEY_SEC, KEY_PUB = bytes(range(64, 96)), bytes(range(160, 192))
WRAP_NONCE = 0xFFFFFFFFFFFFFFFE  # nonce + 2 wraps: word 15 of the state changes inside a batch
SEED = 0x5EED
SCALE = 2.0 ** 40
D1 = [3, 3, 1, 4, 5, 9]
D2 = [0, 1, 2, 1, 10, 21]
# name -> (scheme, N, chain bit sizes or None for BFVDefault(N))
RINGS = {
    "bfv4096": ("bfv", 4096, None),
    "chain1024": ("ckks", 1024, [36, 50, 60]),  # three prime widths through the wide reduction
    "ckks4096": ("ckks", 4096, [50, 40, 50]),
    "bfv16384": ("bfv", 16384, None),  # 72 key limbs: more ChaCha20 blocks than the grid has threads
}


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d values differ, first at %s: got %s want %s"
                             % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _oracle(oracle_mod, name):
    scheme, n, bits = RINGS[name]
    if scheme == "ckks":
        return oracle_mod.Oracle(oracle_mod.CKKS, n, oracle_mod.create_primes(n, bits))
    return oracle_mod.Oracle.bfv_default(n)


def _context(capi, o):
    return capi.Context(capi.CKKS if o.scheme == 2 else capi.BFV, o.n, o.primes, o.t)


class HostSampling:
    """ABC_HIP_HOST_SAMPLING=1 on context g inside the block, the default again behind it"""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        os.environ["ABC_HIP_HOST_SAMPLING"] = "1"
        self.g.reload_env()

    def __exit__(self, *exc):
        os.environ.pop("ABC_HIP_HOST_SAMPLING", None)
        self.g.reload_env()


@pytest.fixture(scope="module")
def rings(oracle_mod, capi):
    """name -> (oracle, context); keys=True: both with keygen(SEED), the shared seeded spec gives them the same keys"""
    made, keyed = {}, set()

    def get(name, keys=False):
        if name not in made:
            o = _oracle(oracle_mod, name)
            made[name] = (o, _context(capi, o))
        o, g = made[name]
        if keys and name not in keyed:
            o.keygen(SEED)
            g.keygen(SEED)
            keyed.add(name)
        return o, g

    yield get
    for _, g in made.values():
        g.close()


# ---- the raw draws ----
@pytest.mark.parametrize("name", list(RINGS))
def test_keyed_small_matches_spec(name, rings):
    o, g = rings(name)
    for count, nonce in ((1, 11), (3, WRAP_NONCE), (5, WRAP_NONCE - 1)):
        _same("%s count %d" % (name, count), g.keyed_small(KEY, nonce, count), ks.encrypt_small(KEY, nonce, o.n, count))


def test_keyed_small_grid_stride(rings):
    """44 ciphertexts at N = 2^14 are 270 336 blocks, the grid 262 144 threads: the loop runs twice, the second pass ragged"""
    o, g = rings("bfv16384")
    got = g.keyed_small(KEY, 3, 44)
    _same("44 x 2^14", got, ks.encrypt_small(KEY, 3, o.n, 44))
    assert set(np.unique(got[:, 0])) == {-1, 0, 1} and np.abs(got[:, 1:].astype(int)).max() <= 21


@pytest.mark.parametrize("name", list(RINGS))
def test_keyed_uniform_matches_spec(name, rings):
    o, g = rings(name)
    streams = (1, 2, 2 + (2 * o.n - 1))
    for nkeys, stream in ((1, streams[0]), (o.L, streams[1]), (o.L if o.L < 8 else 1, streams[2])):
        got = g.keyed_uniform(KEY_PUB, stream, nkeys)
        _same("%s nkeys %d stream %d" % (name, nkeys, stream), got, ks.key_uniform(KEY_PUB, stream, o.n, o.primes, nkeys))
    with HostSampling(g):
        _same(name + " host twin", g.keyed_uniform(KEY_PUB, 2, 1), ks.key_uniform(KEY_PUB, 2, o.n, o.primes, 1))
        _same(name + " host twin, small", g.keyed_small(KEY, WRAP_NONCE, 3), ks.encrypt_small(KEY, WRAP_NONCE, o.n, 3))


def test_keyed_entries_check_their_arguments(rings, capi):
    o, g = rings("bfv4096")
    with pytest.raises(capi.AbcHipError):
        g.keyed_uniform(KEY_PUB, 1, o.L + 1)
    with pytest.raises(capi.AbcHipError):
        g.keyed_uniform(KEY_PUB, 1, 0)
    with pytest.raises(ValueError):
        g.keyed_small(KEY[:16], 0, 1)


# ---- encryption ----
def _plains(o, count, seed):
    rng = np.random.default_rng(seed)
    if o.scheme == 2:
        vals = rng.uniform(-1, 1, (count, o.n // 2))
        return vals, np.stack([o.ckks_encode(v, SCALE) for v in vals])
    vals = rng.integers(0, o.t, (count, o.n))
    return vals, np.stack([o.encode(v) for v in vals])


@pytest.mark.parametrize("name", ["bfv4096", "ckks4096"])
@pytest.mark.parametrize("count", [1, 5])
def test_encrypt_keyed(name, count, rings):
    """device draws == host twin, ciphertext i == the single call with nonce + i, and the oracle (same seeded keys) decrypts them"""
    o, g = rings(name, keys=True)
    vals, pls = _plains(o, count, 7)
    nonce = WRAP_NONCE - 1
    cts = g.encrypt_keyed(pls, KEY, nonce)
    assert cts.shape == (count, 2, o.L, o.n)
    with HostSampling(g):
        _same(name + " host sampling", g.encrypt_keyed(pls, KEY, nonce), cts)
    for i in range(count):
        _same(name + " single call %d" % i, g.encrypt_keyed(pls[i], KEY, nonce + i), cts[i])
        if o.scheme == 2:
            # |error of a coefficient| <= |e0| + |e1 s| + |u e| + rounding < 21 (2N + 1) + N + 2 < 2^18.5 at N = 2^12; a slot sums N
            # coefficients times roots of unity: below 2^30.5 / scale = 2^-9.5
            assert np.abs(o.ckks_decode(o.decrypt(cts[i]), SCALE).real - vals[i]).max() < 2.0 ** -9
        else:
            _same(name + " oracle decrypt %d" % i, o.decrypt(cts[i]), pls[i])
    if count > 1:
        assert len({cts[i].tobytes() for i in range(count)}) == count


def test_encrypt_secure_is_fresh_and_decrypts(rings):
    o, g = rings("bfv4096", keys=True)
    _, pls = _plains(o, 5, 8)
    a, b = g.encrypt(pls, None), g.encrypt(pls, None)
    assert not np.array_equal(a, b)
    assert len({x.tobytes() for x in list(a) + list(b)}) == 10
    for cts in (a, b):
        for i in range(5):
            _same("oracle decrypt %d" % i, o.decrypt(cts[i]), pls[i])
    with HostSampling(g):
        c, d = g.encrypt(pls, None), g.encrypt(pls, None)  # the host twin under a fresh OS key per call
    assert not np.array_equal(a, c)
    assert not np.array_equal(c, d)
    _same("host-sampled secure encryption decrypts", g.decrypt(c), pls)


# ---- key generation ----
def test_secure_entries_under_host_sampling(oracle_mod, capi):
    """OS-keyed key generation and encryption through the host twin: fresh keys per call, regenerated in place, and the keys
    serve the device sampler afterwards"""
    o = _oracle(oracle_mod, "bfv4096")
    g = _context(capi, o)
    _, pls = _plains(o, 2, 9)
    with HostSampling(g):
        g.keygen(None)
        first = g.get_key("sk")
        g.keygen(None)
        assert not np.array_equal(g.get_key("sk"), first)
        assert g.held_buffers() == 0  # every key regenerated into the buffer it had
        _same("host-sampled keys and encryption", g.decrypt(g.encrypt(pls, None)), pls)
    _same("host-sampled keys, device-sampled encryption", g.decrypt(g.encrypt(pls, None)), pls)
    g.close()


def _all_keys(g, elts):
    return [("sk", g.get_key("sk")), ("pk", g.get_key("pk")), ("relin", g.get_key("relin"))] + \
        [("galois %d" % e, g.get_key("galois", e)) for e in elts]


@pytest.mark.parametrize("name", ["chain1024", "bfv4096"])
def test_keygen_keyed_host_device_identical(name, oracle_mod, capi):
    o = _oracle(oracle_mod, name)
    g = _context(capi, o)
    g.keygen_keyed(KEY_SEC, KEY_PUB)
    elts = [2 * o.n - 1, 3]
    assert set(elts) <= set(g.galois_elts())
    dev = _all_keys(g, elts)
    with HostSampling(g):
        g.keygen_keyed(KEY_SEC, KEY_PUB)
    for (what, a), (_, b) in zip(dev, _all_keys(g, elts)):
        _same(name + " " + what, b, a)
    g.keygen_keyed(KEY_PUB, KEY_SEC)  # other keys: other words
    assert not np.array_equal(g.get_key("sk"), dev[0][1])
    g.close()


def test_key_equation(oracle_mod, capi):
    """every published word is accounted for by the spec: key[i][1][j] = a_i[j], and key[i][0][j] + a s - [j == i] (q_sp mod q_i)
    new_key = -e_i, exactly, with s, a and e from the Python restatement"""
    o = _oracle(oracle_mod, "chain1024")
    g = _context(capi, o)
    g.keygen_keyed(KEY_SEC, KEY_PUB)
    n, L, primes = o.n, o.L, o.primes
    sk = g.get_key("sk")
    s = ks.secret(KEY_SEC, n).astype(np.int64)
    for j, q in enumerate(primes):
        _same("secret key limb %d" % j, o.intt(j, sk[j]), (s % q).astype(np.uint64))
    sko = sk.astype(object)

    def check(what, key, stream, nkeys, new_key):
        a = ks.key_uniform(KEY_PUB, stream, n, primes, nkeys)
        e = ks.key_errors(KEY_SEC, stream, n, nkeys)
        assert len(key) == nkeys
        key_equation(o, key, a, e, sk, new_key, what)  # tests/key_material_spec.py

    check("pk", g.get_key("pk")[None], 1, 1, None)
    check("relin", g.get_key("relin"), 2, L, np.stack([(sko[j] * sko[j] % q).astype(np.uint64) for j, q in enumerate(primes)]))
    elt = 2 * n - 1
    check("galois", g.get_key("galois", elt), 2 + elt, L, o.galois_permute(sk, elt, True))
    g.close()


@pytest.mark.parametrize("how", ["keyed", "secure"])
def test_operations_under_device_sampled_keys(how, oracle_mod, capi):
    """BFVDefault(4096): encrypt, mul_relin, rotate by 1 and by 7 (= 8 - 1: two hops), decrypt"""
    o = oracle_mod.Oracle.bfv_default(4096)
    o.keygen(SEED)  # for the expected slots only: they do not depend on the keys
    g = capi.Context.bfv_default(4096)
    if how == "keyed":
        g.keygen_keyed(KEY_SEC, KEY_PUB)
    else:
        g.keygen(None)
    pls = np.stack([o.encode(np.array(oracle_mod.expand_vector(d, o.n), dtype=np.int64)) for d in (D1, D2)])
    cts = g.encrypt_keyed(pls, KEY, 0) if how == "keyed" else g.encrypt(pls, None)
    _same("decrypt", g.decrypt(cts), pls)
    prod = g.mul_relin(cts[0], cts[1])
    assert list(o.decode(g.decrypt(prod))[:6]) == [0, 3, 2, 4, 50, 189]
    ref = o.encrypt(pls[0], 1)
    for step in (1, 7):
        _same("rotate %d" % step, o.decode(g.decrypt(g.rotate(cts[0], step))), o.decode(o.decrypt(o.rotate(ref, step))))
    g.close()


def test_recorded_graph_replays_after_keygen_keyed(oracle_mod, capi):
    """keys are rewritten in place (include/abc_hip.h, graphs): a circuit recorded under seeded keys computes under the keyed ones"""
    o = oracle_mod.Oracle.bfv_default(4096)
    o.keygen(SEED)
    g = capi.Context.bfv_default(4096)
    g.keygen(SEED)
    pls = np.stack([o.encode(np.array(oracle_mod.expand_vector(d, o.n), dtype=np.int64)) for d in (D1, D2)])
    a, b = o.encrypt(pls[0], 1), o.encrypt(pls[1], 2)
    da, db = g.upload(a), g.upload(b)
    tmp, out = g.alloc(a.nbytes), g.alloc(a.nbytes)
    one = C.c_size_t(1)

    def circuit():
        g.op("mul_relin", da.ptr, db.ptr, tmp.ptr, g.L, one)
        g.op("rotate", tmp.ptr, out.ptr, g.L, 1, one)

    circuit()
    g.sync()
    g.graph_begin()
    circuit()
    graph = g.graph_end()
    g.graph_launch(graph)
    g.sync()
    want = o.rotate(o.mul_relin(a, b), 1)
    _same("replay under the recorded keys", g.download(out, a.shape), want)
    g.keygen_keyed(KEY_SEC, KEY_PUB)
    assert g.held_buffers() == 0  # every key regenerated into the buffer it had
    cts = g.encrypt_keyed(pls, KEY, 0)
    for buf, ct in ((da, cts[0]), (db, cts[1])):
        g.op("memcpy_h2d", buf.ptr, ct.ctypes.data_as(C.c_void_p), C.c_size_t(ct.nbytes))
    g.graph_launch(graph)
    g.sync()
    got = g.download(out, a.shape)
    assert not np.array_equal(got, want)
    _same("replay under the keyed keys: slots", o.decode(g.decrypt(got)), o.decode(o.decrypt(want)))
    g.graph_destroy(graph)
    g.close()
