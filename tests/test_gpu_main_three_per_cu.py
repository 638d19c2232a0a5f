"""GPU parity of the two forms of the key-switch main kernel (k_split4_main_fp, N = 2^14, up to four data limbs).

The default form runs its pair phase one output component at a time and requests that phase's operands after the transform
(80 VGPRs or fewer: three workgroups per CU); ABC_HIP_MAIN_TWO_PER_CU=1 selects the one-piece pair phase with every operand
requested before the transform (two workgroups per CU).  Same step, same route, same arithmetic: every case below runs under
both settings and must return the oracle's residues bit for bit.  The kernel is fixed to N = 2^14, so the small dimension is
the number of ciphertexts.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16384
FORMS = {"three_per_cu": {}, "two_per_cu": {"ABC_HIP_MAIN_TWO_PER_CU": "1"}}
_SPLIT4 = "split14 front=lean pack=1 main=split4"


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s: got %d want %d" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _random_ct(primes, nl, rng):
    return np.stack([rng.integers(0, q, size=(2, N), dtype=np.uint64) for q in primes[:nl]], axis=1)


def _runs_ct(primes, nl, rng, shift):
    """residues from {0, 1, (q-1)/2, (q+1)/2, q-2, q-1} and random values, over long runs of q-1, (q-1)/2, (q+1)/2 and 0
    (`shift` moves the runs, so that two operands meet in different combinations)"""
    ct = np.empty((2, nl, N), dtype=np.uint64)
    for j in range(nl):
        q = primes[j]
        pool = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
        pick = rng.integers(0, 8, size=(2, N))
        rnd = rng.integers(0, q, size=(2, N), dtype=np.uint64)
        ct[:, j, :] = np.where(pick < 6, pool[np.minimum(pick, 5)], rnd)
        run = N // 8
        for r, v in enumerate([q - 1, (q - 1) // 2, (q + 1) // 2, 0]):
            lo = ((r + shift) % 8) * run
            ct[r & 1, j, lo:lo + run] = v
            ct[1 - (r & 1), j, lo + run // 2:lo + run] = v
    return ct


class _Chain:
    """one oracle per prime chain, its keys, and a cache of expected results (computed once, shared by both forms)"""

    def __init__(self, om, bits, seed):
        self.primes = om.create_primes(N, bits)
        self.o = om.Oracle(om.CKKS, N, self.primes)
        self.o.keygen(seed)
        self.L = len(bits) - 1
        rng = np.random.default_rng(seed)
        self.x = {nl: _random_ct(self.primes, nl, rng) for nl in range(1, self.L + 1)}
        self.y = {nl: _random_ct(self.primes, nl, rng) for nl in range(1, self.L + 1)}
        self.ex = {nl: _runs_ct(self.primes, nl, rng, 0) for nl in range(1, self.L + 1)}
        self.ey = {nl: _runs_ct(self.primes, nl, rng, 3) for nl in range(1, self.L + 1)}
        self._want = {}

    def want(self, key, fn):
        if key not in self._want:
            self._want[key] = fn()
        return self._want[key]

    def mul(self, nl, a, b):
        ops = {"x": self.x, "y": self.y, "ex": self.ex, "ey": self.ey}
        return self.want(("mul", nl, a, b), lambda: self.o.mul_relin(ops[a][nl], ops[b][nl]))

    def context(self, capi, monkeypatch, form, env=None):
        for k, v in dict(FORMS[form], **(env or {})).items():
            monkeypatch.setenv(k, v)
        o = self.o
        g = capi.Context(capi.CKKS, N, self.primes)
        g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
        return g


@pytest.fixture(scope="module")
def hot(oracle_mod):
    return _Chain(oracle_mod, [50, 40, 40, 40, 50], 0xABC07001)


@pytest.fixture(scope="module")
def mixed_pack(oracle_mod):
    return _Chain(oracle_mod, [50, 48, 44, 36, 50], 0xABC07002)  # raw, 6-byte, 6-byte and 5-byte half-done limbs


@pytest.fixture(scope="module")
def wide_ends(oracle_mod):
    return _Chain(oracle_mod, [60, 40, 40, 40, 60], 0xABC07003)


PAIRS = [("x", "y"), ("ex", "ey"), ("y", "ex")]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
def test_mul_relin_every_level(nl, pairs, form, hot, capi, monkeypatch):
    g = hot.context(capi, monkeypatch, form)
    assert g.route("mul_relin", nl, pairs) == _SPLIT4
    ops = {"x": hot.x, "y": hot.y, "ex": hot.ex, "ey": hot.ey}
    a = np.stack([ops[p][nl] for p, _ in PAIRS[:pairs]])
    b = np.stack([ops[p][nl] for _, p in PAIRS[:pairs]])
    got = g.mul_relin(a, b)
    for i, (p, r) in enumerate(PAIRS[:pairs]):
        _same("%s mul_relin nl=%d pair %d of %d" % (form, nl, i, pairs), got[i], hot.mul(nl, p, r))
    g.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_mixed_packing_kinds_below_a_50_bit_special_prime(form, mixed_pack, capi, monkeypatch):
    """{50,48,44,36 | 50}: raw doubles, 6-byte and 5-byte packed half-done limbs all reach the main kernel's limb loads"""
    ch = mixed_pack
    g = ch.context(capi, monkeypatch, form)
    assert g.route("mul_relin", 4, 2) == _SPLIT4 and g.route("rotate", 4) == "fold " + _SPLIT4
    got = g.mul_relin(np.stack([ch.x[4], ch.ex[4]]), np.stack([ch.y[4], ch.ey[4]]))
    _same(form + " mixed packing mul_relin", got[0], ch.mul(4, "x", "y"))
    _same(form + " mixed packing mul_relin, runs", got[1], ch.mul(4, "ex", "ey"))
    _same(form + " mixed packing rotate", g.rotate(ch.ex[4], 5), ch.want("rot_ex", lambda: ch.o.rotate(ch.ex[4], 5)))
    g.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("twin", ["fp64_twin", "u64_keys"])
def test_key_twin_present_and_absent(twin, form, hot, capi, monkeypatch):
    """both instantiations of the pair phase: key words read as doubles from the key's fp64 twin, or converted per use"""
    g = hot.context(capi, monkeypatch, form, {"ABC_HIP_NO_KEY_TWIN": "1"} if twin == "u64_keys" else None)
    for nl in (4, 2):
        _same("%s %s mul_relin nl=%d" % (form, twin, nl), g.mul_relin(hot.x[nl], hot.y[nl]), hot.mul(nl, "x", "y"))
    _same("%s %s rotate" % (form, twin), g.rotate(hot.x[4], 5), hot.want(("rot", 4), lambda: hot.o.rotate(hot.x[4], 5)))
    g.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("alias", ["out_is_a", "out_is_b"])
def test_out_aliases_an_operand(alias, form, hot, capi, monkeypatch):
    """a and b are last read by the thread that then writes those words -- in both halves of the pair phase"""
    g = hot.context(capi, monkeypatch, form)
    a = np.stack([hot.x[4], hot.ex[4], hot.y[4]])
    b = np.stack([hot.y[4], hot.ey[4], hot.ex[4]])
    da, db = g.upload(a), g.upload(b)
    dst = da if alias == "out_is_a" else db
    g.op("mul_relin", da.ptr, db.ptr, dst.ptr, 4, C.c_size_t(3))
    res = g.download(dst, a.shape)
    for i, (p, r) in enumerate(PAIRS):
        _same("%s %s pair %d" % (form, alias, i), res[i], hot.mul(4, p, r))
    da.free(); db.free()
    g.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_runs_of_extreme_residues(form, hot, capi, monkeypatch):
    """long runs of q-1, (q-1)/2, (q+1)/2 and 0 in a and b, at every level: the ends of the fp64 magnitude bounds"""
    g = hot.context(capi, monkeypatch, form)
    for nl in (4, 3, 2, 1):
        _same("%s runs nl=%d" % (form, nl), g.mul_relin(hot.ex[nl], hot.ey[nl]), hot.mul(nl, "ex", "ey"))
        _same("%s runs squared nl=%d" % (form, nl), g.mul_relin(hot.ex[nl], hot.ex[nl]), hot.mul(nl, "ex", "ex"))
    g.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_main_step_over_a_subset_of_the_data_primes(form, wide_ends, capi, monkeypatch):
    """{60,40,40,40,60}: the integer sequence hands its three fp64-capable data primes to this kernel (ni = 3 < nl = 4, nibble map)"""
    ch = wide_ends
    g = ch.context(capi, monkeypatch, form)
    assert g.route("mul_relin", 4, 2) == "isplit14 guard=1 fpmask=0xe"
    got = g.mul_relin(np.stack([ch.x[4], ch.ex[4]]), np.stack([ch.y[4], ch.ey[4]]))
    _same(form + " 60-bit ends mul_relin", got[0], ch.mul(4, "x", "y"))
    _same(form + " 60-bit ends mul_relin, runs", got[1], ch.mul(4, "ex", "ey"))
    _same(form + " 60-bit ends rotate", g.rotate(ch.x[4], 5), ch.want("rot_x", lambda: ch.o.rotate(ch.x[4], 5)))
    g.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_ragged_multi_chunk_batch(form, hot, capi, monkeypatch):
    """five pairs in chunks of two: 2, 2, 1 over two lanes"""
    g = hot.context(capi, monkeypatch, form, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "2"})
    names = PAIRS + [("ex", "ex"), ("x", "y")]
    ops = {"x": hot.x, "y": hot.y, "ex": hot.ex, "ey": hot.ey}
    got = g.mul_relin(np.stack([ops[p][4] for p, _ in names]), np.stack([ops[r][4] for _, r in names]))
    for i, (p, r) in enumerate(names):
        _same("%s chunked pair %d" % (form, i), got[i], hot.mul(4, p, r))
    g.close()


def _galois_crosses_blocks(elt):
    """NTT-index form: slot i holds the evaluation at psi^(2 bitrev(i) + 1); does the gather for `elt` leave a 1024-point block?"""
    logn = N.bit_length() - 1
    i = np.arange(N, dtype=np.uint64)
    rev = np.zeros(N, dtype=np.uint64)
    for b in range(logn):
        rev |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(logn - 1 - b)
    src_rev = (((np.uint64(2) * rev + np.uint64(1)) * np.uint64(elt)) % np.uint64(2 * N) - np.uint64(1)) >> np.uint64(1)
    src = np.zeros(N, dtype=np.uint64)
    for b in range(logn):
        src |= ((src_rev >> np.uint64(b)) & np.uint64(1)) << np.uint64(logn - 1 - b)
    return bool(np.any((src >> np.uint64(10)) != (i >> np.uint64(10))))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
def test_rotate_and_relinearize_every_level(nl, form, hot, capi, monkeypatch):
    """the key-switch mode of the kernel: gathered diagonal operand and addends, (c0) for a rotation, (c0, c1) for relinearize"""
    g = hot.context(capi, monkeypatch, form)
    o = hot.o
    assert g.route("rotate", nl, 2) == "fold " + _SPLIT4
    assert _galois_crosses_blocks(g.elt_from_step(5))
    got = g.rotate(np.stack([hot.x[nl], hot.ex[nl]]), 5)
    _same("%s rotate nl=%d" % (form, nl), got[0], hot.want(("rot", nl), lambda: o.rotate(hot.x[nl], 5)))
    _same("%s rotate runs nl=%d" % (form, nl), got[1], hot.want(("rot_ex", nl), lambda: o.rotate(hot.ex[nl], 5)))
    t3 = hot.want(("t3", nl), lambda: o.multiply(hot.x[nl], hot.ey[nl]))
    _same("%s relinearize nl=%d" % (form, nl), g.relinearize(t3), hot.want(("relin", nl), lambda: o.relinearize(t3)))
    g.close()
