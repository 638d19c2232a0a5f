"""GPU parity of the light operations in every operand form the C ABI accepts (include/abc_hip.h), word for word against the CPU
oracle: one plaintext per ciphertext (plain_stride != 0) next to the broadcast form, size-3 operands, d_out aliasing an operand
(the reference's *_inplace call sites), abc_hip_apply_galois called directly, the BatchEncoder on every ring.

Inputs are residues, not encryptions (fuzz_parity.random_ct: uniform values plus 0, 1, (q +- 1)/2, q - 2, q - 1 and a run of
q - 1), so negate of 0 and a - a are in every batch.  Shapes are the smallest at which each path exists.

multiply_plain has two kernel sequences and its choice is not part of the route table (bfv_multiply_plain, abc_kernels_bfv.hip):
the fused forward / product / inverse kernel for rings 2^10 .. 2^13 with fp64 transforms and data primes below 2^50, and at
N = 2^14 only where count * size * L > 48; otherwise k_plain_lift, transforms, k_mul_plain_ntt.  Each test below names the
sequence its context takes and pins the facts that select it (ring, prime widths, switches, count * size * L).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_parity import random_ct  # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN_OPS = ("multiply_plain", "add_plain", "sub_plain")
_SPLIT14 = "split14 front=lean pack=1 main=split4"


def _report(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ; first at %s got %d want %d" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


_same = _report


def _naf(value):
    """non-adjacent form of a step count, as Evaluator::rotate_internal decomposes it"""
    out, i = [], 0
    while value:
        zi = 2 - (value & 3) if value & 1 else 0
        value = (value - zi) >> 1
        if zi:
            out.append(zi << i if zi > 0 else -((-zi) << i))
        i += 1
    return out


def _load_all_keys(o, g):
    g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})


# ---------------- contexts shared by several tests ----------------
@pytest.fixture(scope="module")
def bfv12(oracle_mod, capi):
    """BFVDefault(4096): two 36-bit data primes + special, every key"""
    o = oracle_mod.Oracle.bfv_default(4096)
    o.keygen(0xABC00021)
    g = capi.Context.bfv_default(4096)
    assert g.primes == o.primes and g.t == o.t
    _load_all_keys(o, g)
    yield o, g
    g.close()


def _ckks(oracle_mod, capi, n, bits, seed):
    primes = oracle_mod.create_primes(n, bits)
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    o.keygen(seed)
    g = capi.Context(capi.CKKS, n, primes)
    _load_all_keys(o, g)
    return o, g


@pytest.fixture(scope="module")
def ckks12(oracle_mod, capi):
    """CKKS N = 2^12, [50, 40, 40, 50]: three fp64 data limbs"""
    o, g = _ckks(oracle_mod, capi, 4096, [50, 40, 40, 50], 0xABC00022)
    yield o, g
    g.close()


@pytest.fixture(scope="module")
def ckks12_wide(oracle_mod, capi):
    """CKKS N = 2^12, [60, 40, 60]: mul_mod on a 60-bit prime"""
    o, g = _ckks(oracle_mod, capi, 4096, [60, 40, 60], 0xABC00023)
    yield o, g
    g.close()


@pytest.fixture(scope="module")
def ckks14(oracle_mod, capi):
    """CKKS N = 2^14, [50, 40, 40, 40, 50]: the benchmark's chain, rotations fold the permutation into the split key switch"""
    o, g = _ckks(oracle_mod, capi, 16384, [50, 40, 40, 40, 50], 0xABC00024)
    yield o, g
    g.close()


def _cts(rng, o, nl, batch, size=2):
    return random_ct(rng, [int(p) for p in o.primes], nl, o.n, batch, size=size)


# ---------------- raw calls: explicit stride, explicit aliasing ----------------
def _plain_call(g, op, ct, plain, stride, in_place):
    """abc_hip_<op>(ct, plain, stride, out) with out = a fresh buffer or ct itself; out of place also checks that ct is left alone"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    batch, size, nl, _ = ct.shape
    cb, pb = g.upload(ct), g.upload(np.ascontiguousarray(plain, dtype=np.uint64))
    out = cb if in_place else g.alloc(ct.nbytes)
    try:
        g.op(op, cb.ptr, pb.ptr, C.c_size_t(stride), out.ptr, size, nl, C.c_size_t(batch))
        res = g.download(out, ct.shape)
        if not in_place:
            _same(op + " left its input alone", g.download(cb, ct.shape), ct)
    finally:
        cb.free(); pb.free()
        if not in_place:
            out.free()
    return res


def _binop_call(g, op, a, b, alias):
    """add / sub / negate (b None) with out = fresh buffer (alias None), a ('a'), b ('b'); alias 'same': b IS a (a - a)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    batch, size, nl, _ = a.shape
    ba = g.upload(a)
    bb = ba if alias == "same" else g.upload(b) if b is not None else None
    out = ba if alias == "a" else bb if alias == "b" else g.alloc(a.nbytes)
    try:
        if bb is None:
            g.op(op, ba.ptr, out.ptr, size, nl, C.c_size_t(batch))
        else:
            g.op(op, ba.ptr, bb.ptr, out.ptr, size, nl, C.c_size_t(batch))
        return g.download(out, a.shape)
    finally:
        for buf in {id(x): x for x in (ba, bb, out) if x is not None}.values():
            buf.free()


def _rotate_call(g, ct, steps, in_place):
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    batch, _, nl, _ = ct.shape
    cb = g.upload(ct)
    out = cb if in_place else g.alloc(ct.nbytes)
    try:
        g.op("rotate", cb.ptr, out.ptr, nl, int(steps), C.c_size_t(batch))
        return g.download(out, ct.shape)
    finally:
        cb.free()
        if not in_place:
            out.free()


# ---------------- A. plain operations, BFV ----------------
def _bfv_plains(rng, t, n, rows):
    """rows of words in [0, t) with 0, 1, t - 1 and both sides of k_plain_lift's threshold (t + 1)/2 planted; the last row is all t - 1"""
    p = rng.integers(0, t, size=(rows, n), dtype=np.uint64)
    edge = np.array([0, 1, t - 1, (t - 1) // 2, (t + 1) // 2], dtype=np.uint64)
    for r in range(rows):
        p[r, rng.choice(n, size=40, replace=False)] = np.tile(edge, 8)
    p[rows - 1] = t - 1
    return p


def _bfv_plain_forms(o, g, rng, shapes, tag, ops=PLAIN_OPS, strides=(False, True), places=(False, True)):
    """every op x {broadcast, one plaintext per ciphertext} x {out of place, out == ct} on (count, size) ciphertexts"""
    n, L = o.n, len(o.primes) - 1
    for batch, size in shapes:
        ct = _cts(rng, o, L, batch, size)
        pl = _bfv_plains(rng, o.t, n, max(batch, 2))
        for op in ops:
            for per_ct in strides:
                want = np.stack([getattr(o, op)(ct[i], pl[i if per_ct else 0]) for i in range(batch)])
                for in_place in places:
                    got = _plain_call(g, op, ct, pl[:batch] if per_ct else pl[0], n if per_ct else 0, in_place)
                    _same("%s %s count=%d size=%d stride=%s %s" % (tag, op, batch, size, "N" if per_ct else "0",
                                                                 "out==ct" if in_place else "out of place"), got, want)


def _bfv_plain_ctx(oracle_mod, capi, n, bits):
    primes = oracle_mod.default_bfv_primes(n) if bits is None else oracle_mod.create_primes(n, bits)
    t = oracle_mod.plain_modulus_batching(n, 20)
    o = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)  # no keys: the plain operations need none
    g = capi.Context(capi.BFV, n, primes, t)
    assert g.primes == o.primes and g.t == o.t == capi.plain_modulus_batching(n, 20)
    return o, g


# (ring, chain, switches, fused?): which multiply_plain sequence the context takes, and the facts that select it
BFV_PLAIN_CONTEXTS = {
    "fused_n1024_two_40bit_primes": (1024, [40, 40, 41], {}, True),
    "fused_bfv_default_4096": (4096, None, {}, True),
    "fused_bfv_default_8192": (8192, None, {}, True),
    "unfused_n4096_no_fused": (4096, None, {"ABC_HIP_NO_FUSED": "1"}, False),
    "unfused_n4096_no_fp64": (4096, None, {"ABC_HIP_NO_FP64": "1"}, False),
    "unfused_n8192_55bit_primes": (8192, [55, 55, 56], {}, False),
}


@pytest.mark.parametrize("name", list(BFV_PLAIN_CONTEXTS))
def test_bfv_plain_ops_stride_size_alias(name, oracle_mod, capi, monkeypatch):
    n, bits, env, fused = BFV_PLAIN_CONTEXTS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the context is created
    o, g = _bfv_plain_ctx(oracle_mod, capi, n, bits)
    L = len(o.primes) - 1
    # the fused kernel wants 2^10 <= N < 2^14 (at 2^14: the batch rule, tested below), data primes below 2^50, no switch
    assert fused == (not env and max(int(p).bit_length() for p in o.primes[:L]) <= 50 and 10 <= g.logn < 14)
    rng = np.random.default_rng(n + len(name))
    _bfv_plain_forms(o, g, rng, [(3, 2), (3, 3)], name)
    g.close()


def test_bfv_multiply_plain_switch_at_n16384(oracle_mod, capi):
    """BFVDefault(16384): count * size * L <= 48 keeps the spread-out transforms (k_plain_lift, k_mul_plain_ntt), above 48 the fused
    kernel runs.  Both sides of the boundary, reached once by count at size 2 and once at size 3; both equal the oracle."""
    o, g = _bfv_plain_ctx(oracle_mod, capi, 16384, None)
    L = g.L
    assert max(int(p).bit_length() for p in o.primes[:L]) <= 50
    shapes = []
    for size in (2, 3):
        assert 48 % (size * L) == 0, "BFVDefault(16384) changed: derive the pairs again"
        below = 48 // (size * L)
        assert below * size * L == 48 and (below + 1) * size * L > 48
        shapes += [(below, size), (below + 1, size)]
    if L == 8:
        assert shapes == [(3, 2), (4, 2), (2, 3), (3, 3)]
    rng = np.random.default_rng(16384)
    _bfv_plain_forms(o, g, rng, shapes, "bfv16384 switch", ops=("multiply_plain",))
    # add_plain / sub_plain have one kernel: the largest shape, every form
    _bfv_plain_forms(o, g, rng, [shapes[-1]], "bfv16384", ops=("add_plain", "sub_plain"))
    g.close()


def test_bfv_plain_ops_n32768_per_ciphertext_plaintexts(oracle_mod, capi):
    """N = 2^15 has the unfused sequence only: three lifted plaintexts stay in the workspace while the strided transforms of the
    ciphertexts run; one multiply_plain and one add_plain of three ciphertexts with a plaintext each"""
    o, g = _bfv_plain_ctx(oracle_mod, capi, 32768, [45, 45, 46])
    rng = np.random.default_rng(32768)
    _bfv_plain_forms(o, g, rng, [(3, 2)], "bfv32768", ops=("multiply_plain", "add_plain"), strides=(True,), places=(False,))
    g.close()


# ---------------- B. plain operations, CKKS ----------------
def _ckks_plains(rng, o, nl, rows):
    return random_ct(rng, [int(p) for p in o.primes], nl, o.n, rows, size=1)[:, 0]  # [rows][nl][N], the ciphertexts' edge words


def _ckks_plain_forms(o, g, seed, tag):
    n, L = o.n, len(o.primes) - 1
    rng = np.random.default_rng(seed)
    for nl in sorted({1, 2, L}):
        for size in (2, 3):
            for batch in (1, 3):
                ct = _cts(rng, o, nl, batch, size)
                pl = _ckks_plains(rng, o, nl, max(batch, 2))
                for op in PLAIN_OPS:
                    for per_ct in (False, True):
                        want = np.stack([getattr(o, op)(ct[i], pl[i if per_ct else 0]) for i in range(batch)])
                        for in_place in (False, True):
                            got = _plain_call(g, op, ct, pl[:batch] if per_ct else pl[0], nl * n if per_ct else 0, in_place)
                            _same("%s %s nl=%d size=%d count=%d stride=%s %s" % (
                                tag, op, nl, size, batch, "nl*N" if per_ct else "0", "out==ct" if in_place else "out of place"), got, want)


def test_ckks_plain_ops_stride_size_level_alias(ckks12):
    o, g = ckks12
    _ckks_plain_forms(o, g, 50, "ckks [50,40,40,50]")


def test_ckks_plain_ops_on_a_60_bit_prime(ckks12_wide):
    o, g = ckks12_wide
    assert int(o.primes[0]).bit_length() == 60
    _ckks_plain_forms(o, g, 60, "ckks [60,40,60]")


@pytest.mark.parametrize("which", ["ckks12", "ckks12_wide"])
def test_ckks_plaintexts_laid_out_for_the_top_level(which, request):
    """plaintexts [count][L][N] (stride L * N) applied to ciphertexts at nl < L: row i starts at i * L * N and its first nl limbs are
    read (abc_hip.h: a CKKS stride may exceed nl * N)"""
    o, g = request.getfixturevalue(which)
    n, L = o.n, len(o.primes) - 1
    rng = np.random.default_rng(L)
    pl = _ckks_plains(rng, o, L, 3)
    for nl in range(1, L):
        for size in (2, 3):
            ct = _cts(rng, o, nl, 3, size)
            for op in PLAIN_OPS:
                want = np.stack([getattr(o, op)(ct[i], np.ascontiguousarray(pl[i, :nl])) for i in range(3)])
                for in_place in (False, True):
                    got = _plain_call(g, op, ct, pl, L * n, in_place)
                    _same("%s %s nl=%d of L=%d size=%d stride=L*N in_place=%d" % (which, op, nl, L, size, in_place), got, want)


# ---------------- the plain_stride contract ----------------
def _refused(g, capi, op, ct, plain, stride, text):
    """the call fails with its message, writes nothing, and the context goes on working"""
    ct = np.ascontiguousarray(ct)
    cb, pb = g.upload(ct), g.upload(plain)
    out = g.upload(np.full(ct.shape, 7, dtype=np.uint64))
    with pytest.raises(capi.AbcHipError, match=text):
        g.op(op, cb.ptr, pb.ptr, C.c_size_t(stride), out.ptr, ct.shape[1], ct.shape[2], C.c_size_t(ct.shape[0]))
    assert (g.download(out, ct.shape) == 7).all() and np.array_equal(g.download(cb, ct.shape), ct)
    for b in (cb, pb, out):
        b.free()


def test_bfv_plain_stride_other_than_0_or_n_is_refused(bfv12, capi):
    o, g = bfv12
    n, L = o.n, len(o.primes) - 1
    rng = np.random.default_rng(1)
    ct = _cts(rng, o, L, 2)
    pl = _bfv_plains(rng, o.t, n, 2)
    for op in PLAIN_OPS:
        for stride in (1, n - 1, n + 1, 2 * n, L * n):
            _refused(g, capi, op, ct, pl, stride, op + ": plain_stride must be 0 or N")
        want = np.stack([getattr(o, op)(ct[i], pl[i]) for i in range(2)])
        _same(op + " after a refusal", _plain_call(g, op, ct, pl, n, False), want)


def test_ckks_plain_stride_below_a_row_is_refused(ckks12, capi):
    o, g = ckks12
    n, L = o.n, len(o.primes) - 1
    rng = np.random.default_rng(2)
    for nl in (1, L):
        ct = _cts(rng, o, nl, 2)
        pl = _ckks_plains(rng, o, nl, 2)
        for op in PLAIN_OPS:
            for stride in (1, n - 1, nl * n - 1):
                _refused(g, capi, op, ct, pl, stride, op + ": plain_stride must be 0 or at least nl \\* N")
            want = np.stack([getattr(o, op)(ct[i], pl[i]) for i in range(2)])
            _same("%s nl=%d after a refusal" % (op, nl), _plain_call(g, op, ct, pl, nl * n, False), want)


# ---------------- C. size 3 and aliasing: add, sub, negate ----------------
def _addsub_forms(o, g, nl, seed, tag):
    rng = np.random.default_rng(seed)
    for size in (2, 3):
        a, b = _cts(rng, o, nl, 3, size), _cts(rng, o, nl, 3, size)
        for op in ("add", "sub"):
            want = np.stack([getattr(o, op)(x, y) for x, y in zip(a, b)])
            for alias in (None, "a", "b"):
                _same("%s %s size=%d nl=%d out==%s" % (tag, op, size, nl, alias), _binop_call(g, op, a, b, alias), want)
        same = np.stack([o.sub(x, x) for x in a])
        assert not same.any()
        _same("%s a - a size=%d nl=%d" % (tag, size, nl), _binop_call(g, "sub", a, None, "same"), same)
        want = np.stack([o.negate(x) for x in a])
        assert (want[a == 0] == 0).all() and (a == 0).any()  # negate of 0 stays 0, and the batch has such words
        for alias in (None, "a"):
            _same("%s negate size=%d nl=%d out==%s" % (tag, size, nl, alias), _binop_call(g, "negate", a, None, alias), want)


def test_bfv_add_sub_negate_size3_and_aliased(bfv12):
    o, g = bfv12
    _addsub_forms(o, g, len(o.primes) - 1, 31, "bfv4096")


@pytest.mark.parametrize("level", ["bottom", "top"])
def test_ckks_add_sub_negate_size3_and_aliased(level, ckks12):
    o, g = ckks12
    _addsub_forms(o, g, 1 if level == "bottom" else len(o.primes) - 1, 32, "ckks4096")


# ---------------- C. size 3: rescale and mod_switch on every rescale route of a small ring ----------------
RESCALE_CASES = {
    # name: (N, chain, switches, {nl: route})
    "fp_n4096": (4096, [50, 40, 40, 50], {}, {3: "fp", 2: "fp"}),
    "mixed_n4096_60bit": (4096, [60, 40, 40, 60], {}, {3: "mixed fpmask=0x6", 2: "mixed fpmask=0x2"}),
    "generic_n4096_no_fused": (4096, [50, 40, 40, 50], {"ABC_HIP_NO_FUSED": "1"}, {3: "generic", 2: "generic"}),
    "fp_n16384": (16384, [50, 40, 40, 40, 50], {}, {4: "fp"}),
}


@pytest.mark.parametrize("name", list(RESCALE_CASES))
def test_rescale_and_mod_switch_size3_batch(name, oracle_mod, capi, monkeypatch):
    n, bits, env, routes = RESCALE_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    primes = oracle_mod.create_primes(n, bits)
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)  # no keys needed
    g = capi.Context(capi.CKKS, n, primes)
    rng = np.random.default_rng(n + len(name))
    for nl, route in routes.items():
        assert g.route("rescale", nl, 3) == route, (name, nl)
        for size in (3, 2):
            ct = _cts(rng, o, nl, 3, size)
            _same("%s rescale nl=%d size=%d" % (name, nl, size), g.rescale(ct), np.stack([o.rescale(x) for x in ct]))
            _same("%s mod_switch nl=%d size=%d" % (name, nl, size), g.mod_switch(ct), np.stack([o.mod_switch(x) for x in ct]))
    g.close()


# ---------------- C. decrypt: size 3, batches of distinct rows ----------------
def test_ckks_decrypt_size3_every_level(ckks12):
    o, g = ckks12
    rng = np.random.default_rng(41)
    for nl in sorted({1, 2, len(o.primes) - 1}):
        for size in (3, 2):
            ct = _cts(rng, o, nl, 3, size)
            _same("ckks decrypt size=%d nl=%d" % (size, nl), g.decrypt(ct), np.stack([o.decrypt(x) for x in ct]))


def _bfv_decrypt(oracle_mod, capi, n, bits, sizes, seed):
    primes = oracle_mod.default_bfv_primes(n) if bits is None else oracle_mod.create_primes(n, bits)
    t = oracle_mod.plain_modulus_batching(n, 20)
    o = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)
    o.keygen(seed, elts=[])  # decryption needs the secret key only
    g = capi.Context(capi.BFV, n, primes, t)
    g.load_keys(sk=o.secret_key())
    rng = np.random.default_rng(seed)
    for size in sizes:
        ct = _cts(rng, o, len(primes) - 1, 3, size)
        _same("bfv decrypt N=%d size=%d" % (n, size), g.decrypt(ct), np.stack([o.decrypt(x) for x in ct]))
    g.close()


@pytest.mark.parametrize("n", [8192, 16384])
def test_bfv_decrypt_size3_batch(n, oracle_mod, capi):
    _bfv_decrypt(oracle_mod, capi, n, None, (3,), 0xABC00040 + n)


def test_bfv_decrypt_n32768_size2_and_size3(oracle_mod, capi):
    _bfv_decrypt(oracle_mod, capi, 32768, [45, 45, 46], (2, 3), 0xABC00045)


# ---------------- D. Galois ----------------
GALOIS_CONTEXTS = {
    # fixture, switches, route of one Galois element at the top level
    "bfv4096": ("bfv12", {}, "permute lds_fp"),
    "ckks16384_fold": ("ckks14", {}, "fold " + _SPLIT14),
    "ckks16384_permute": ("ckks14", {"ABC_HIP_NO_GALOIS_FUSION": "1"}, "permute " + _SPLIT14),
    "ckks4096": ("ckks12", {}, "permute lds_fp"),
}


class _Switched:
    """switches on a shared context: set, re-read, and put back at the end whatever happens"""

    def __init__(self, g, env, monkeypatch):
        self.g, self.env, self.mp = g, env, monkeypatch

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, v)
        self.g.reload_env()

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k)
        self.g.reload_env()


@pytest.mark.parametrize("name", list(GALOIS_CONTEXTS))
def test_apply_galois_direct(name, request, capi, monkeypatch):
    """abc_hip_apply_galois against Oracle.apply_galois: 3 (one slot to the left), 2N - 1 (BFV: column swap, CKKS: conjugation) and an
    element from the middle of the key list; in place it is refused and changes nothing"""
    fixture, env, route = GALOIS_CONTEXTS[name]
    o, g = request.getfixturevalue(fixture)
    n, L = o.n, len(o.primes) - 1
    elts = o.galois_elts()
    assert sorted(g.galois_elts()) == sorted(elts) and 2 * n - 1 in elts and 3 in elts
    rng = np.random.default_rng(len(name))
    with _Switched(g, env, monkeypatch):
        assert g.route("rotate", L, 2) == route
        ct = _cts(rng, o, L, 2)
        for elt in (3, 2 * n - 1, elts[len(elts) // 2]):
            _same("%s apply_galois %d" % (name, elt), g.apply_galois(ct, elt), np.stack([o.apply_galois(x, elt) for x in ct]))
        if o.scheme == 2:  # a lower level: the key's limbs are no longer contiguous with the special prime
            low = _cts(rng, o, 2, 2)
            assert g.route("rotate", 2, 2) == route
            _same("%s apply_galois 2N-1 nl=2" % name, g.apply_galois(low, 2 * n - 1), np.stack([o.apply_galois(x, 2 * n - 1) for x in low]))
        cb = g.upload(ct)
        with pytest.raises(capi.AbcHipError, match="apply_galois: in-place not supported"):
            g.op("apply_galois", cb.ptr, cb.ptr, L, C.c_uint32(3), C.c_size_t(2))
        _same(name + " refused in-place apply_galois left its operand alone", g.download(cb, ct.shape), ct)
        cb.free()
        _same(name + " apply_galois after the refusal", g.apply_galois(ct[0], 3), o.apply_galois(ct[0], 3))


@pytest.mark.parametrize("name", list(GALOIS_CONTEXTS))
def test_rotate_in_place(name, request, monkeypatch):
    """abc_hip_rotate with d_out == d_in: a step with a key (one hop through an arena, then a copy), a step of two non-adjacent-form
    terms and one of three (ping-pong through arenas 1 and 2, the last hop lands on the operand), and step 0.  This pins the
    result of every form, not which hop sequence produced it: without rotate()'s `out == cur` case the single hop would call
    apply_galois aliased, which then permutes into arena 0 first (route_rotate, in_place) and returns the same words -- a library
    built that way passes here too."""
    fixture, env, route = GALOIS_CONTEXTS[name]
    o, g = request.getfixturevalue(fixture)
    L = len(o.primes) - 1
    have = set(g.galois_elts())
    steps = {1: 1, 7: 2, 11: 3, -21: 3}  # step: terms
    for step, terms in steps.items():
        assert len(_naf(step)) == terms and sum(_naf(step)) == step
        assert (g.elt_from_step(step) in have) == (terms == 1), step
        assert all(g.elt_from_step(s) in have for s in _naf(step))
    rng = np.random.default_rng(len(name) + 100)
    with _Switched(g, env, monkeypatch):
        assert g.route("rotate", L, 2) == route
        ct = _cts(rng, o, L, 2)
        for step in list(steps) + [0]:
            want = np.stack([o.rotate(x, step) for x in ct])
            apart = _rotate_call(g, ct, step, False)
            _same("%s rotate %d out of place" % (name, step), apart, want)
            _same("%s rotate %d out == in" % (name, step), _rotate_call(g, ct, step, True), apart)
        assert np.array_equal(_rotate_call(g, ct, 0, True), ct)


# ---------------- E. BatchEncoder on every ring ----------------
@pytest.mark.parametrize("logn", range(10, 17))
def test_batch_encode_decode_every_ring(logn, oracle_mod, capi):
    n = 1 << logn
    primes = oracle_mod.create_primes(n, [40, 41])
    t = oracle_mod.plain_modulus_batching(n, 20)
    o = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)
    g = capi.Context(capi.BFV, n, primes, t)
    assert g.t == t and t % (2 * n) == 1
    rng = np.random.default_rng(logn)
    half = (t - 1) // 2
    vals = rng.integers(-half, half + 1, size=(3, n), dtype=np.int64)
    planted = np.array([0, 1, -1, half, -half], dtype=np.int64)
    for r in range(3):  # first, middle and last slot of each half (row) of the batching matrix
        for k, slot in enumerate((0, n // 4, n // 2 - 1, n // 2, 3 * n // 4, n - 1)):
            vals[r, slot] = planted[(k + r) % 5]
    assert len({v.tobytes() for v in vals}) == 3
    _same("batch_encode N=2^%d" % logn, g.batch_encode(vals), np.stack([o.encode(v) for v in vals]))
    words = rng.integers(0, t, size=(3, n), dtype=np.uint64)
    pb = g.upload(words)
    out = g.alloc(words.nbytes)
    g.op("batch_decode", pb.ptr, out.ptr, C.c_size_t(3))
    got = g.download(out, words.shape, np.int64)
    want = np.stack([o.decode(w) for w in words])
    assert (want < 0).any() and (want > 0).any()
    _same("batch_decode N=2^%d" % logn, got, want)
    _same("batch_decode N=2^%d left its input alone" % logn, g.download(pb, words.shape), words)
    pb.free(); out.free()
    g.close()
