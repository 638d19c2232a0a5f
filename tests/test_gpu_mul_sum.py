"""Sums of ciphertext products with one relinearisation on the device: abc_hip_multiply_sum (the K-term CKKS tensor-sum kernel, or
product by product on the per-term route) and abc_hip_mul_sum_relin (that sum in an arena, then the key switch of the level).
Every comparison is word for word against tests/mul_sum_spec.py -- the CPU oracle's multiply per term, its add at size 3, and ONE
relinearize -- never against a sum of relinearised products, which is a different ciphertext (tests/test_mul_sum_spec.py).

The kernel's decision points, all on both sides in TERMS below: eight pointer pairs per launch (K = 8 | 9, 16 | 17, 33 = four
launches and a tail of one), the fp64 accumulators re-centred after terms 3 and 6 of a launch (K = 3 | 4, 5 | 7, and 11 | 12 = 8 + 3 | 4 in
a second launch; K = 6 | 7 too), the unrolled loop's tail at every K that is no multiple of 8, and the integer accumulator, which reduces
once per launch: at most 17 products of 60-bit residues, of the 256 that 128 bits hold (test_integer_accumulator_overflow_point
runs the K at which a call WITHOUT the launch boundary would overflow)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mul_sum_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TERMS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33]
MORE_TERMS = [6, 11, 12]  # the second re-centring of a launch, and both of a second launch
FP_CHAIN, MIXED_CHAIN, WIDE_CHAIN = [50, 40, 40, 50], [60, 40, 40, 60], [60, 60, 60]
SPAN = 512  # coefficients of one limb a workgroup of the tensor-sum kernel owns


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


@contextlib.contextmanager
def _env(g, settings):
    """the ABC_HIP_* switches are read by reload_env; restored, and read again, on the way out"""
    old = {k: os.environ.get(k) for k in settings}
    os.environ.update(settings)
    g.reload_env()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        g.reload_env()


def _random_cts(rng, primes, nl, shape, n):
    """random canonical residues, [*shape][2][nl][N]"""
    return np.stack([rng.integers(0, q, size=tuple(shape) + (2, n), dtype=np.uint64) for q in primes[:nl]], axis=len(shape) + 1)


def _call(g, name, a_ptrs, b_ptrs, out_ptr, nl, count):
    g.op(name, g.term_pointers(a_ptrs), g.term_pointers(b_ptrs), len(a_ptrs), out_ptr, nl, C.c_size_t(count))


class Pool:
    """host arrays [count][2][nl][N] uploaded once; a call names its terms by index, so sharing a pointer is sharing an index"""

    def __init__(self, g, arrays):
        self.g, self.arrays = g, [np.ascontiguousarray(a) for a in arrays]
        self.bufs = [g.upload(a) for a in self.arrays]
        self.count, _, self.nl, self.n = self.arrays[0].shape

    def run(self, name, ia, ib, size):
        shp = (self.count, size, self.nl, self.n)
        out = self.g.upload(np.full(shp, SENTINEL, dtype=np.uint64))
        try:
            _call(self.g, name, [self.bufs[i].ptr for i in ia], [self.bufs[i].ptr for i in ib], out.ptr, self.nl, self.count)
            return self.g.download(out, shp)
        finally:
            out.free()

    def unchanged(self):
        for a, b in zip(self.arrays, self.bufs):
            _same("an operand is left alone", self.g.download(b, a.shape), a)

    def free(self):
        for b in self.bufs:
            b.free()


def _prefix_sums(o, a, b, ks):
    """{K: [count][3][nl][N]} for every K in ks: the oracle's product per term and ciphertext, added up once in term order"""
    count = a.shape[1]
    want, acc = {}, [None] * count
    for k in range(max(ks)):
        for r in range(count):
            p = o.multiply(a[k, r], b[k, r])
            acc[r] = p if acc[r] is None else o.add(acc[r], p)
        if k + 1 in ks:
            want[k + 1] = np.stack(acc)
    return want


def _data(kind, rng, primes, nl, terms, count, n):
    """(a, b) [terms][count][2][nl][N]"""
    q = np.array(primes[:nl], dtype=np.uint64)[:, None]
    if kind == "random":
        return _random_cts(rng, primes, nl, (terms, count), n), _random_cts(rng, primes, nl, (terms, count), n)
    a = np.empty((terms, count, 2, nl, n), dtype=np.uint64)
    if kind == "max":  # (q - 1)^2 in every product of every term: the largest sums there are
        a[:] = q - 1
        return a, a.copy()
    # 0 / 1 / q-1 by coefficient index, shifted per term, q-1 in both factors at the ends of the ring and of a workgroup's span
    idx = np.arange(n)
    vals = np.stack([np.zeros_like(q), np.ones_like(q), q - 1])  # [3][nl][1]
    b = np.empty_like(a)
    for k in range(terms):
        a[k] = vals[(idx + k) % 3, :, 0].T
        b[k] = vals[(2 * idx + k) % 3, :, 0].T
    for s in (0, 1, SPAN - 1, SPAN, n - SPAN - 1, n - SPAN, n - 2, n - 1):
        a[..., s] = q[:, 0] - 1
        b[..., s] = q[:, 0] - 1
    return a, b


class KernelRig:
    """one oracle and one device context on a CKKS chain at N = 2^10, count 3; the references of every K for the three kinds of
    data, computed once per level and left unchanged"""

    def __init__(self, om, capi, bits, n=1024):
        primes = om.create_primes(n, bits)
        self.o = om.Oracle(om.CKKS, n, primes)
        self.g = capi.Context(capi.CKKS, n, self.o.primes)
        self.n, self.primes, self.bits = n, list(primes), bits
        self._cases = {}

    def case(self, kind, nl, count=3):
        k = (kind, nl, count)
        if k not in self._cases:
            ks = set(TERMS + MORE_TERMS)
            rng = np.random.default_rng(sum(self.bits) + nl)
            a, b = _data(kind, rng, self.primes, nl, max(ks), count, self.n)
            want = _prefix_sums(self.o, a, b, ks)
            for w in want.values():
                w.setflags(write=False)
            self._cases[k] = (a, b, want)
        return self._cases[k]

    def check(self, tag, nl, kinds=("random", "max", "pattern"), ks=TERMS + MORE_TERMS):
        for kind in kinds:
            a, b, want = self.case(kind, nl)
            pool = Pool(self.g, list(a) + list(b))
            try:
                for K in ks:
                    got = pool.run("multiply_sum", range(K), range(len(a), len(a) + K), 3)
                    _same("%s nl=%d %s K=%d" % (tag, nl, kind, K), got, want[K])
                pool.unchanged()
            finally:
                pool.free()

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def kernel_rigs(oracle_mod, capi):
    made = {}

    def get(bits):
        if tuple(bits) not in made:
            made[tuple(bits)] = KernelRig(oracle_mod, capi, bits)
        return made[tuple(bits)]

    yield get
    for r in made.values():
        r.close()


# ---- the kernel alone ----
@pytest.mark.parametrize("nl", [3, 1])
def test_kernel_fp_chain(kernel_rigs, nl):
    r = kernel_rigs(FP_CHAIN)
    assert r.g.route("mul_sum_relin", nl, 3).endswith(" tensor=sum")
    r.check("fp", nl)


def test_kernel_mixed_chain(kernel_rigs):
    """limb 0 on the integers, limbs 1 and 2 in fp64, one launch"""
    kernel_rigs(MIXED_CHAIN).check("mixed", 3)


def test_kernel_mixed_chain_all_integer(kernel_rigs):
    r = kernel_rigs(MIXED_CHAIN)
    with _env(r.g, {"ABC_HIP_NO_MIXED": "1"}):
        r.check("no_mixed", 3)


def test_kernel_no_fp64(kernel_rigs, oracle_mod, capi, monkeypatch):
    """ABC_HIP_NO_FP64 is read when the context is created: the same chain, references shared, integers throughout"""
    r = kernel_rigs(MIXED_CHAIN)
    monkeypatch.setenv("ABC_HIP_NO_FP64", "1")
    g = capi.Context(capi.CKKS, r.n, r.o.primes)
    monkeypatch.delenv("ABC_HIP_NO_FP64")
    keep, r.g = r.g, g
    try:
        r.check("no_fp64", 3)
    finally:
        r.g = keep
        g.close()


def test_kernel_widest_primes(kernel_rigs):
    """a chain of 60-bit primes, the widest abc_hip_ctx_create accepts"""
    r = kernel_rigs(WIDE_CHAIN)
    assert all(p.bit_length() == 60 for p in r.primes)
    r.check("wide", 2)


def test_integer_accumulator_overflow_point(kernel_rigs):
    """2K products of (q-1)^2 pass 2^128 from K on: derived from the prime, 129 for 60 bits.  Every residue q - 1."""
    r = kernel_rigs(WIDE_CHAIN)
    q = max(r.primes[:2])
    K = next(k for k in range(1, 10 ** 6) if 2 * k * (q - 1) ** 2 >= 1 << 128)
    assert K == 129
    a = np.empty((1, 2, 2, r.n), dtype=np.uint64)
    a[:] = (np.array(r.primes[:2], dtype=np.uint64) - 1)[:, None]
    one = r.o.multiply(a[0], a[0])
    want = one
    for _ in range(K - 1):
        want = r.o.add(want, one)
    pool = Pool(r.g, [a])
    try:
        _same("K = %d terms of (q-1) (x) (q-1)" % K, pool.run("multiply_sum", [0] * K, [0] * K, 3)[0], want)
    finally:
        pool.free()


# ---- other shapes ----
@pytest.mark.parametrize("n,bits,nl,count", [(16384, [50, 40, 40, 40, 50], 4, 2), (32768, FP_CHAIN, 3, 2), (65536, [50, 40, 50], 2, 1)],
                         ids=["2^14", "2^15", "2^16"])
def test_kernel_other_rings(oracle_mod, capi, n, bits, nl, count):
    om = oracle_mod
    o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
    g = capi.Context(capi.CKKS, n, o.primes)
    try:
        rng = np.random.default_rng(n)
        a, b = _data("random", rng, o.primes, nl, 3, count, n)
        want = _prefix_sums(o, a, b, {3})[3]
        _same("N=%d nl=%d" % (n, nl), g.multiply_sum(list(a), list(b)), want)
    finally:
        g.close()


# ---- operand forms ----
def test_operand_forms(kernel_rigs):
    r = kernel_rigs(FP_CHAIN)
    g, o, n, nl, count = r.g, r.o, r.n, 3, 3
    a, b, _ = r.case("random", nl)
    x, y, z = a[0], a[1], b[0]
    ref = lambda as_, bs: np.stack([spec.multiply_sum(o, [t[i] for t in as_], [t[i] for t in bs]) for i in range(count)])  # noqa: E731
    pool = Pool(g, [x, y, z])
    try:
        _same("squares: a_k is b_k", pool.run("multiply_sum", [0, 1, 2], [0, 1, 2], 3), ref([x, y, z], [x, y, z]))
        _same("one pointer in two terms", pool.run("multiply_sum", [0, 0, 1], [1, 2, 0], 3), ref([x, x, y], [y, z, x]))
        pool.unchanged()
    finally:
        pool.free()
    # term buffers that are sub-ranges of one allocation: four ciphertext batches back to back, terms (0, 1) and (2, 3)
    block = np.ascontiguousarray(np.stack([x, y, z, a[2]]))
    d_block, d_out = g.upload(block), g.alloc(count * 3 * nl * n * 8)
    try:
        step = x.nbytes
        ptr = lambda i: C.c_void_p(d_block.ptr.value + i * step)  # noqa: E731
        _call(g, "multiply_sum", [ptr(0), ptr(2)], [ptr(1), ptr(3)], d_out.ptr, nl, count)
        _same("sub-ranges of one allocation", g.download(d_out, (count, 3, nl, n)), ref([x, z], [y, a[2]]))
    finally:
        d_block.free()
        d_out.free()


# ---- mul_sum_relin against the spec, one context per key-switch route ----
class RelinRig:
    def __init__(self, om, capi, scheme, n, bits=None, env=None, monkeypatch=None):
        if scheme == "ckks":
            self.o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
        else:
            self.o = om.Oracle.bfv_default(n)
        self.o.keygen(0x5A1, elts=[])  # relinearisation key only
        self.g = capi.Context(capi.CKKS if scheme == "ckks" else capi.BFV, n, self.o.primes, self.o.t)
        self.g.load_keys(sk=self.o.secret_key(), pk=self.o.public_key(), relin=self.o.relin_key())
        self.scheme, self.n, self.L = scheme, n, self.o.L
        self._terms = {}

    def terms(self, nl, count, how_many):
        """(a, b) [how_many][count][2][nl][N]: random residues for CKKS, fresh encryptions for BFV (its multiply rounds)"""
        k = (nl, count, how_many)
        if k not in self._terms:
            o, rng = self.o, np.random.default_rng(self.n + nl)
            if self.scheme == "ckks":
                t = _random_cts(rng, o.primes, nl, (2, how_many, count), self.n)
            else:
                t = np.stack([o.encrypt(o.encode(rng.integers(0, 64, self.n)), 100 + i) for i in range(2 * how_many * count)])
                t = t.reshape((2, how_many, count) + t.shape[1:])
            t.setflags(write=False)
            self._terms[k] = t
        return self._terms[k]

    def want(self, a, b):
        count = a.shape[1]
        return np.stack([spec.mul_sum_relin(self.o, list(a[:, i]), list(b[:, i])) for i in range(count)])

    def check(self, tag, nl, count, ks=(2, 5)):
        a, b = self.terms(nl, count, max(ks))
        for K in ks:
            got = self.g.mul_sum_relin(list(a[:K]), list(b[:K]))
            _same("%s nl=%d K=%d" % (tag, nl, K), got, self.want(a[:K], b[:K]))

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def relin_rigs(oracle_mod, capi):
    made = {}

    def get(scheme, n, bits=None):
        k = (scheme, n, tuple(bits or ()))
        if k not in made:
            made[k] = RelinRig(oracle_mod, capi, scheme, n, bits)
        return made[k]

    yield get
    for r in made.values():
        r.close()


HEAD14 = [50, 40, 40, 40, 50]


@pytest.mark.parametrize("nl", [4, 2, 1])
def test_relin_split14(relin_rigs, nl):
    r = relin_rigs("ckks", 16384, HEAD14)
    assert r.g.route("mul_sum_relin", nl, 2) == "split14 front=lean pack=1 main=split4 tensor=sum"
    r.check("split14", nl, 2)


@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_SPLIT": "1"}, "lds_fp tensor=sum"),
    ({"ABC_HIP_NO_FUSED": "1"}, "generic front=plain tensor=sum"),
    ({"ABC_HIP_NO_TENSOR_SUM": "1"}, "split14 front=lean pack=1 main=split4 tensor=per_term"),
], ids=["no_split", "no_fused", "no_tensor_sum"])
def test_relin_split14_switches(relin_rigs, env, route):
    r = relin_rigs("ckks", 16384, HEAD14)
    with _env(r.g, env):
        assert r.g.route("mul_sum_relin", 4, 2) == route
        r.check(" ".join(env), 4, 2)
    assert r.g.route("mul_sum_relin", 4, 2) == "split14 front=lean pack=1 main=split4 tensor=sum"


def test_relin_isplit(relin_rigs):
    r = relin_rigs("ckks", 16384, [60, 40, 40, 40, 60])
    assert r.g.route("mul_sum_relin", 4, 2) == "isplit14 guard=1 fpmask=0xe tensor=sum"
    r.check("isplit", 4, 2)


def test_relin_gsplit15(relin_rigs):
    r = relin_rigs("ckks", 32768, FP_CHAIN)
    assert r.g.route("mul_sum_relin", 3, 2) == "gsplit15 tensor=sum"
    r.check("gsplit15", 3, 2)


@pytest.mark.parametrize("n", [4096, 1024])
def test_relin_lds_fp(relin_rigs, n):
    r = relin_rigs("ckks", n, FP_CHAIN)
    assert r.g.route("mul_sum_relin", 3, 3) == "lds_fp tensor=sum"
    r.check("lds_fp", 3, 3)
    with _env(r.g, {"ABC_HIP_NO_TENSOR_SUM": "1"}):
        assert r.g.route("mul_sum_relin", 3, 3) == "lds_fp tensor=per_term"
        r.check("lds_fp per_term", 3, 3)


@pytest.mark.parametrize("n,count,ks", [(4096, 2, (2, 5)), (8192, 2, (2, 5)), (16384, 1, (2,))], ids=["4096", "8192", "16384"])
def test_relin_bfv_per_term(relin_rigs, n, count, ks):
    r = relin_rigs("bfv", n)
    assert r.g.route("mul_sum_relin", r.L, count) == r.g.route("relinearize", r.L, count) + " tensor=per_term"
    r.check("bfv", r.L, count, ks)
    a, b = r.terms(r.L, count, max(ks))
    want3 = np.stack([spec.multiply_sum(r.o, list(a[:2, i]), list(b[:2, i])) for i in range(count)])
    _same("bfv multiply_sum", r.g.multiply_sum(list(a[:2]), list(b[:2])), want3)


# ---- groups of ciphertexts ----
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_groups_and_ragged_last_group(relin_rigs, lanes):
    """ABC_HIP_CHUNK=2: groups of chunk * lanes ciphertexts -- two up to a batch of eight, which runs on one lane whatever
    ABC_HIP_LANES says, four at eleven on two lanes -- the last one ragged; d_out is the first term's left factor, and in a second call
    the last term's right factor"""
    r = relin_rigs("ckks", 4096, FP_CHAIN)
    g, n, nl, K = r.g, r.n, 3, 3
    with _env(g, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": lanes}):
        for count in (5, 7, 11):
            a, b = r.terms(nl, count, K)
            want = r.want(a, b)
            assert g.route("mul_sum_relin", nl, count) == "lds_fp tensor=sum"
            _same("count %d out of place" % count, g.mul_sum_relin(list(a), list(b)), want)
            for alias in ("a0", "bK"):
                pool = Pool(g, list(a) + list(b))
                try:
                    out = pool.bufs[0] if alias == "a0" else pool.bufs[2 * K - 1]
                    _call(g, "mul_sum_relin", [x.ptr for x in pool.bufs[:K]], [x.ptr for x in pool.bufs[K:]], out.ptr, nl, count)
                    _same("count %d d_out is %s" % (count, alias), g.download(out, (count, 2, nl, n)), want)
                finally:
                    pool.free()


# ---- equalities ----
def test_one_term_none_and_no_ciphertexts(relin_rigs):
    for r, nl in ((relin_rigs("ckks", 16384, HEAD14), 4), (relin_rigs("bfv", 4096), None)):
        g, n = r.g, r.n
        nl = nl or r.L
        a, b = r.terms(nl, 2, 5)
        _same("K = 1 is mul_relin", g.mul_sum_relin([a[0]], [b[0]]), g.mul_relin(a[0], b[0]))
        _same("K = 1 is multiply", g.multiply_sum([a[0]], [b[0]]), g.multiply(a[0], b[0]))
        for name, size in (("multiply_sum", 3), ("mul_sum_relin", 2)):
            shp = (2, size, nl, n)
            d_out = g.upload(np.full(shp, SENTINEL, dtype=np.uint64))
            _call(g, name, [], [], d_out.ptr, nl, 2)
            assert not g.download(d_out, shp).any(), name + ": an empty sum is zero"
            g.op("memcpy_h2d", d_out.ptr, np.full(shp, SENTINEL, dtype=np.uint64).ctypes.data_as(C.c_void_p), C.c_size_t(int(np.prod(shp)) * 8))
            d_a, d_b = g.upload(a[0]), g.upload(b[0])
            _call(g, name, [d_a.ptr], [d_b.ptr], d_out.ptr, nl, 0)
            g.sync()
            assert (g.download(d_out, shp) == SENTINEL).all(), name + ": count = 0 writes nothing"
            for x in (d_out, d_a, d_b):
                x.free()


# ---- refused calls: nothing written, the context still works ----
def test_refused_calls(oracle_mod, capi, relin_rigs):
    r = relin_rigs("ckks", 4096, FP_CHAIN)
    g, n, nl, count = r.g, r.n, 3, 3
    a, b = r.terms(nl, count, 2)
    d_a, d_b = [g.upload(x) for x in a], [g.upload(x) for x in b]
    sentinel = np.full((count, 3, nl, n), SENTINEL, dtype=np.uint64)
    d_o = g.upload(sentinel)
    held = g.held_buffers()
    pa, pb = [x.ptr for x in d_a], [x.ptr for x in d_b]
    words = count * 2 * nl * n

    for name, size in (("multiply_sum", 3), ("mul_sum_relin", 2)):
        def call(as_=pa, bs=pb, k=None, out=None, level=nl, cnt=count):
            k = len(as_) if k is None else k
            g.op(name, g.term_pointers(as_), g.term_pointers(bs), k, out or d_o.ptr, level, C.c_size_t(cnt))

        with pytest.raises(capi.AbcHipError, match="bad term list"):
            call(k=-1)
        with pytest.raises(capi.AbcHipError, match="null term pointer"):
            call(as_=[pa[0], None])
        with pytest.raises(capi.AbcHipError, match="null term pointer"):
            call(bs=[None, pb[1]])
        for level in (0, 4, -1):
            with pytest.raises(capi.AbcHipError, match="limb count out of range"):
                call(level=level)
        out_words = count * size * nl * n
        # a term inside the output: on its first and on its last word; the output on a term's last word
        for off in (1, out_words - 1):
            with pytest.raises(capi.AbcHipError, match="must not overlap"):
                call(as_=[pa[0], C.c_void_p(d_o.ptr.value + 8 * off)])
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(out=C.c_void_p(d_b[1].ptr.value + 8 * (words - 1)))
        if size == 3:  # exactly a term's pointer: legal for mul_sum_relin alone
            with pytest.raises(capi.AbcHipError, match="d_out3 must not overlap a term"):
                call(out=pa[0])
    g.sync()
    _same("refused calls wrote nothing", g.download(d_o, sentinel.shape), sentinel)
    for x, h in zip(d_a + d_b, list(a) + list(b)):
        _same("... nor to a term", g.download(x, h.shape), h)
    assert g.held_buffers() == held

    # no relinearisation key: a context of its own; multiply_sum needs none
    g2 = capi.Context(capi.CKKS, n, r.o.primes)
    try:
        e_a, e_b, e_o = g2.upload(a[0]), g2.upload(b[0]), g2.upload(sentinel)
        with pytest.raises(capi.AbcHipError, match="no relinearisation key"):
            _call(g2, "mul_sum_relin", [e_a.ptr], [e_b.ptr], e_o.ptr, nl, count)
        g2.sync()
        _same("no key: nothing written", g2.download(e_o, sentinel.shape), sentinel)
        _call(g2, "multiply_sum", [e_a.ptr], [e_b.ptr], e_o.ptr, nl, count)
        _same("multiply_sum without a key", g2.download(e_o, sentinel.shape), g.multiply(a[0], b[0]))
    finally:
        g2.close()

    # BFV lives at the top level
    rb = relin_rigs("bfv", 4096)
    ta, tb = rb.terms(rb.L, 2, 5)
    f_a, f_b, f_o = rb.g.upload(ta[0]), rb.g.upload(tb[0]), rb.g.upload(np.full((2, 3, rb.L, rb.n), SENTINEL, dtype=np.uint64))
    for name in ("multiply_sum", "mul_sum_relin"):
        with pytest.raises(capi.AbcHipError, match="top level"):
            _call(rb.g, name, [f_a.ptr], [f_b.ptr], f_o.ptr, rb.L - 1, 2)
    rb.g.sync()
    assert (rb.g.download(f_o, (2, 3, rb.L, rb.n)) == SENTINEL).all()

    # and the context still works
    _same("after the refusals", g.mul_sum_relin(list(a), list(b)), r.want(a, b))
    for x in d_a + d_b + [d_o, f_a, f_b, f_o]:
        x.free()


# ---- recorded circuits ----
@pytest.mark.parametrize("env,tail", [({}, "tensor=sum"), ({"ABC_HIP_NO_TENSOR_SUM": "1"}, "tensor=per_term")], ids=["sum", "per_term"])
def test_recorded_calls_follow_their_inputs(relin_rigs, env, tail):
    """both calls in one recording (eagerly once first: the arenas get their size), replayed twice on rewritten inputs"""
    r = relin_rigs("ckks", 4096, FP_CHAIN)
    g, n, nl, count, K = r.g, r.n, 3, 3, 3
    a, b = r.terms(nl, count, K)
    with _env(g, env):
        assert g.route("mul_sum_relin", nl, count).endswith(tail)
        d_a, d_b = [g.upload(x) for x in a], [g.upload(x) for x in b]
        d_o3, d_o2 = g.alloc(count * 3 * nl * n * 8), g.alloc(count * 2 * nl * n * 8)
        held = g.held_buffers()

        def circuit():
            _call(g, "multiply_sum", [x.ptr for x in d_a], [x.ptr for x in d_b], d_o3.ptr, nl, count)
            _call(g, "mul_sum_relin", [x.ptr for x in d_a], [x.ptr for x in d_b], d_o2.ptr, nl, count)

        circuit()
        g.sync()
        g.graph_begin()
        circuit()
        exe = g.graph_end()
        try:
            for turn, order in enumerate(([0, 1, 2], [2, 0, 1], [1, 2, 0])):
                a2, b2 = np.ascontiguousarray(a[:, order]), np.ascontiguousarray(b[order][:, ::-1])
                for d, h in zip(d_a + d_b, list(a2) + list(b2)):
                    g.op("memcpy_h2d", d.ptr, h.ctypes.data_as(C.c_void_p), C.c_size_t(h.nbytes))
                for d, words in ((d_o3, count * 3 * nl * n), (d_o2, count * 2 * nl * n)):
                    g.op("memcpy_h2d", d.ptr, np.full(words, SENTINEL, dtype=np.uint64).ctypes.data_as(C.c_void_p), C.c_size_t(words * 8))
                if turn:
                    g.graph_launch(exe)
                else:
                    circuit()
                want3 = np.stack([spec.multiply_sum(r.o, list(a2[:, i]), list(b2[:, i])) for i in range(count)])
                _same("turn %d size 3" % turn, g.download(d_o3, want3.shape), want3)
                _same("turn %d relinearised" % turn, g.download(d_o2, (count, 2, nl, n)), r.want(a2, b2))
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for x in d_a + d_b + [d_o3, d_o2]:
            x.free()


# ---- end to end ----
def test_end_to_end_ckks(capi):
    """encode, encrypt, sum of four slot-wise products, decrypt, decode.  Entries in [-1, 1] at scale 2^40: the bound is four times
    the 1e-4 that tests/test_gpu_mulplain_rescale.py::test_weights_end_to_end allows one product, which is no rescale closer to the noise"""
    n, scale = 4096, 2.0 ** 40
    g = capi.Context(capi.CKKS, n, capi.create_primes(n, [50, 40, 40, 50]))
    try:
        g.keygen(0xE2E)
        rng = np.random.default_rng(23)
        v, w = rng.uniform(-1, 1, (4, n // 2)), rng.uniform(-1, 1, (4, n // 2))
        cv = [g.encrypt(g.ckks_encode(x, scale), seed=10 + i) for i, x in enumerate(v)]
        cw = [g.encrypt(g.ckks_encode(x, scale), seed=20 + i) for i, x in enumerate(w)]
        assert g.route("mul_sum_relin", g.L, 1) == "lds_fp tensor=sum"
        out = g.mul_sum_relin(cv, cw)
        dec = g.ckks_decode(g.decrypt(out), scale * scale)
        err = np.abs(dec.real - (v * w).sum(axis=0)).max()
        print("ckks sum of four products: max |error| = %.3g" % err)
        assert err < 4e-4 and np.abs(dec.imag).max() < 4e-4
    finally:
        g.close()


def test_end_to_end_bfv_and_noise(capi):
    """the same on BFV, exactly; and the lazy result's invariant noise budget is at least the per-term result's (one key switch's
    noise instead of four: a statement about the scheme, read off the two ciphertexts)"""
    g = capi.Context.bfv_default(4096)
    try:
        g.keygen(0xB2E)
        n, t = g.n, g.t
        rng = np.random.default_rng(29)
        v, w = rng.integers(0, 100, (4, n)), rng.integers(0, 100, (4, n))
        cv = [g.encrypt(g.batch_encode(x), seed=10 + i) for i, x in enumerate(v)]
        cw = [g.encrypt(g.batch_encode(x), seed=20 + i) for i, x in enumerate(w)]
        assert g.route("mul_sum_relin", g.L, 1).endswith(" tensor=per_term")
        lazy = g.mul_sum_relin(cv, cw)
        eager = g.mul_relin(cv[0], cw[0])
        for x, y in zip(cv[1:], cw[1:]):
            eager = g.add(eager, g.mul_relin(x, y))
        want = (v * w).sum(axis=0) % t
        for name, ct in (("lazy", lazy), ("eager", eager)):
            assert np.array_equal(np.asarray(g.batch_decode(g.decrypt(ct))) % t, want), name
        nb_lazy, nb_eager = g.noise_budget(lazy), g.noise_budget(eager)
        print("noise budget: lazy %s, per-term %s" % (nb_lazy, nb_eager))
        assert np.all(np.asarray(nb_lazy) >= np.asarray(nb_eager))
    finally:
        g.close()
