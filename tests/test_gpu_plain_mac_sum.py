"""abc_hip_multiply_plain_sum on the device: (addend or 0) + sum over k of plain_k (.) ct_k by the K-term kernel k_ckks_plain_mac_sum, or
term by term under ABC_HIP_NO_PLAIN_MAC_SUM.  Every comparison is word for word against tests/plain_sum_spec.py: the CPU oracle's
multiply_plain per term and its add.

The kernel's decision points, from its constants (abc_kernels_eval.hip), all on both sides in TERMS below: kPlainMacTerms = 8 pointer
pairs per launch (K = 8 | 9, 16 | 17, and 25 = three launches and a tail of one); the fp64 accumulators re-centred after
kPlainMacFpTerms = 4 terms of a launch (K = 4 | 5, and 12 | 13 = 8 + 4 | 5 in a second launch, which carries the first one's words by
pointer); every K from 1 to 9, the tail of the unrolled loop; the integer accumulator, which reduces once per launch: at most 9
products of 60-bit residues, of the 256 that 128 bits hold."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plain_sum_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TERMS = list(range(1, 10)) + [12, 13, 16, 17, 25]
FP_CHAIN, MIXED_CHAIN, WIDE_CHAIN = [50, 40, 40, 50], [60, 40, 40, 60], [60, 60, 60]
SPAN = 512  # coefficients of one limb a workgroup of the kernel owns


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


def _call(g, ct_ptrs, plain_ptrs, stride, addend, out, size, nl, count, n_terms=None):
    g.op("multiply_plain_sum", g.term_pointers(ct_ptrs), g.term_pointers(plain_ptrs), C.c_size_t(stride),
         len(ct_ptrs) if n_terms is None else n_terms, addend, out, size, nl, C.c_size_t(count))


def _fill(g, buf, arr):
    arr = np.ascontiguousarray(arr)
    g.op("memcpy_h2d", buf.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes))


def _data(kind, rng, primes, L, nl, size, terms, count, n):
    """(cts [terms][count][size][nl][N], plains [terms][count][L][N]): the data kinds of tests/test_gpu_mul_sum.py; every plaintext
    row is encoded for the whole chain (limb j modulo q_j), and differs per term and per ciphertext"""
    qs = np.array(primes[:L], dtype=np.uint64)
    if kind == "random":
        a = np.stack([rng.integers(0, q, size=(terms, count, size, n), dtype=np.uint64) for q in primes[:nl]], axis=3)
        p = np.stack([rng.integers(0, q, size=(terms, count, n), dtype=np.uint64) for q in primes[:L]], axis=2)
        return a, p
    a = np.empty((terms, count, size, nl, n), dtype=np.uint64)
    p = np.empty((terms, count, L, n), dtype=np.uint64)
    if kind == "max":  # (q - 1)^2 in every product of every term: the largest sums there are
        a[:] = (qs[:nl] - 1)[:, None]
        p[:] = (qs - 1)[:, None]
        return a, p
    # 0 / 1 / q-1 by coefficient index, shifted per term and ciphertext, q-1 in both factors at the ends of the ring and of a span
    idx = np.arange(n)
    vals = np.stack([np.zeros_like(qs), np.ones_like(qs), qs - 1])  # [3][L]
    for k in range(terms):
        for r in range(count):
            a[k, r] = vals[(idx + k + r) % 3, :nl].T
            p[k, r] = vals[(2 * idx + k + 2 * r) % 3].T
    for s in (0, 1, SPAN - 1, SPAN, n - SPAN - 1, n - SPAN, n - 2, n - 1):
        a[..., s] = qs[:nl] - 1
        p[..., s] = qs - 1
    return a, p


def _prefix_sums(o, a, p, ks):
    """{K: [count][size][nl][N]} for every K in ks: the oracle's multiply_plain per term and ciphertext, added up once in term order;
    p [terms][count][rows][N], or [terms][rows][N] for one plaintext per term"""
    count = a.shape[1]
    want, acc = {}, [None] * count
    for k in range(max(ks)):
        for r in range(count):
            acc[r] = spec.multiply_plain_sum(o, [a[k, r]], [p[k, r] if p.ndim == 4 else p[k]], addend=acc[r])
        if k + 1 in ks:
            want[k + 1] = np.stack(acc)
    return want


class Rig:
    """one oracle and one device context on a CKKS chain at N = 2^10, count 3; the references of every K, computed once per
    (data kind, level, size) and left unchanged"""

    def __init__(self, om, capi, bits, n=1024):
        primes = om.create_primes(n, bits)
        self.o = om.Oracle(om.CKKS, n, primes)
        self.g = capi.Context(capi.CKKS, n, self.o.primes)
        self.n, self.primes, self.bits, self.L = n, list(primes), bits, len(primes) - 1
        self._cases = {}

    def case(self, kind, nl, size, count=3):
        key = (kind, nl, size, count)
        if key not in self._cases:
            rng = np.random.default_rng(sum(self.bits) + 10 * nl + size)
            a, p = _data(kind, rng, self.primes, self.L, nl, size, max(TERMS), count, self.n)
            per_ct, per_term = _prefix_sums(self.o, a, p, set(TERMS)), _prefix_sums(self.o, a, p[:, 0], set(TERMS))
            for w in list(per_ct.values()) + list(per_term.values()) + [a, p]:
                w.setflags(write=False)
            self._cases[key] = (a, p, per_ct, per_term)
        return self._cases[key]

    def check(self, tag, nl, sizes=(2, 3), kinds=("random", "max", "pattern"), ks=TERMS):
        g, n, L = self.g, self.n, self.L
        for size in sizes:
            for kind in kinds:
                a, p, per_ct, per_term = self.case(kind, nl, size)
                count = a.shape[1]
                d_a, d_p = [g.upload(x) for x in a], [g.upload(x) for x in p]
                d_o = g.upload(np.full((count, size, nl, n), SENTINEL, dtype=np.uint64))
                try:
                    for K in ks:
                        what = "%s nl=%d size=%d %s K=%d" % (tag, nl, size, kind, K)
                        # one plaintext per ciphertext, rows of L limbs L * N apart (nl < L: rows of a higher level)
                        _call(g, [x.ptr for x in d_a[:K]], [x.ptr for x in d_p[:K]], L * n, None, d_o.ptr, size, nl, count)
                        _same(what + " per ciphertext", g.download(d_o, per_ct[K].shape), per_ct[K])
                        # one plaintext per term for the batch: the first ciphertext's row
                        _call(g, [x.ptr for x in d_a[:K]], [x.ptr for x in d_p[:K]], 0, None, d_o.ptr, size, nl, count)
                        _same(what + " per term", g.download(d_o, per_term[K].shape), per_term[K])
                    for d, h in zip(d_a + d_p, list(a) + list(p)):
                        _same("an operand is left alone", g.download(d, h.shape), h)
                finally:
                    for x in d_a + d_p + [d_o]:
                        x.free()

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def rigs(oracle_mod, capi):
    made = {}

    def get(bits):
        if tuple(bits) not in made:
            made[tuple(bits)] = Rig(oracle_mod, capi, bits)
        return made[tuple(bits)]

    yield get
    for r in made.values():
        r.close()


# ---- the kernel, every K ----
@pytest.mark.parametrize("nl", [3, 1])
def test_kernel_fp_chain(rigs, nl):
    r = rigs(FP_CHAIN)
    assert " macsum=kernel " in r.g.route("diag_matvec_bsgs", nl, 3)
    r.check("fp", nl)


def test_kernel_mixed_chain(rigs):
    """limb 0 on the integers, limbs 1 and 2 in fp64, one launch"""
    rigs(MIXED_CHAIN).check("mixed", 3)


def test_kernel_mixed_chain_all_integer(rigs):
    r = rigs(MIXED_CHAIN)
    with _env(r.g, {"ABC_HIP_NO_MIXED": "1"}):
        r.check("no_mixed", 3)


def test_kernel_no_fp64(rigs, capi, monkeypatch):
    """ABC_HIP_NO_FP64 is read when the context is created: the same chain, references shared, integers throughout"""
    r = rigs(MIXED_CHAIN)
    monkeypatch.setenv("ABC_HIP_NO_FP64", "1")
    g = capi.Context(capi.CKKS, r.n, r.o.primes)
    monkeypatch.delenv("ABC_HIP_NO_FP64")
    keep, r.g = r.g, g
    try:
        r.check("no_fp64", 3)
    finally:
        r.g = keep
        g.close()


def test_kernel_widest_primes(rigs):
    """a chain of 60-bit primes, the widest abc_hip_ctx_create accepts"""
    r = rigs(WIDE_CHAIN)
    assert all(p.bit_length() == 60 for p in r.primes)
    r.check("wide", 2)


@pytest.mark.parametrize("bits,nl", [(FP_CHAIN, 3), (MIXED_CHAIN, 3)], ids=["fp", "mixed"])
def test_per_term_route_gives_the_same_words(rigs, bits, nl):
    r = rigs(bits)
    with _env(r.g, {"ABC_HIP_NO_PLAIN_MAC_SUM": "1"}):
        assert " macsum=per_term " in r.g.route("diag_matvec_bsgs", nl, 3)
        r.check("per_term", nl, ks=[1, 2, 5, 9])
    assert " macsum=kernel " in r.g.route("diag_matvec_bsgs", nl, 3)


# ---- addends, plaintext forms, operand forms ----
@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_PLAIN_MAC_SUM": "1"}], ids=["kernel", "per_term"])
@pytest.mark.parametrize("bits,nl", [(FP_CHAIN, 3), (MIXED_CHAIN, 3), (FP_CHAIN, 1)], ids=["fp", "mixed", "fp-1"])
def test_addend_absent_separate_and_the_output_itself(rigs, bits, nl, env):
    r = rigs(bits)
    g, o, n, L = r.g, r.o, r.n, r.L
    with _env(g, env):
        for size in (2, 3):
            a, p, per_ct, _ = r.case("random", nl, size)
            count = a.shape[1]
            addend = np.ascontiguousarray(r.case("max", nl, size)[0][0])  # q - 1 everywhere: the largest carried words
            d_a, d_p = [g.upload(x) for x in a[:17]], [g.upload(x) for x in p[:17]]
            d_add, d_o = g.upload(addend), g.alloc(addend.nbytes)
            try:
                for K in (1, 4, 5, 8, 9, 17):
                    want = np.stack([o.add(addend[i], per_ct[K][i]) for i in range(count)])
                    ca, cp = [x.ptr for x in d_a[:K]], [x.ptr for x in d_p[:K]]
                    _fill(g, d_o, np.full(addend.shape, SENTINEL, dtype=np.uint64))
                    _call(g, ca, cp, L * n, d_add.ptr, d_o.ptr, size, nl, count)
                    _same("size %d K=%d separate addend" % (size, K), g.download(d_o, want.shape), want)
                    _same("the addend is left alone", g.download(d_add, addend.shape), addend)
                    _fill(g, d_o, addend)
                    _call(g, ca, cp, L * n, d_o.ptr, d_o.ptr, size, nl, count)
                    _same("size %d K=%d d_out is d_addend" % (size, K), g.download(d_o, want.shape), want)
            finally:
                for x in d_a + d_p + [d_add, d_o]:
                    x.free()


def test_plaintext_forms_and_operand_forms(rigs):
    r = rigs(FP_CHAIN)
    g, o, n, L, nl, size = r.g, r.o, r.n, r.L, 2, 2
    a, p, _, _ = r.case("random", nl, size)
    count, K = a.shape[1], 3
    ref = lambda cts, pls: np.stack([spec.multiply_plain_sum(o, [c[i] for c in cts], [q[i] for q in pls]) for i in range(count)])  # noqa: E731
    # rows of exactly nl limbs, nl * N apart
    compact = np.ascontiguousarray(p[:K, :, :nl])
    assert compact.shape[2] * n == nl * n < L * n
    got = g.multiply_plain_sum(list(a[:K]), list(compact))
    _same("rows of nl limbs", got, ref(a[:K], p[:K]))
    _same("rows of L limbs at nl < L", g.multiply_plain_sum(list(a[:K]), list(p[:K])), ref(a[:K], p[:K]))
    bcast = [np.ascontiguousarray(p[k, k % count, :nl]) for k in range(K)]
    want_b = np.stack([spec.multiply_plain_sum(o, [a[k, i] for k in range(K)], bcast) for i in range(count)])
    _same("one plaintext per term", g.multiply_plain_sum(list(a[:K]), bcast), want_b)
    # one pointer in two terms: the ciphertext, the plaintext, and the whole pair
    x, y, pa, pb = a[0], a[1], p[0], p[1]
    _same("a ciphertext in two terms", g.multiply_plain_sum([x, x, y], [pa, pb, pa]), ref([x, x, y], [pa, pb, pa]))
    _same("a pair twice", g.multiply_plain_sum([x, y, x], [pa, pb, pa]), ref([x, y, x], [pa, pb, pa]))
    # sub-ranges of one allocation: ciphertexts, plaintexts, addend and output back to back
    ct_words, pl_words = x.size, pa.size
    block = np.concatenate([x.ravel(), y.ravel(), pa.ravel(), pb.ravel(), a[2].ravel(), np.full(ct_words, SENTINEL, dtype=np.uint64)])
    d = g.upload(block)
    try:
        at = lambda w: C.c_void_p(d.ptr.value + 8 * w)  # noqa: E731
        o_pl, o_add, o_out = 2 * ct_words, 2 * ct_words + 2 * pl_words, 3 * ct_words + 2 * pl_words
        _call(g, [at(0), at(ct_words)], [at(o_pl), at(o_pl + pl_words)], L * n, at(o_add), at(o_out), size, nl, count)
        back = g.download(d, block.shape)
        want = np.stack([o.add(a[2, i], ref([x, y], [pa, pb])[i]) for i in range(count)])
        _same("sub-ranges of one allocation", back[o_out:].reshape(want.shape), want)
        _same("... and nothing else written", back[:o_out], block[:o_out])
    finally:
        d.free()


def test_no_terms_and_no_ciphertexts(rigs):
    r = rigs(FP_CHAIN)
    g, n, nl = r.g, r.n, 3
    for size in (2, 3):
        a, p, _, _ = r.case("random", nl, size)
        count = a.shape[1]
        shp = (count, size, nl, n)
        sentinel = np.full(shp, SENTINEL, dtype=np.uint64)
        d_o, d_a, d_p = g.upload(sentinel), g.upload(a[0]), g.upload(p[0])
        try:
            _call(g, [], [], 0, None, d_o.ptr, size, nl, count)
            assert not g.download(d_o, shp).any(), "an empty sum without an addend is zero"
            _fill(g, d_o, sentinel)
            _call(g, [], [], 0, d_a.ptr, d_o.ptr, size, nl, count)
            _same("an empty sum is the addend", g.download(d_o, shp), a[0])
            _call(g, [], [], 0, d_o.ptr, d_o.ptr, size, nl, count)
            _same("... also in place", g.download(d_o, shp), a[0])
            _fill(g, d_o, sentinel)
            _call(g, [d_a.ptr], [d_p.ptr], 0, d_a.ptr, d_o.ptr, size, nl, 0)
            g.sync()
            _same("count = 0 writes nothing", g.download(d_o, shp), sentinel)
        finally:
            for x in (d_o, d_a, d_p):
                x.free()
    _same("the convenience form of an empty sum", g.multiply_plain_sum([], [], size=3, nl=2, count=2), np.zeros((2, 3, 2, n), dtype=np.uint64))


# ---- refused calls: nothing written, the context still works ----
def test_refused_calls(rigs, capi):
    r = rigs(FP_CHAIN)
    g, n, L, nl, size = r.g, r.n, r.L, 2, 2
    a, p, per_ct, _ = r.case("random", nl, size)
    count = a.shape[1]
    d_a, d_p = [g.upload(x) for x in a[:2]], [g.upload(x) for x in p[:2]]
    sentinel = np.full((count, size, nl, n), SENTINEL, dtype=np.uint64)
    d_o, d_add = g.upload(sentinel), g.upload(a[2])
    held = g.held_buffers()
    ca, cp = [x.ptr for x in d_a], [x.ptr for x in d_p]
    words, plain_words = count * size * nl * n, (count - 1) * L * n + nl * n

    def call(cts=ca, pls=cp, stride=L * n, addend=None, out=None, sz=size, level=nl, k=None):
        _call(g, cts, pls, stride, addend, out or d_o.ptr, sz, level, count, n_terms=k)

    with pytest.raises(capi.AbcHipError, match="bad term list"):
        call(k=-1)
    with pytest.raises(capi.AbcHipError, match="null term pointer"):
        call(cts=[ca[0], None])
    with pytest.raises(capi.AbcHipError, match="null term pointer"):
        call(pls=[None, cp[1]])
    for level in (0, L + 1, -1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            call(level=level)
    for sz in (1, 4, 0):
        with pytest.raises(capi.AbcHipError, match="size must be 2 or 3"):
            call(sz=sz)
    for stride in (1, nl * n - 1):
        with pytest.raises(capi.AbcHipError, match="plain_stride must be 0 or at least nl"):
            call(stride=stride)
    at = lambda buf, w: C.c_void_p(buf.ptr.value + 8 * w)  # noqa: E731
    # a term inside the output: on its first and on its last word; the output on a term's last word
    for off in (1, words - 1):
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(cts=[ca[0], at(d_o, off)])
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(pls=[at(d_o, off), cp[1]])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_a[1], words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_p[0], plain_words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=ca[0])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(pls=[cp[0], cp[1]], stride=0, out=at(d_p[1], nl * n - 1))
    # the addend: exactly d_out or clear of it
    for off in (1, words - 1):
        with pytest.raises(capi.AbcHipError, match="may be d_addend"):
            call(addend=at(d_o, off))
    with pytest.raises(capi.AbcHipError, match="may be d_addend"):
        call(addend=d_add.ptr, out=at(d_add, words - 1))
    g.sync()
    _same("refused calls wrote nothing", g.download(d_o, sentinel.shape), sentinel)
    for x, h in zip(d_a + d_p + [d_add], list(a[:2]) + list(p[:2]) + [a[2]]):
        _same("... nor to an operand", g.download(x, h.shape), h)
    assert g.held_buffers() == held

    # a BFV context
    gb = capi.Context.bfv_default(4096)
    try:
        f_a, f_p = gb.upload(np.zeros((1, 2, gb.L, gb.n), dtype=np.uint64)), gb.upload(np.zeros((gb.L, gb.n), dtype=np.uint64))
        f_o = gb.upload(np.full((1, 2, gb.L, gb.n), SENTINEL, dtype=np.uint64))
        with pytest.raises(capi.AbcHipError, match="CKKS only"):
            _call(gb, [f_a.ptr], [f_p.ptr], 0, None, f_o.ptr, 2, gb.L, 1)
        gb.sync()
        assert (gb.download(f_o, (1, 2, gb.L, gb.n)) == SENTINEL).all()
    finally:
        gb.close()

    # and the context still works
    call()
    _same("after the refusals", g.download(d_o, sentinel.shape), per_ct[2])
    for x in d_a + d_p + [d_o, d_add]:
        x.free()


# ---- other rings ----
@pytest.mark.parametrize("n,bits,nl,K", [(16384, [50, 40, 40, 40, 50], 4, 9), (32768, FP_CHAIN, 3, 5)], ids=["2^14", "2^15"])
def test_other_rings(oracle_mod, capi, n, bits, nl, K):
    om = oracle_mod
    o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
    g = capi.Context(capi.CKKS, n, o.primes)
    try:
        rng = np.random.default_rng(n)
        a, p = _data("random", rng, o.primes, o.L, nl, 2, K, 2, n)
        want = _prefix_sums(o, a, p, {K})[K]
        want = np.stack([o.add(a[0, i], want[i]) for i in range(2)])
        _same("N=%d nl=%d K=%d" % (n, nl, K), g.multiply_plain_sum(list(a), list(p), addend=a[0]), want)
    finally:
        g.close()


# ---- recorded circuits ----
@pytest.mark.parametrize("env,tail", [({}, "macsum=kernel"), ({"ABC_HIP_NO_PLAIN_MAC_SUM": "1"}, "macsum=per_term")], ids=["kernel", "per_term"])
def test_recorded_call_follows_its_inputs(rigs, env, tail):
    """the call in a recording (eagerly once first: the arena gets its size), replayed twice on rewritten inputs; K = 9 is two launches"""
    r = rigs(FP_CHAIN)
    g, o, n, L, nl, size, K = r.g, r.o, r.n, r.L, 3, 2, 9
    a, p, _, _ = r.case("random", nl, size)
    count = a.shape[1]
    with _env(g, env):
        assert tail in g.route("diag_matvec_bsgs", nl, count)
        d_a, d_p = [g.upload(x) for x in a[:K]], [g.upload(x) for x in p[:K]]
        d_add, d_o = g.upload(a[K]), g.alloc(a[K].nbytes)
        held = g.held_buffers()

        def circuit():
            _call(g, [x.ptr for x in d_a], [x.ptr for x in d_p], L * n, d_add.ptr, d_o.ptr, size, nl, count)

        circuit()
        g.sync()
        g.graph_begin()
        circuit()
        exe = g.graph_end()
        try:
            for turn, order in enumerate(([0, 1, 2], [2, 0, 1], [1, 2, 0])):
                a2, p2 = np.ascontiguousarray(a[:K + 1][:, order]), np.ascontiguousarray(p[:K][::-1][:, order])
                for d, h in zip(d_a + d_p + [d_add], list(a2[:K]) + list(p2) + [a2[K]]):
                    _fill(g, d, h)
                _fill(g, d_o, np.full(a2[K].shape, SENTINEL, dtype=np.uint64))
                if turn:
                    g.graph_launch(exe)
                else:
                    circuit()
                want = np.stack([spec.multiply_plain_sum(o, list(a2[:K, i]), list(p2[:, i]), addend=a2[K, i]) for i in range(count)])
                _same("turn %d" % turn, g.download(d_o, want.shape), want)
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for x in d_a + d_p + [d_add, d_o]:
            x.free()
