"""abc_hip_multiply_plain_sum_rescale on the device: rescale((addend or 0) + sum over k of plain_k (.) ct_k), the sum of the last up
to eight terms formed in the loads of the LDS-resident rescale kernels (k_plainsum_rescale_intt_fp / _intt_mixed / _ntt), the terms
before those by k_ckks_plain_mac_sum into an arena; or the whole sum into the arena and the rescale on it (sumrescale=separate).
Every comparison is word for word against tests/plain_sum_rescale_spec.py: the CPU oracle's multiply_plain per term, its add, and ONE
rescale behind the sum.

By measurement the route fuses sums of up to four terms on large batches only (test_the_measured_rule_...); the parity tests below run
under ABC_HIP_PLAIN_SUM_RESCALE_TERMS=8, which fuses at every shape with up to eight terms in the pair.  The decision points, all on
both sides in TERMS below: eight terms in the pair (K = 8 | 9: from 9 on the streaming kernel feeds the carry; 16 | 17: one leading
launch | two; 25: three and a tail of one); the fp64 accumulator is
re-centred after kPlainMacFpTerms = 4 products (K = 4 | 5, and 12 | 13 = a carry plus 4 | 5); every K from 1 to 9, the tail of the
unrolled loop; the integer accumulator reduces once: a carried word and 8 products of 60-bit residues, of the 256 that 128 bits hold."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plain_sum_rescale_spec as spec  # noqa: E402
import plain_sum_spec as base  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TERMS = list(range(1, 10)) + [12, 13, 16, 17, 25]
FP_CHAIN, MIXED_CHAIN, WIDE_CHAIN = [50, 40, 40, 50], [60, 40, 40, 60], [60, 60, 60]


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


@contextlib.contextmanager
def _env(g, settings):
    """the ABC_HIP_* switches are read by reload_env (a value of None: unset); restored, and read again, on the way out"""
    old = {k: os.environ.get(k) for k in settings}
    for k, v in settings.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
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
    g.op("multiply_plain_sum_rescale", g.term_pointers(ct_ptrs), g.term_pointers(plain_ptrs), C.c_size_t(stride),
         len(ct_ptrs) if n_terms is None else n_terms, addend, out, size, nl, C.c_size_t(count))


def _fill(g, buf, arr):
    arr = np.ascontiguousarray(arr)
    g.op("memcpy_h2d", buf.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes))


def _data(kind, rng, primes, L, nl, size, terms, count, n):
    """(cts [terms][count][size][nl][N], plains [terms][count][L][N]); every plaintext row is encoded for the whole chain (limb j modulo
    q_j), and differs per term and per ciphertext.  random; max: q - 1 in every ciphertext and plaintext word; pattern: 0 / 1 / q - 1 by
    coefficient, with q - 1 in both factors at the ends of the ring and of a workgroup's N / 16 threads, on every limb -- the dropped
    one and the kept ones"""
    qs = np.array(primes[:L], dtype=np.uint64)
    if kind == "random":
        a = np.stack([rng.integers(0, q, size=(terms, count, size, n), dtype=np.uint64) for q in primes[:nl]], axis=3)
        p = np.stack([rng.integers(0, q, size=(terms, count, n), dtype=np.uint64) for q in primes[:L]], axis=2)
        return a, p
    a = np.empty((terms, count, size, nl, n), dtype=np.uint64)
    p = np.empty((terms, count, L, n), dtype=np.uint64)
    if kind == "max":
        a[:] = (qs[:nl] - 1)[:, None]
        p[:] = (qs - 1)[:, None]
        return a, p
    idx = np.arange(n)
    vals = np.stack([np.zeros_like(qs), np.ones_like(qs), qs - 1])  # [3][L]
    for k in range(terms):
        for r in range(count):
            a[k, r] = vals[(idx + k + r) % 3, :nl].T
            p[k, r] = vals[(2 * idx + k + 2 * r) % 3].T
    t = n // 16  # threads of a workgroup
    for s in (0, 1, t - 1, t, 2 * t - 1, n // 2 - 1, n // 2, n - t - 1, n - t, n - 2, n - 1):
        a[..., s] = qs[:nl] - 1
        p[..., s] = qs - 1
    return a, p


def _prefix_sums(o, a, p, ks, addend=None):
    """{K: [count][size][nl][N]} for every K in ks: (addend or 0) + the oracle's multiply_plain per term and ciphertext, added up once in
    term order, NOT rescaled; p [terms][count][rows][N], or [terms][rows][N] for one plaintext per term"""
    count = a.shape[1]
    want, acc = {}, [None if addend is None else addend[r] for r in range(count)]
    for k in range(max(ks)):
        for r in range(count):
            acc[r] = base.multiply_plain_sum(o, [a[k, r]], [p[k, r] if p.ndim == 4 else p[k]], addend=acc[r])
        if k + 1 in ks:
            want[k + 1] = np.stack(acc)
    return want


def _rescaled(o, sums):
    return {K: np.stack([o.rescale(x) for x in v]) for K, v in sums.items()}


class Rig:
    """one oracle and one device context on a CKKS chain at N = 2^10, count 3; the references of every K, computed once per (data kind,
    level, size) and left unchanged"""

    def __init__(self, om, capi, bits, n=1024):
        primes = om.create_primes(n, bits)
        self.o = om.Oracle(om.CKKS, n, primes)
        self.g = capi.Context(capi.CKKS, n, self.o.primes)
        self.n, self.primes, self.bits, self.L = n, list(primes), bits, len(primes) - 1
        self._cases = {}

    def case(self, kind, nl, size, count=3):
        """(a, p, addend, sums, want): sums / want[form][K], form 0 .. 3 = per ciphertext, per term, and either with the addend"""
        key = (kind, nl, size, count)
        if key not in self._cases:
            rng = np.random.default_rng(sum(self.bits) + 10 * nl + size)
            a, p = _data(kind, rng, self.primes, self.L, nl, size, max(TERMS), count, self.n)
            # the addend: q - 1 everywhere for the max kind (the largest carried words), else random
            addend = np.ascontiguousarray(_data("max" if kind == "max" else "random", rng, self.primes, self.L, nl, size, 1, count, self.n)[0][0])
            ks = set(TERMS)
            sums = [_prefix_sums(self.o, a, p, ks), _prefix_sums(self.o, a, p[:, 0], ks), _prefix_sums(self.o, a, p, ks, addend),
                    _prefix_sums(self.o, a, p[:, 0], ks, addend)]
            want = [_rescaled(self.o, s) for s in sums]
            for w in [x for d in sums + want for x in d.values()] + [a, p, addend]:
                w.setflags(write=False)
            self._cases[key] = (a, p, addend, sums, want)
        return self._cases[key]

    def check(self, tag, nl, sizes=(2, 3), kinds=("random", "max", "pattern"), ks=TERMS):
        g, n, L = self.g, self.n, self.L
        for size in sizes:
            for kind in kinds:
                a, p, addend, _, want = self.case(kind, nl, size)
                count = a.shape[1]
                d_a, d_p, d_add = [g.upload(x) for x in a], [g.upload(x) for x in p], g.upload(addend)
                shp = (count, size, nl - 1, n)
                d_o = g.upload(np.full(shp, SENTINEL, dtype=np.uint64))
                try:
                    for K in ks:
                        what = "%s nl=%d size=%d %s K=%d" % (tag, nl, size, kind, K)
                        ca, cp = [x.ptr for x in d_a[:K]], [x.ptr for x in d_p[:K]]
                        # one plaintext per ciphertext, rows of L limbs L * N apart (nl < L: rows of a higher level); then one per term
                        for form, (stride, add) in enumerate(((L * n, None), (0, None), (L * n, d_add.ptr), (0, d_add.ptr))):
                            _call(g, ca, cp, stride, add, d_o.ptr, size, nl, count)
                            _same("%s form %d" % (what, form), g.download(d_o, shp), want[form][K])
                    for d, h in zip(d_a + d_p + [d_add], list(a) + list(p) + [addend]):
                        _same("an operand is left alone", g.download(d, h.shape), h)
                finally:
                    for x in d_a + d_p + [d_o, d_add]:
                        x.free()

    def close(self):
        self.g.close()


FORCE = "ABC_HIP_PLAIN_SUM_RESCALE_TERMS"


@pytest.fixture(scope="module", autouse=True)
def fused_at_every_shape():
    """the route sends small batches and long sums to the separate route by measurement; the parity tests of the K-term kernels run
    them at count 3 and K up to 25 all the same: ABC_HIP_PLAIN_SUM_RESCALE_TERMS=8 for this module (the tests of the rule unset it)"""
    old = os.environ.get(FORCE)
    os.environ[FORCE] = "8"
    yield
    if old is None:
        os.environ.pop(FORCE, None)
    else:
        os.environ[FORCE] = old


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


# ---- the fused pair, every K ----
@pytest.mark.parametrize("nl", [3, 2])
def test_fused_fp_chain(rigs, nl):
    r = rigs(FP_CHAIN)
    assert r.g.route("plain_sum_rescale", nl, 3) == "fp sumrescale=fused"
    r.check("fp", nl)


def test_fused_mixed_chain(rigs):
    """limb 0 on the integers, limbs 1 and 2 -- the dropped one -- in fp64"""
    r = rigs(MIXED_CHAIN)
    assert r.g.route("plain_sum_rescale", 3, 3) == "mixed fpmask=0x6 sumrescale=fused"
    r.check("mixed", 3)


def test_fused_mixed_chain_integer_dropped_limb(rigs):
    """two limbs of {60,40,...}: the kept limb on the integers, the dropped one in fp64; and under NO_MIXED all on the integers"""
    r = rigs(MIXED_CHAIN)
    assert r.g.route("plain_sum_rescale", 2, 3) == "mixed fpmask=0x2 sumrescale=fused"
    r.check("mixed-2", 2, kinds=("max", "pattern"), ks=[1, 5, 8, 9])
    with _env(r.g, {"ABC_HIP_NO_MIXED": "1"}):
        assert r.g.route("plain_sum_rescale", 3, 3) == "mixed fpmask=0x0 sumrescale=fused"
        r.check("no_mixed", 3)


def test_fused_no_fp64(rigs, capi, monkeypatch):
    """ABC_HIP_NO_FP64 is read when the context is created: the same chain, references shared, integers throughout"""
    r = rigs(MIXED_CHAIN)
    monkeypatch.setenv("ABC_HIP_NO_FP64", "1")
    g = capi.Context(capi.CKKS, r.n, r.o.primes)
    monkeypatch.delenv("ABC_HIP_NO_FP64")
    keep, r.g = r.g, g
    try:
        assert g.route("plain_sum_rescale", 3, 3) == "mixed fpmask=0x0 sumrescale=fused"
        r.check("no_fp64", 3)
    finally:
        r.g = keep
        g.close()


def test_fused_widest_primes(rigs):
    """a chain of 60-bit primes, the widest abc_hip_ctx_create accepts: the dropped limb's inverse transform on the integers"""
    r = rigs(WIDE_CHAIN)
    assert all(p.bit_length() == 60 for p in r.primes)
    assert r.g.route("plain_sum_rescale", 2, 3) == "mixed fpmask=0x0 sumrescale=fused"
    r.check("wide", 2)


# ---- fewer terms in the fused pair: the streaming kernel takes whole launches first, down to the carry alone ----
@pytest.mark.parametrize("terms", ["4", "2", "1", "0"])
def test_fewer_fused_terms_give_the_same_words(rigs, terms):
    for bits, nl in ((FP_CHAIN, 3), (MIXED_CHAIN, 3)):
        r = rigs(bits)
        with _env(r.g, {FORCE: terms}):
            assert r.g.route("plain_sum_rescale", nl, 3).endswith("sumrescale=fused")
            r.check("fused terms " + terms, nl, sizes=(2,), kinds=("random", "max"), ks=[1, 2, 3, 4, 5, 8, 9, 12, 17])


# ---- the route's own rule (profiles/plain_sum_rescale_ab.log): up to four terms, 256 polynomials and 2^20 coefficients ----
def test_the_measured_rule_on_a_small_and_on_a_large_batch(rigs):
    r = rigs(FP_CHAIN)
    g, o, n, L, nl, count = r.g, r.o, r.n, r.L, 2, 512
    with _env(g, {FORCE: None}):
        assert g.route("plain_sum_rescale", 3, 3) == "fp sumrescale=separate"
        r.check("rule, count 3", 3, sizes=(2,), kinds=("random",), ks=[1, 4, 5, 9])
        assert g.route("plain_sum_rescale", nl, count) == "fp sumrescale=fused"      # 1024 polynomials of 2^10 coefficients
        assert g.route("plain_sum_rescale", nl, count - 1) == "fp sumrescale=separate"
        rng = np.random.default_rng(512)
        a, p = _data("random", rng, r.primes, L, nl, 2, 5, count, n)
        for K in (2, 4, 5):  # 4 | 5: the pair takes the whole sum | the separate route
            want = _rescaled(o, _prefix_sums(o, a[:K], p[:K, 0], {K}))[K]
            _same("count %d K=%d" % (count, K), g.multiply_plain_sum_rescale(list(a[:K]), list(p[:K, 0])), want)
            with _env(g, {"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"}):
                _same("... separate", g.multiply_plain_sum_rescale(list(a[:K]), list(p[:K, 0])), want)


# ---- the separate route gives the same words ----
@pytest.mark.parametrize("env,route", [({"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"}, "fp sumrescale=separate"),
                                       ({"ABC_HIP_NO_PLAIN_MAC_SUM": "1"}, "fp sumrescale=separate"),
                                       ({"ABC_HIP_NO_FUSED": "1"}, "generic sumrescale=separate")], ids=["no_fusion", "no_mac_sum", "no_fused"])
def test_separate_route_gives_the_same_words(rigs, env, route):
    r = rigs(FP_CHAIN)
    with _env(r.g, env):
        assert r.g.route("plain_sum_rescale", 3, 3) == route
        r.check("separate", 3, kinds=("random", "max"), ks=[1, 2, 5, 8, 9, 17])
    assert r.g.route("plain_sum_rescale", 3, 3) == "fp sumrescale=fused"


def test_separate_route_on_a_wide_chain_without_the_integer_kernels(rigs):
    r = rigs(MIXED_CHAIN)
    with _env(r.g, {"ABC_HIP_NO_ISPLIT": "1"}):
        assert r.g.route("plain_sum_rescale", 3, 3) == "generic sumrescale=separate"
        r.check("no_isplit", 3, sizes=(2,), kinds=("random",), ks=[3, 9])


# ---- against the device's own calls ----
@pytest.mark.parametrize("bits,nl", [(FP_CHAIN, 3), (MIXED_CHAIN, 3), (WIDE_CHAIN, 2)], ids=["fp", "mixed", "wide"])
def test_equals_the_devices_own_sum_then_rescale_and_its_one_term_call(rigs, bits, nl):
    r = rigs(bits)
    g = r.g
    for size in (2, 3):
        a, p, addend, _, _ = r.case("random", nl, size)
        for K in (1, 8, 9):
            for add in (None, addend):
                two = g.rescale(g.multiply_plain_sum(list(a[:K]), list(p[:K]), addend=add))
                _same("size %d K=%d: multiply_plain_sum + rescale" % (size, K), g.multiply_plain_sum_rescale(list(a[:K]), list(p[:K]), addend=add), two)
        _same("size %d: K = 1 is multiply_plain_rescale" % size, g.multiply_plain_sum_rescale([a[0]], [p[0]]), g.multiply_plain_rescale(a[0], p[0]))
        _same("... with one plaintext for the batch", g.multiply_plain_sum_rescale([a[0]], [p[0, 0]]), g.multiply_plain_rescale(a[0], p[0, 0]))


# ---- plaintext forms, operand forms ----
def test_plaintext_forms_and_operand_forms(rigs):
    r = rigs(FP_CHAIN)
    g, o, n, L, nl, size = r.g, r.o, r.n, r.L, 2, 2
    a, p, _, _, _ = r.case("random", nl, size)
    count, K = a.shape[1], 3
    ref = lambda cts, pls, add=None: np.stack([spec.multiply_plain_sum_rescale(o, [c[i] for c in cts], [q[i] for q in pls],  # noqa: E731
                                                                               addend=None if add is None else add[i]) for i in range(count)])
    compact = np.ascontiguousarray(p[:K, :, :nl])  # rows of exactly nl limbs, nl * N apart
    assert compact.shape[2] * n == nl * n < L * n
    _same("rows of nl limbs", g.multiply_plain_sum_rescale(list(a[:K]), list(compact)), ref(a[:K], p[:K]))
    _same("rows of L limbs at nl < L", g.multiply_plain_sum_rescale(list(a[:K]), list(p[:K])), ref(a[:K], p[:K]))
    bcast = [np.ascontiguousarray(p[k, k % count, :nl]) for k in range(K)]
    want_b = np.stack([spec.multiply_plain_sum_rescale(o, [a[k, i] for k in range(K)], bcast) for i in range(count)])
    _same("one plaintext per term", g.multiply_plain_sum_rescale(list(a[:K]), bcast), want_b)
    # one pointer in two terms: the ciphertext, the plaintext, and the whole pair
    x, y, pa, pb = a[0], a[1], p[0], p[1]
    _same("a ciphertext in two terms", g.multiply_plain_sum_rescale([x, x, y], [pa, pb, pa]), ref([x, x, y], [pa, pb, pa]))
    _same("a pair twice", g.multiply_plain_sum_rescale([x, y, x], [pa, pb, pa]), ref([x, y, x], [pa, pb, pa]))
    # sub-ranges of one allocation: ciphertexts, plaintexts, addend and output back to back
    ct_words, pl_words, out_words = x.size, pa.size, count * size * (nl - 1) * n
    block = np.concatenate([x.ravel(), y.ravel(), pa.ravel(), pb.ravel(), a[2].ravel(), np.full(out_words + 8, SENTINEL, dtype=np.uint64)])
    d = g.upload(block)
    try:
        at = lambda w: C.c_void_p(d.ptr.value + 8 * w)  # noqa: E731
        o_pl, o_add, o_out = 2 * ct_words, 2 * ct_words + 2 * pl_words, 3 * ct_words + 2 * pl_words
        _call(g, [at(0), at(ct_words)], [at(o_pl), at(o_pl + pl_words)], L * n, at(o_add), at(o_out), size, nl, count)
        back = g.download(d, block.shape)
        want = ref([x, y], [pa, pb], a[2])
        _same("sub-ranges of one allocation", back[o_out:o_out + out_words].reshape(want.shape), want)
        _same("... and nothing else written", np.concatenate([back[:o_out], back[o_out + out_words:]]), np.concatenate([block[:o_out], block[o_out + out_words:]]))
    finally:
        d.free()


def test_no_terms_and_no_ciphertexts(rigs):
    r = rigs(FP_CHAIN)
    g, o, n, nl = r.g, r.o, r.n, 3
    for size in (2, 3):
        a, p, _, _, _ = r.case("random", nl, size)
        count = a.shape[1]
        shp = (count, size, nl - 1, n)
        sentinel = np.full(shp, SENTINEL, dtype=np.uint64)
        d_o, d_a, d_p = g.upload(sentinel), g.upload(a[0]), g.upload(p[0])
        try:
            _call(g, [], [], 0, None, d_o.ptr, size, nl, count)
            assert not g.download(d_o, shp).any(), "an empty sum without an addend is zero"
            _fill(g, d_o, sentinel)
            _call(g, [], [], 0, d_a.ptr, d_o.ptr, size, nl, count)
            _same("an empty sum is the rescaled addend", g.download(d_o, shp), np.stack([o.rescale(x) for x in a[0]]))
            _fill(g, d_o, sentinel)
            _call(g, [d_a.ptr], [d_p.ptr], 0, d_a.ptr, d_o.ptr, size, nl, 0)
            g.sync()
            _same("count = 0 writes nothing", g.download(d_o, shp), sentinel)
        finally:
            for x in (d_o, d_a, d_p):
                x.free()
    _same("the convenience form of an empty sum", g.multiply_plain_sum_rescale([], [], size=3, nl=3, count=2), np.zeros((2, 3, 2, n), dtype=np.uint64))


# ---- refused calls: nothing written, the context still works ----
def test_refused_calls(rigs, capi):
    r = rigs(FP_CHAIN)
    g, n, L, nl, size = r.g, r.n, r.L, 2, 2
    a, p, addend, _, want = r.case("random", nl, size)
    count = a.shape[1]
    d_a, d_p = [g.upload(x) for x in a[:2]], [g.upload(x) for x in p[:2]]
    # the output buffer is as large as an INPUT, sentinel throughout: a call that mistook the shapes would show
    sentinel = np.full((count, size, nl, n), SENTINEL, dtype=np.uint64)
    d_o, d_add = g.upload(sentinel), g.upload(addend)
    held = g.held_buffers()
    ca, cp = [x.ptr for x in d_a], [x.ptr for x in d_p]
    in_words, out_words, plain_words = count * size * nl * n, count * size * (nl - 1) * n, (count - 1) * L * n + nl * n

    def call(cts=ca, pls=cp, stride=L * n, add=None, out=None, sz=size, level=nl, k=None):
        _call(g, cts, pls, stride, add, out or d_o.ptr, sz, level, count, n_terms=k)

    with pytest.raises(capi.AbcHipError, match="bad term list"):
        call(k=-1)
    with pytest.raises(capi.AbcHipError, match="null term pointer"):
        call(cts=[ca[0], None])
    with pytest.raises(capi.AbcHipError, match="null term pointer"):
        call(pls=[None, cp[1]])
    for level in (0, L + 1, -1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            call(level=level)
    with pytest.raises(capi.AbcHipError, match="no limb left to drop"):
        call(level=1)
    for sz in (1, 4, 0):
        with pytest.raises(capi.AbcHipError, match="size must be 2 or 3"):
            call(sz=sz)
    for stride in (1, nl * n - 1):
        with pytest.raises(capi.AbcHipError, match="plain_stride must be 0 or at least nl"):
            call(stride=stride)
    at = lambda buf, w: C.c_void_p(buf.ptr.value + 8 * w)  # noqa: E731
    # a term inside the output: on its first and on its last word; the output on a term's last word; equality is no exception
    for off in (0, 1, out_words - 1):
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(cts=[ca[0], at(d_o, off)])
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(pls=[at(d_o, off), cp[1]])
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(add=at(d_o, off))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_a[1], in_words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_p[0], plain_words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=ca[0])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(add=d_add.ptr, out=at(d_add, in_words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(pls=[cp[0], cp[1]], stride=0, out=at(d_p[1], nl * n - 1))
    g.sync()
    _same("refused calls wrote nothing", g.download(d_o, sentinel.shape), sentinel)
    for x, h in zip(d_a + d_p + [d_add], list(a[:2]) + list(p[:2]) + [addend]):
        _same("... nor to an operand", g.download(x, h.shape), h)
    assert g.held_buffers() == held

    # a BFV context
    gb = capi.Context.bfv_default(4096)
    try:
        f_a, f_p = gb.upload(np.zeros((1, 2, gb.L, gb.n), dtype=np.uint64)), gb.upload(np.zeros((gb.L, gb.n), dtype=np.uint64))
        f_o = gb.upload(np.full((1, 2, gb.L, gb.n), SENTINEL, dtype=np.uint64))
        with pytest.raises(capi.AbcHipError, match="CKKS operation"):
            _call(gb, [f_a.ptr], [f_p.ptr], 0, None, f_o.ptr, 2, gb.L, 1)
        gb.sync()
        assert (gb.download(f_o, (1, 2, gb.L, gb.n)) == SENTINEL).all()
    finally:
        gb.close()

    # and the context still works
    call()
    back = g.download(d_o, sentinel.shape).ravel()
    _same("after the refusals", back[:out_words].reshape(want[0][2].shape), want[0][2])
    assert (back[out_words:] == SENTINEL).all(), "nothing behind the nl - 1 limbs per polynomial is written"
    for x in d_a + d_p + [d_o, d_add]:
        x.free()


# ---- other rings ----
@pytest.mark.parametrize("n,bits,nl,K,route", [
    (4096, FP_CHAIN, 3, 9, "fp sumrescale=fused"),
    (16384, [50, 40, 40, 40, 50], 4, 9, "fp sumrescale=fused"),
    (16384, [50, 40, 40, 40, 50], 2, 5, "fp sumrescale=fused"),
    (16384, [60, 40, 40, 60], 3, 9, "mixed fpmask=0x6 sumrescale=fused"),
    (32768, FP_CHAIN, 3, 9, "generic sumrescale=separate"),
], ids=["2^12", "2^14-4", "2^14-2", "2^14-mixed", "2^15"])
def test_other_rings(oracle_mod, capi, n, bits, nl, K, route):
    om = oracle_mod
    o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
    g = capi.Context(capi.CKKS, n, o.primes)
    try:
        assert g.route("plain_sum_rescale", nl, 2) == route
        rng = np.random.default_rng(n + nl)
        a, p = _data("pattern" if nl == 2 else "random", rng, o.primes, o.L, nl, 2, K, 2, n)
        want = _rescaled(o, _prefix_sums(o, a, p, {K}, addend=a[0]))[K]
        _same("N=%d nl=%d K=%d" % (n, nl, K), g.multiply_plain_sum_rescale(list(a), list(p), addend=a[0]), want)
    finally:
        g.close()


# ---- recorded circuits ----
@pytest.mark.parametrize("env,route", [({}, "fp sumrescale=fused"), ({"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"}, "fp sumrescale=separate")],
                         ids=["fused", "separate"])
def test_recorded_call_follows_its_inputs(rigs, env, route):
    """the call in a recording (eagerly once first: the arena gets its size), replayed twice on rewritten inputs; K = 9: one term through
    the streaming kernel and the arena, eight in the fused pair"""
    r = rigs(FP_CHAIN)
    g, o, n, L, nl, size, K = r.g, r.o, r.n, r.L, 3, 2, 9
    a, p, _, _, _ = r.case("random", nl, size)
    count = a.shape[1]
    shp = (count, size, nl - 1, n)
    with _env(g, env):
        assert g.route("plain_sum_rescale", nl, count) == route
        d_a, d_p = [g.upload(x) for x in a[:K]], [g.upload(x) for x in p[:K]]
        d_add, d_o = g.upload(a[K]), g.alloc(int(np.prod(shp)) * 8)
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
                _fill(g, d_o, np.full(shp, SENTINEL, dtype=np.uint64))
                if turn:
                    g.graph_launch(exe)
                else:
                    circuit()
                want = np.stack([spec.multiply_plain_sum_rescale(o, list(a2[:K, i]), list(p2[:, i]), addend=a2[K, i]) for i in range(count)])
                _same("turn %d" % turn, g.download(d_o, shp), want)
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for x in d_a + d_p + [d_add, d_o]:
            x.free()


# ---- from encode to decode ----
def test_weighted_sum_of_four_ciphertexts_from_encode_to_decode(rigs):
    """sum of w_k * x_k over four encrypted vectors, one call, decoded at scale^2 / q_2: within the project's 1e-4 bound"""
    r = rigs(FP_CHAIN)
    g, o, n = r.g, r.o, r.n
    o.keygen(0x51AE, elts=[])
    rng = np.random.default_rng(4)
    scale = 2.0 ** 40
    xs, ws = rng.uniform(-1, 1, (4, n // 2)), rng.uniform(-1, 1, (4, n // 2))
    cts = [o.encrypt(o.ckks_encode(v, scale), 40 + k) for k, v in enumerate(xs)]
    plains = [o.ckks_encode(w, scale) for w in ws]
    got = g.multiply_plain_sum_rescale(cts, plains)
    _same("the call", got, spec.multiply_plain_sum_rescale(o, cts, plains))
    err = np.abs(o.ckks_decode(o.decrypt(got), scale * scale / o.primes[o.L - 1]) - (xs * ws).sum(axis=0)).max()
    print("max |error| of the decoded weighted sum: %.3g" % err)
    assert err < 1e-4
