"""abc_hip_bfv_plain_to_ntt and abc_hip_bfv_multiply_plain_sum on the device: (addend or 0) + sum over k of plain_k * ct_k with ONE
inverse transform, by k_bfv_plain_sum_fp (plainsum=fused) or by stand-alone transforms around k_ckks_plain_mac_sum
(plainsum=ntt_domain).  Every comparison is word for word: against tests/bfv_plain_sum_spec.py (the exact NTT-domain model, which
takes any residues), against abc_hip_multiply_plain (K = 1) and against the device's own multiply_plain + add.

Decision points of the fused kernel (abc_kernels_bfv.hip), both sides in TERMS: kBfvPlainSumTerms = 8 term pointers per launch, an
NTT-domain partial sum in an arena between launches (K = 8 | 9, 16 | 17, 25 = three launches and a tail of one); the fp64
accumulators re-centred after kBfvPlainSumFpTerms = 4 terms (K = 4 | 5, 12 | 13); every K from 1 to 9.  The general route has the
same launch boundary (kPlainMacTerms = 8) for its forward-transform arena and its carry."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfv_plain_sum_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TERMS = list(range(1, 10)) + [12, 13, 16, 17, 25]
N, COUNT = 1024, 3
CHAINS = {"40-40-50": [40, 40, 50], "49-49-50": [49, 49, 50], "50-50-50": [50, 50, 50], "60-40-60": [60, 40, 60]}
LANE = 16  # words of a limb one lane of the fused kernel holds


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


def _call(g, ct_ptrs, form, plain_ptrs, stride, addend, out, size, count, n_terms=None):
    g.op("bfv_multiply_plain_sum", g.term_pointers(ct_ptrs), form, g.term_pointers(plain_ptrs), C.c_size_t(stride),
         len(ct_ptrs) if n_terms is None else n_terms, addend, out, size, C.c_size_t(count))


def _fill(g, buf, arr):
    arr = np.ascontiguousarray(arr)
    g.op("memcpy_h2d", buf.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes))


def _data(kind, rng, qs, size, terms, count, n):
    """(cts [terms][count][size][L][N], plains [terms][count][L][N]): residues below q_i in every word, NTT-form plaintexts as the
    call takes them"""
    L = len(qs)
    qa = np.array(qs, dtype=np.uint64)
    if kind == "random":
        a = np.stack([rng.integers(0, q, size=(terms, count, size, n), dtype=np.uint64) for q in qs], axis=3)
        p = np.stack([rng.integers(0, q, size=(terms, count, n), dtype=np.uint64) for q in qs], axis=2)
        return a, p
    a = np.empty((terms, count, size, L, n), dtype=np.uint64)
    p = np.empty((terms, count, L, n), dtype=np.uint64)
    if kind == "half":
        # NTT-form terms whose products are the largest the fp64 product can be, all of one sign per coefficient: 1 * (q - 1) / 2 is
        # +(q - 1) / 2 at even coefficients, (q - 1) * (q - 1) / 2 is -(q - 1) / 2 at odd ones -- the sums that come closest to the
        # accumulator's limit (on a 50-bit chain: the carried word and eight such products, 5 q of the 8 q that 2^53 holds)
        a[:] = np.where(np.arange(n) % 2 == 0, np.uint64(1), (qa - 1)[:, None])
        p[:] = ((qa - 1) // 2)[:, None]
        return a, p
    if kind == "max":  # q - 1 in every ciphertext and plaintext word: with NTT-form terms every product is (q - 1)^2
        a[:] = (qa - 1)[:, None]
        p[:] = (qa - 1)[:, None]
        return a, p
    # 0 / 1 / q-1 by coefficient index, shifted per term and ciphertext, q-1 in both factors at the ends of the ring and of a lane's words
    idx = np.arange(n)
    vals = np.stack([np.zeros_like(qa), np.ones_like(qa), qa - 1])  # [3][L]
    for k in range(terms):
        for r in range(count):
            a[k, r] = vals[(idx + k + r) % 3].T
            p[k, r] = vals[(2 * idx + k + 2 * r) % 3].T
    for s in (0, 1, LANE - 1, LANE, n - LANE - 1, n - LANE, n - 2, n - 1):
        a[..., s] = qa - 1
        p[..., s] = qa - 1
    return a, p


def _prefix_sums(o, a, p, form, ks):
    """{K: [count][size][L][N]} for every K in ks: the exact NTT-domain sums (Python integers) of the first K terms, inverted once
    per K; p [terms][count][L][N], or [terms][L][N] for one plaintext per term"""
    terms, count, size, L, n = a.shape
    acc = np.zeros((count, size, L, n), dtype=object)
    want = {}
    for k in range(max(ks)):
        for r in range(count):
            x = a[k, r] if form == spec.NTT else spec.ct_to_ntt(o, a[k, r])
            pk = p[k, r] if p.ndim == 4 else p[k]
            acc[r] = acc[r] + x.astype(object) * pk.astype(object)[None]
        if k + 1 in ks:
            out = np.empty((count, size, L, n), dtype=np.uint64)
            for r in range(count):
                for s in range(size):
                    for i in range(L):
                        q = o.primes[i]
                        out[r, s, i] = o.intt(i, np.array([int(v) % q for v in acc[r, s, i]], dtype=np.uint64))
            want[k + 1] = out
    return want


class Rig:
    """one oracle and one device context on a BFV chain at N = 2^10, count 3; the references of every K, computed once per
    (data kind, size, ct_form) and left unchanged"""

    def __init__(self, om, capi, name):
        self.bits = CHAINS[name]
        primes = om.create_primes(N, self.bits)
        t = om.plain_modulus_batching(N, 20)
        self.o = om.Oracle(om.BFV, N, primes, t)
        self.g = capi.Context(capi.BFV, N, self.o.primes, t)
        self.n, self.L, self.qs = N, len(primes) - 1, list(primes[:-1])
        self._cases = {}

    def case(self, kind, size, form):
        key = (kind, size)
        if key not in self._cases:
            rng = np.random.default_rng(sum(self.bits) + size)
            a, p = _data(kind, rng, self.qs, size, max(TERMS), COUNT, self.n)
            a.setflags(write=False), p.setflags(write=False)
            self._cases[key] = {"a": a, "p": p}
        c = self._cases[key]
        if form not in c:
            per_ct, per_term = _prefix_sums(self.o, c["a"], c["p"], form, set(TERMS)), _prefix_sums(self.o, c["a"], c["p"][:, 0], form, set(TERMS))
            for w in list(per_ct.values()) + list(per_term.values()):
                w.setflags(write=False)
            c[form] = (per_ct, per_term)
        return (c["a"], c["p"]) + c[form]

    def check(self, tag, size, kinds=("random", "max", "pattern"), ks=TERMS, forms=(spec.COEFF, spec.NTT)):
        g, n, L = self.g, self.n, self.L
        for kind in kinds:
            for form in forms:
                a, p, per_ct, per_term = self.case(kind, size, form)
                d_a, d_p = [g.upload(x) for x in a[:max(ks)]], [g.upload(x) for x in p[:max(ks)]]
                d_o = g.upload(np.full((COUNT, size, L, n), SENTINEL, dtype=np.uint64))
                try:
                    for K in ks:
                        what = "%s size=%d %s form=%d K=%d" % (tag, size, kind, form, K)
                        _call(g, [x.ptr for x in d_a[:K]], form, [x.ptr for x in d_p[:K]], L * n, None, d_o.ptr, size, COUNT)
                        _same(what + " per ciphertext", g.download(d_o, per_ct[K].shape), per_ct[K])
                        _call(g, [x.ptr for x in d_a[:K]], form, [x.ptr for x in d_p[:K]], 0, None, d_o.ptr, size, COUNT)
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

    def get(name):
        if name not in made:
            made[name] = Rig(oracle_mod, capi, name)
        return made[name]

    yield get
    for r in made.values():
        r.close()


# ---- every K, both forms of the terms, three kinds of data ----
@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("name", ["40-40-50", "49-49-50"])
def test_fused_kernel(rigs, name, size):
    r = rigs(name)
    assert r.g.route("bfv_plain_sum", r.L, COUNT) == "plainsum=fused"
    r.check("fused " + name, size)


def test_fused_kernel_on_50_bit_data_primes(rigs):
    """every data prime just below 2^50, where 2^53 is 8 q: products of half a prime's size, one sign per coefficient, and q - 1
    everywhere.  What this can and cannot show is in DESIGN.md: fp_mulmod's products stay within 0.75 q, so no input reaches 8 q in
    one launch even without the re-centring the kernel does after four terms"""
    r = rigs("50-50-50")
    assert all(q.bit_length() == 50 for q in r.qs)
    assert r.g.route("bfv_plain_sum", r.L, COUNT) == "plainsum=fused"
    r.check("fused 50-50-50", 2, kinds=("half", "max"))


@pytest.mark.parametrize("size", [2, 3])
def test_general_route_on_a_wide_prime(rigs, size):
    r = rigs("60-40-60")
    assert r.g.route("bfv_plain_sum", r.L, COUNT) == "plainsum=ntt_domain"
    r.check("general 60-40-60", size)


@pytest.mark.parametrize("size", [2, 3])
def test_general_route_under_no_fused(rigs, size):
    r = rigs("40-40-50")
    with _env(r.g, {"ABC_HIP_NO_FUSED": "1"}):
        assert r.g.route("bfv_plain_sum", r.L, COUNT) == "plainsum=ntt_domain"
        r.check("no_fused", size)
    assert r.g.route("bfv_plain_sum", r.L, COUNT) == "plainsum=fused"


# ---- against the existing calls, on plaintexts modulo t ----
def _real_plains(o, rng, terms, count):
    """[terms][count][N] mod t: t - 1 everywhere, 0 / t - 1 / the two values around the lift threshold by coefficient, random"""
    t, thr = o.t, (o.t + 1) // 2
    edge = np.array([0, t - 1, thr - 1, thr], dtype=np.uint64)
    p = rng.integers(0, t, size=(terms, count, o.n), dtype=np.uint64)
    p[0] = t - 1
    p[1] = edge[np.arange(o.n) % 4]
    return p


@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_FUSED": "1"}], ids=["fused", "ntt_domain"])
@pytest.mark.parametrize("name", ["40-40-50", "60-40-60"])
def test_equals_multiply_plain_and_the_composed_calls(rigs, name, env):
    r = rigs(name)
    g, o, n, L = r.g, r.o, r.n, r.L
    rng = np.random.default_rng(7)
    K = 9
    plains = _real_plains(o, rng, K, COUNT)
    with _env(g, env):
        p_ntt = g.bfv_plain_to_ntt(plains.reshape(-1, n)).reshape(K, COUNT, L, n)
        _same("plain_to_ntt", p_ntt[1, 2], spec.plain_to_ntt(o, plains[1, 2]))
        _same("plain_to_ntt, one row", g.bfv_plain_to_ntt(plains[0, 0]), spec.plain_to_ntt(o, plains[0, 0]))
        for size in (2, 3):
            a = r.case("random", size, spec.COEFF)[0][:K + 1]
            for k in (0, 1, 2):  # K = 1: the words of abc_hip_multiply_plain, one plaintext per ciphertext and one for the batch
                _same("K=1 per ciphertext", g.bfv_multiply_plain_sum([a[k]], [p_ntt[k]]), g.multiply_plain(a[k], plains[k]))
                _same("K=1 per term", g.bfv_multiply_plain_sum([a[k]], [p_ntt[k, 0]]), g.multiply_plain(a[k], plains[k, 0]))
            acc = np.ascontiguousarray(a[K])  # the device's own composed calls, addend first
            for k in range(K):
                acc = g.add(acc, g.multiply_plain(a[k], plains[k]))
            _same("composed on the device", g.bfv_multiply_plain_sum(list(a[:K]), list(p_ntt), addend=a[K]), acc)
            want = np.stack([o.add(a[K, i], spec.composed_sum(o, list(a[:K, i]), list(plains[:, i]))) for i in range(COUNT)])
            _same("composed on the oracle", acc, want)
            a_ntt = [g.ntt_limbs(x) for x in a[:K]]
            _same("terms in NTT form", g.bfv_multiply_plain_sum(a_ntt, list(p_ntt), addend=a[K], ct_form=spec.NTT), acc)


# ---- addends, operand forms ----
@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_FUSED": "1"}], ids=["fused", "ntt_domain"])
@pytest.mark.parametrize("form", [spec.COEFF, spec.NTT], ids=["coeff", "ntt"])
def test_addend_absent_separate_and_the_output_itself(rigs, env, form):
    r = rigs("49-49-50")
    g, o, n, L = r.g, r.o, r.n, r.L
    with _env(g, env):
        for size in (2, 3):
            a, p, per_ct, _ = r.case("random", size, form)
            addend = np.ascontiguousarray(r.case("max", size, form)[0][0])  # q - 1 everywhere: the largest addend
            d_a, d_p = [g.upload(x) for x in a[:17]], [g.upload(x) for x in p[:17]]
            d_add, d_o = g.upload(addend), g.alloc(addend.nbytes)
            try:
                for K in (1, 4, 8, 9, 17):
                    want = np.stack([o.add(addend[i], per_ct[K][i]) for i in range(COUNT)])
                    ca, cp = [x.ptr for x in d_a[:K]], [x.ptr for x in d_p[:K]]
                    _fill(g, d_o, np.full(addend.shape, SENTINEL, dtype=np.uint64))
                    _call(g, ca, form, cp, L * n, d_add.ptr, d_o.ptr, size, COUNT)
                    _same("size %d K=%d separate addend" % (size, K), g.download(d_o, want.shape), want)
                    _same("the addend is left alone", g.download(d_add, addend.shape), addend)
                    _fill(g, d_o, addend)
                    _call(g, ca, form, cp, L * n, d_o.ptr, d_o.ptr, size, COUNT)
                    _same("size %d K=%d d_out is d_addend" % (size, K), g.download(d_o, want.shape), want)
            finally:
                for x in d_a + d_p + [d_add, d_o]:
                    x.free()


@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_FUSED": "1"}], ids=["fused", "ntt_domain"])
def test_repeated_pointers_and_sub_ranges_of_one_allocation(rigs, env):
    r = rigs("40-40-50")
    g, o, n, L, size = r.g, r.o, r.n, r.L, 2
    a, p, _, _ = r.case("random", size, spec.COEFF)
    ref = lambda cts, pls, addend=None: np.stack([spec.multiply_plain_sum(o, [c[i] for c in cts], [q[i] for q in pls],  # noqa: E731
                                                                          addend=None if addend is None else addend[i]) for i in range(COUNT)])
    x, y, pa, pb = a[0], a[1], p[0], p[1]
    with _env(g, env):
        _same("a ciphertext in two terms", g.bfv_multiply_plain_sum([x, x, y], [pa, pb, pa]), ref([x, x, y], [pa, pb, pa]))
        _same("a pair twice", g.bfv_multiply_plain_sum([x, y, x], [pa, pb, pa]), ref([x, y, x], [pa, pb, pa]))
        ct_words, pl_words = x.size, pa.size
        block = np.concatenate([x.ravel(), y.ravel(), pa.ravel(), pb.ravel(), a[2].ravel(), np.full(ct_words, SENTINEL, dtype=np.uint64)])
        d = g.upload(block)
        try:
            at = lambda w: C.c_void_p(d.ptr.value + 8 * w)  # noqa: E731
            o_pl, o_add, o_out = 2 * ct_words, 2 * ct_words + 2 * pl_words, 3 * ct_words + 2 * pl_words
            _call(g, [at(0), at(ct_words)], spec.COEFF, [at(o_pl), at(o_pl + pl_words)], L * n, at(o_add), at(o_out), size, COUNT)
            back = g.download(d, block.shape)
            _same("sub-ranges of one allocation", back[o_out:].reshape(a[2].shape), ref([x, y], [pa, pb], addend=a[2]))
            _same("... and nothing else written", back[:o_out], block[:o_out])
        finally:
            d.free()


def test_no_terms_and_no_ciphertexts(rigs):
    r = rigs("40-40-50")
    g, n, L = r.g, r.n, r.L
    for size in (2, 3):
        a, p, _, _ = r.case("random", size, spec.COEFF)
        shp = (COUNT, size, L, n)
        sentinel = np.full(shp, SENTINEL, dtype=np.uint64)
        d_o, d_a, d_p = g.upload(sentinel), g.upload(a[0]), g.upload(p[0])
        try:
            _call(g, [], 0, [], 0, None, d_o.ptr, size, COUNT)
            assert not g.download(d_o, shp).any(), "an empty sum without an addend is zero"
            _fill(g, d_o, sentinel)
            _call(g, [], 1, [], 0, d_a.ptr, d_o.ptr, size, COUNT)
            _same("an empty sum is the addend", g.download(d_o, shp), a[0])
            _call(g, [], 0, [], 0, d_o.ptr, d_o.ptr, size, COUNT)
            _same("... also in place", g.download(d_o, shp), a[0])
            _fill(g, d_o, sentinel)
            _call(g, [d_a.ptr], 0, [d_p.ptr], 0, d_a.ptr, d_o.ptr, size, 0)
            g.sync()
            _same("count = 0 writes nothing", g.download(d_o, shp), sentinel)
        finally:
            for x in (d_o, d_a, d_p):
                x.free()
    _same("the convenience form of an empty sum", g.bfv_multiply_plain_sum([], [], size=3, count=2), np.zeros((2, 3, L, n), dtype=np.uint64))


# ---- refused calls: nothing written, the context still works ----
def test_refused_calls(rigs, capi):
    r = rigs("40-40-50")
    g, n, L, size = r.g, r.n, r.L, 2
    a, p, per_ct, _ = r.case("random", size, spec.COEFF)
    d_a, d_p = [g.upload(x) for x in a[:2]], [g.upload(x) for x in p[:2]]
    sentinel = np.full((COUNT, size, L, n), SENTINEL, dtype=np.uint64)
    d_o, d_add = g.upload(sentinel), g.upload(a[2])
    held = g.held_buffers()
    ca, cp = [x.ptr for x in d_a], [x.ptr for x in d_p]
    words, plain_words = COUNT * size * L * n, COUNT * L * n

    def call(cts=ca, pls=cp, stride=L * n, addend=None, out=None, sz=size, form=0, k=None):
        _call(g, cts, form, pls, stride, addend, out or d_o.ptr, sz, COUNT, n_terms=k)

    with pytest.raises(capi.AbcHipError, match="bad term list"):
        call(k=-1)
    with pytest.raises(capi.AbcHipError, match="null term pointer"):
        call(cts=[ca[0], None])
    with pytest.raises(capi.AbcHipError, match="null term pointer"):
        call(pls=[None, cp[1]])
    for sz in (1, 4, 0):
        with pytest.raises(capi.AbcHipError, match="size must be 2 or 3"):
            call(sz=sz)
    for stride in (1, n, L * n - 1, L * n + 1, 2 * L * n):
        with pytest.raises(capi.AbcHipError, match="plain_stride must be 0 or L"):
            call(stride=stride)
    for form in (2, -1):
        with pytest.raises(capi.AbcHipError, match="ct_form"):
            call(form=form)
    at = lambda buf, w: C.c_void_p(buf.ptr.value + 8 * w)  # noqa: E731
    for off in (1, words - 1):
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(cts=[ca[0], at(d_o, off)])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(pls=[at(d_o, 1), cp[1]])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_a[1], words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_p[0], plain_words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=ca[0])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(stride=0, out=at(d_p[1], L * n - 1))
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

    # a CKKS context refuses all three calls; the CKKS sum keeps refusing BFV (tests/test_gpu_plain_mac_sum.py)
    primes = capi.create_primes(n, [50, 40, 50])
    gc = capi.Context(capi.CKKS, n, primes)
    try:
        f_a, f_p = gc.upload(np.zeros((1, 2, 2, n), dtype=np.uint64)), gc.upload(np.zeros((2, n), dtype=np.uint64))
        f_o = gc.upload(np.full((1, 2, 2, n), SENTINEL, dtype=np.uint64))
        with pytest.raises(capi.AbcHipError, match="BFV only"):
            _call(gc, [f_a.ptr], 0, [f_p.ptr], 0, None, f_o.ptr, 2, 1)
        with pytest.raises(capi.AbcHipError, match="BFV only"):
            gc.op("bfv_plain_to_ntt", f_p.ptr, f_o.ptr, C.c_size_t(1))
        with pytest.raises(capi.AbcHipError, match="need BFV"):
            gc.route("bfv_plain_sum", 2)
        gc.sync()
        assert (gc.download(f_o, (1, 2, 2, n)) == SENTINEL).all()
    finally:
        gc.close()

    call()
    _same("after the refusals", g.download(d_o, sentinel.shape), per_ct[2])
    for x in d_a + d_p + [d_o, d_add]:
        x.free()


# ---- other rings: one case each, the route asserted ----
def _ring_case(om, capi, o, g, K, count, route):
    rng = np.random.default_rng(o.n + K)
    qs = o.primes[:o.L]
    a = np.stack([rng.integers(0, q, size=(K + 1, count, 2, o.n), dtype=np.uint64) for q in qs], axis=3)
    plains = rng.integers(0, o.t, size=(K, o.n), dtype=np.uint64)
    plains[0] = o.t - 1
    assert g.route("bfv_plain_sum", o.L, count) == route
    p_ntt = g.bfv_plain_to_ntt(plains)
    want = np.stack([o.add(a[K, i], spec.composed_sum(o, list(a[:K, i]), list(plains))) for i in range(count)])
    _same("N=%d K=%d" % (o.n, K), g.bfv_multiply_plain_sum(list(a[:K]), list(p_ntt), addend=a[K]), want)
    a_ntt = [g.ntt_limbs(x) for x in a[:K]]
    _same("N=%d K=%d, NTT-form terms" % (o.n, K), g.bfv_multiply_plain_sum(a_ntt, list(p_ntt), addend=a[K], ct_form=spec.NTT), want)


@pytest.mark.parametrize("n,count,route", [(4096, 2, "plainsum=fused"), (8192, 2, "plainsum=fused"), (16384, 3, "plainsum=ntt_domain"),
                                           (16384, 4, "plainsum=fused")], ids=["2^12", "2^13", "2^14-small", "2^14"])
def test_default_rings(oracle_mod, capi, n, count, route):
    o = oracle_mod.Oracle.bfv_default(n)
    g = capi.Context.bfv_default(n)
    try:
        _ring_case(oracle_mod, capi, o, g, 9, count, route)
    finally:
        g.close()


def _custom_ring(om, capi, n, route):
    """{40,40,50} on a ring without a default chain"""
    primes = om.create_primes(n, [40, 40, 50])
    t = om.plain_modulus_batching(n, 20)
    o = om.Oracle(om.BFV, n, primes, t)
    g = capi.Context(capi.BFV, n, o.primes, t)
    try:
        _ring_case(om, capi, o, g, 9, 2, route)
    finally:
        g.close()


def test_ring_2_15(oracle_mod, capi):
    _custom_ring(oracle_mod, capi, 32768, "plainsum=ntt_domain")


def test_ring_2_11(oracle_mod, capi):
    """the fused kernel's fifth instantiation, whose transform has another pass structure than its neighbours'"""
    _custom_ring(oracle_mod, capi, 2048, "plainsum=fused")


# ---- recorded circuits ----
@pytest.mark.parametrize("env,route", [({}, "plainsum=fused"), ({"ABC_HIP_NO_FUSED": "1"}, "plainsum=ntt_domain")], ids=["fused", "ntt_domain"])
@pytest.mark.parametrize("form", [spec.COEFF, spec.NTT], ids=["coeff", "ntt"])
def test_recorded_call_follows_its_inputs(rigs, env, route, form):
    """the call in a recording (eagerly once first: the arenas get their size), replayed twice on rewritten inputs; K = 9 is two launches"""
    r = rigs("40-40-50")
    g, o, n, L, size, K = r.g, r.o, r.n, r.L, 2, 9
    a, p, _, _ = r.case("random", size, form)
    with _env(g, env):
        assert g.route("bfv_plain_sum", L, COUNT) == route
        d_a, d_p = [g.upload(x) for x in a[:K]], [g.upload(x) for x in p[:K]]
        d_add, d_o = g.upload(a[K]), g.alloc(a[K].nbytes)

        def circuit():
            _call(g, [x.ptr for x in d_a], form, [x.ptr for x in d_p], L * n, d_add.ptr, d_o.ptr, size, COUNT)

        circuit()
        g.sync()
        held = g.held_buffers()
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
                want = np.stack([spec.multiply_plain_sum(o, list(a2[:K, i]), list(p2[:, i]), addend=a2[K, i], ct_form=form) for i in range(COUNT)])
                _same("turn %d" % turn, g.download(d_o, want.shape), want)
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for x in d_a + d_p + [d_add, d_o]:
            x.free()
