"""abc_hip_multiply_const_sum and abc_hip_multiply_const_sum_rescale on the device: (addend or 0) + const + sum over k of w_k * ct_k by
the K-term kernel k_ckks_const_mac_sum, each term read at its own level, or the composed sequence under ABC_HIP_NO_CONST_MAC_SUM.
Every comparison is word for word against tests/const_sum_spec.py: the CPU oracle's mod_switch, multiply_plain with the constant
plaintext, add and add_plain.

The kernel's decision points, from its constants (abc_kernels_eval.hip), all on both sides in TERMS below: kConstMacTerms = 8 terms
per launch (K = 8 | 9, 16 | 17, and 25 = three launches and a tail of one); the fp64 accumulators re-centred after kPlainMacFpTerms
= 4 terms of a launch (K = 4 | 5, and 12 | 13 in a second launch, which carries the first one's words by pointer); K = 0, the launch
that writes addend + constant; every K up to 9, the tail of the unrolled loop; the integer accumulator at 60-bit residues."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import const_sum_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TERMS = list(range(0, 10)) + [12, 13, 16, 17, 25]
FP_CHAIN, MIXED_CHAIN, WIDE_CHAIN = [50, 40, 40, 50], [60, 40, 40, 60], [60, 60, 60]
SPAN = 512  # coefficients of one limb a workgroup of the kernel owns
u64p = C.POINTER(C.c_uint64)


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


def _call(g, ct_ptrs, ct_nl, weights, const, addend, out, size, nl, count, n_terms=None, rescale=False):
    """the raw call: weights [K][nl] and const [nl] as they are (no shape is checked here: the refusals are the library's)"""
    k = len(ct_ptrs) if n_terms is None else n_terms
    w = np.ascontiguousarray(weights if weights is not None and len(ct_ptrs) else np.zeros(16), dtype=np.uint64).ravel()
    cst = None if const is None else np.ascontiguousarray(const, dtype=np.uint64)
    levels = None if ct_nl is None else (C.c_int * max(len(ct_nl), 1))(*[int(x) for x in ct_nl])
    g.op("multiply_const_sum_rescale" if rescale else "multiply_const_sum", g.term_pointers(ct_ptrs), levels, w.ctypes.data_as(u64p), k,
         None if cst is None else cst.ctypes.data_as(u64p), addend, out, size, nl, C.c_size_t(count))


def _fill(g, buf, arr):
    arr = np.ascontiguousarray(arr)
    g.op("memcpy_h2d", buf.ptr, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes))


def _data(kind, rng, primes, nl, size, terms, count, n):
    """(cts [terms][count][size][nl][N], weights [terms][nl], const [nl])"""
    qs = np.array(primes[:nl], dtype=np.uint64)
    if kind == "random":
        a = np.stack([rng.integers(0, q, size=(terms, count, size, n), dtype=np.uint64) for q in primes[:nl]], axis=3)
        w = np.stack([rng.integers(0, q, size=terms, dtype=np.uint64) for q in primes[:nl]], axis=1)
        return a, w, np.array([rng.integers(0, q, dtype=np.uint64) for q in primes[:nl]], dtype=np.uint64)
    a = np.empty((terms, count, size, nl, n), dtype=np.uint64)
    if kind == "max":  # (q - 1)^2 in every product of every term, q - 1 carried and added: the largest sums there are
        a[:] = (qs - 1)[:, None]
        return a, np.tile(qs - 1, (terms, 1)), qs - 1
    # 0 / 1 / q-1 by coefficient index, shifted per term and ciphertext, q-1 at the ends of the ring and of a span; weights 0, 1, q-1
    idx = np.arange(n)
    vals = np.stack([np.zeros_like(qs), np.ones_like(qs), qs - 1])  # [3][nl]
    for k in range(terms):
        for r in range(count):
            a[k, r] = vals[(idx + k + r) % 3].T
    for s in (0, 1, SPAN - 1, SPAN, n - SPAN - 1, n - SPAN, n - 2, n - 1):
        a[..., s] = qs - 1
    w = np.stack([vals[(k + 2) % 3] for k in range(terms)])
    return a, w, np.ones_like(qs)


def _prefix_sums(o, a, w, ks):
    """{K: [count][size][nl][N]} for every K in ks: the spec's sum without constant and addend, added up once in term order"""
    count, size, nl = a.shape[1], a.shape[2], a.shape[3]
    want, acc = {}, [None] * count
    if 0 in ks:
        want[0] = np.zeros(a.shape[1:], dtype=np.uint64)
    for k in range(max(ks)):
        for r in range(count):
            acc[r] = spec.multiply_const_sum(o, [a[k, r]], [w[k]], addend=acc[r], size=size, nl=nl)
        if k + 1 in ks:
            want[k + 1] = np.stack(acc)
    return want


def _plus_const(o, cts, const):
    return np.stack([spec.multiply_const_sum(o, [], [], const=const, addend=c) for c in cts])


class Rig:
    """one oracle and one device context on a CKKS chain at N = 2^10, count 3; the references of every K, computed once per (data
    kind, level, size) and left unchanged"""

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
            a, w, cst = _data(kind, rng, self.primes, nl, size, max(TERMS), count, self.n)
            sums = _prefix_sums(self.o, a, w, set(TERMS))
            for x in list(sums.values()) + [a, w, cst]:
                x.setflags(write=False)
            self._cases[key] = (a, w, cst, sums)
        return self._cases[key]

    def check(self, tag, nl, sizes=(2, 3), kinds=("random", "max", "pattern"), ks=TERMS):
        g, n = self.g, self.n
        for size in sizes:
            for kind in kinds:
                a, w, cst, sums = self.case(kind, nl, size)
                count = a.shape[1]
                d_a = [g.upload(x) for x in a]
                d_o = g.upload(np.full((count, size, nl, n), SENTINEL, dtype=np.uint64))
                try:
                    for K in ks:
                        what = "%s nl=%d size=%d %s K=%d" % (tag, nl, size, kind, K)
                        _call(g, [x.ptr for x in d_a[:K]], None, w[:K], None, None, d_o.ptr, size, nl, count)
                        _same(what, g.download(d_o, sums[K].shape), sums[K])
                        if K in (0, 1, 4, 8, 9, 25):  # the constant rides on the first launch alone
                            _call(g, [x.ptr for x in d_a[:K]], [nl] * K, w[:K], cst, None, d_o.ptr, size, nl, count)
                            _same(what + " + const", g.download(d_o, sums[K].shape), _plus_const(self.o, sums[K], cst))
                    for d, h in zip(d_a, list(a)):
                        _same("an operand is left alone", g.download(d, h.shape), h)
                finally:
                    for x in d_a + [d_o]:
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
    rigs(FP_CHAIN).check("fp", nl)


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
def test_composed_route_gives_the_same_words(rigs, bits, nl):
    r = rigs(bits)
    with _env(r.g, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}):
        r.check("composed", nl, ks=[0, 1, 2, 5, 9])


# ---- terms held above nl ----
@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}], ids=["kernel", "composed"])
@pytest.mark.parametrize("bits", [FP_CHAIN, MIXED_CHAIN], ids=["fp", "mixed"])
def test_terms_one_and_two_levels_up_are_read_in_place(rigs, bits, env):
    """nl = 1 on a three-limb chain: terms at 3, 2 and 1 limbs mixed, eleven of them (two launches).  Against the spec, and against
    the device's own mod_switch + multiply_plain_sum on filled plaintexts"""
    r = rigs(bits)
    g, o, n, nl, count = r.g, r.o, r.n, 1, 3
    rng = np.random.default_rng(31)
    levels = [3, 1, 2, 1, 3, 3, 2, 1, 2, 3, 1]
    for size in (2, 3):
        cts = [np.stack([rng.integers(0, q, size=(count, size, n), dtype=np.uint64) for q in r.primes[:l]], axis=2) for l in levels]
        w = np.stack([rng.integers(0, q, size=len(levels), dtype=np.uint64) for q in r.primes[:nl]], axis=1)
        cst = np.array([r.primes[0] - 1], dtype=np.uint64)
        addend = np.ascontiguousarray(cts[1][::-1])
        want = np.stack([spec.multiply_const_sum(o, [c[i] for c in cts], w, const=cst, addend=addend[i], nl=nl) for i in range(count)])
        with _env(g, env):
            _same("size %d: the spec" % size, g.multiply_const_sum(cts, w, const=cst, addend=addend, nl=nl), want)
        # the device's own sequence: mod_switch down, the weights as filled plaintexts, multiply_plain_sum, add_plain
        low = []
        for c in cts:
            while c.shape[2] > nl:
                c = g.mod_switch(c)
            low.append(c)
        plains = [spec.const_plain(x, n) for x in w]
        own = g.add_plain(g.multiply_plain_sum(low, plains, addend=addend), spec.const_plain(cst, n))
        _same("size %d: mod_switch + multiply_plain_sum + add_plain on the device" % size, own, want)


# ---- constant, addend, operand forms ----
@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}], ids=["kernel", "composed"])
@pytest.mark.parametrize("bits,nl", [(FP_CHAIN, 3), (MIXED_CHAIN, 3), (FP_CHAIN, 1)], ids=["fp", "mixed", "fp-1"])
def test_constant_only_addend_only_and_the_output_as_its_addend(rigs, bits, nl, env):
    r = rigs(bits)
    g, o, n = r.g, r.o, r.n
    with _env(g, env):
        for size in (2, 3):
            a, w, cst, sums = r.case("random", nl, size)
            count = a.shape[1]
            addend = np.ascontiguousarray(r.case("max", nl, size)[0][0])  # q - 1 everywhere: the largest carried words
            big = r.case("max", nl, size)[2]
            d_a = [g.upload(x) for x in a[:17]]
            d_add, d_o = g.upload(addend), g.alloc(addend.nbytes)
            try:
                _fill(g, d_o, np.full(addend.shape, SENTINEL, dtype=np.uint64))
                _call(g, [], None, None, big, None, d_o.ptr, size, nl, count)
                got = g.download(d_o, addend.shape)
                assert not got[:, 1:].any() and (got[:, 0] == big[None, :, None]).all(), "the constant over zeros, component 0 only"
                _call(g, [], None, None, None, d_add.ptr, d_o.ptr, size, nl, count)
                _same("an empty sum is the addend", g.download(d_o, addend.shape), addend)
                _call(g, [], None, None, big, d_add.ptr, d_o.ptr, size, nl, count)
                _same("addend + constant", g.download(d_o, addend.shape), _plus_const(o, addend, big))
                for K in (1, 4, 5, 8, 9, 17):
                    want = _plus_const(o, np.stack([o.add(addend[i], sums[K][i]) for i in range(count)]), big)
                    ca = [x.ptr for x in d_a[:K]]
                    _fill(g, d_o, np.full(addend.shape, SENTINEL, dtype=np.uint64))
                    _call(g, ca, None, w[:K], big, d_add.ptr, d_o.ptr, size, nl, count)
                    _same("size %d K=%d separate addend" % (size, K), g.download(d_o, want.shape), want)
                    _same("the addend is left alone", g.download(d_add, addend.shape), addend)
                    _fill(g, d_o, addend)
                    _call(g, ca, None, w[:K], big, d_o.ptr, d_o.ptr, size, nl, count)
                    _same("size %d K=%d d_out is d_addend" % (size, K), g.download(d_o, want.shape), want)
            finally:
                for x in d_a + [d_add, d_o]:
                    x.free()


def test_one_pointer_in_two_terms_and_sub_ranges_of_one_allocation(rigs):
    r = rigs(FP_CHAIN)
    g, o, n, nl, size = r.g, r.o, r.n, 2, 2
    a, w, cst, _ = r.case("random", nl, size)
    count = a.shape[1]
    ref = lambda cts, ws, **kw: np.stack([spec.multiply_const_sum(o, [c[i] for c in cts], ws, nl=nl, **{k: (v[i] if k == "addend" else v) for k, v in kw.items()}) for i in range(count)])  # noqa: E731
    x, y = a[0], a[1]
    _same("a ciphertext in two terms", g.multiply_const_sum([x, x, y], w[:3]), ref([x, x, y], w[:3]))
    _same("... and three", g.multiply_const_sum([x, y, x, x], w[:4], const=cst), ref([x, y, x, x], w[:4], const=cst))
    _same("multiply_const is K = 1", g.multiply_const(x, 0.5, 2.0 ** 30), ref([x], [spec.const_words(o.primes, 0.5, 2.0 ** 30, nl)]))
    _same("add_const is K = 0", g.add_const(x, -1.25, 2.0 ** 40), _plus_const(o, x, spec.const_words(o.primes, -1.25, 2.0 ** 40, nl)))
    assert [int(v) for v in g.const_words(-1.25, 2.0 ** 40, nl)] == [int(v) for v in spec.const_words(o.primes, -1.25, 2.0 ** 40, nl)]
    # sub-ranges of one allocation: two terms, the addend and the output back to back
    words = x.size
    block = np.concatenate([x.ravel(), y.ravel(), a[2].ravel(), np.full(words, SENTINEL, dtype=np.uint64)])
    d = g.upload(block)
    try:
        at = lambda k: C.c_void_p(d.ptr.value + 8 * k)  # noqa: E731
        _call(g, [at(0), at(words)], None, w[:2], cst, at(2 * words), at(3 * words), size, nl, count)
        back = g.download(d, block.shape)
        _same("sub-ranges of one allocation", back[3 * words:].reshape(x.shape), ref([x, y], w[:2], const=cst, addend=a[2]))
        _same("... and nothing else written", back[:3 * words], block[:3 * words])
    finally:
        d.free()


def test_count_zero_and_the_convenience_form_of_an_empty_sum(rigs):
    r = rigs(FP_CHAIN)
    g, n, nl, size = r.g, r.n, 3, 2
    a, w, cst, _ = r.case("random", nl, size)
    shp = a[0].shape
    sentinel = np.full(shp, SENTINEL, dtype=np.uint64)
    d_o, d_a = g.upload(sentinel), g.upload(a[0])
    try:
        _call(g, [d_a.ptr], None, w[:1], cst, d_a.ptr, d_o.ptr, size, nl, 0)
        _call(g, [d_a.ptr], None, w[:1], cst, None, d_o.ptr, size, nl, 0, rescale=True)
        g.sync()
        _same("count = 0 writes nothing", g.download(d_o, shp), sentinel)
    finally:
        d_o.free(); d_a.free()
    _same("an empty sum", g.multiply_const_sum([], None, size=3, nl=2, count=2), np.zeros((2, 3, 2, n), dtype=np.uint64))


# ---- refused calls: nothing written, the context still works ----
def test_refused_calls(rigs, capi):
    r = rigs(FP_CHAIN)
    g, n, L, nl, size = r.g, r.n, r.L, 2, 2
    a, w, cst, sums = r.case("random", nl, size)
    count = a.shape[1]
    d_a = [g.upload(x) for x in a[:2]]
    sentinel = np.full((count, size, nl, n), SENTINEL, dtype=np.uint64)
    d_o, d_add = g.upload(sentinel), g.upload(a[2])
    held = g.held_buffers()
    ca = [x.ptr for x in d_a]
    words = count * size * nl * n
    q = r.primes

    def call(cts=ca, levels=None, ws=w[:2], const=None, addend=None, out=None, sz=size, level=nl, k=None, rescale=False):
        _call(g, cts, levels, ws, const, addend, out or d_o.ptr, sz, level, count, n_terms=k, rescale=rescale)

    for rs in (False, True):
        with pytest.raises(capi.AbcHipError, match="bad term list"):
            call(k=-1, rescale=rs)
        with pytest.raises(capi.AbcHipError, match="null term pointer"):
            call(cts=[ca[0], None], rescale=rs)
        for level in (0, L + 1, -1):
            with pytest.raises(capi.AbcHipError, match="limb count out of range"):
                call(level=level, ws=np.zeros((2, 16), dtype=np.uint64), rescale=rs)
        for sz in (1, 4, 0):
            with pytest.raises(capi.AbcHipError, match="size must be 2 or 3"):
                call(sz=sz, rescale=rs)
        for levels in ([nl, nl - 1], [L + 1, nl]):
            with pytest.raises(capi.AbcHipError, match="a term's limb count must be in nl .. L"):
                call(levels=levels, rescale=rs)
        bad_w = np.array(w[:2])
        bad_w[1, 1] = q[1]
        with pytest.raises(capi.AbcHipError, match="a weight word is not below its prime"):
            call(ws=bad_w, rescale=rs)
        with pytest.raises(capi.AbcHipError, match="a constant word is not below its prime"):
            call(const=np.array([0, 2 ** 64 - 1], dtype=np.uint64), rescale=rs)
    with pytest.raises(capi.AbcHipError, match="no limb left to drop"):
        call(level=1, ws=w[:2, :1], rescale=True)
    at = lambda buf, k: C.c_void_p(buf.ptr.value + 8 * k)  # noqa: E731
    # a term inside the output: on its first and on its last word; the output on a term's last word; a RAISED term's last limb
    for off in (1, words - 1):
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(cts=[ca[0], at(d_o, off)])
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=at(d_a[1], words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=ca[0])
    big = g.alloc(count * size * L * n * 8 + words * 8)  # a term at L limbs directly in front of the output
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(cts=[ca[0], big.ptr], levels=[nl, L], out=at(big, count * size * L * n - 1))
    call(cts=[ca[0], ca[1]], levels=[nl, nl], out=at(big, count * size * L * n))  # clear of it: accepted
    # the addend: exactly d_out or clear of it; the rescaled form takes no overlap at all
    for off in (1, words - 1):
        with pytest.raises(capi.AbcHipError, match="may be d_addend"):
            call(addend=at(d_o, off))
    with pytest.raises(capi.AbcHipError, match="may be d_addend"):
        call(addend=d_add.ptr, out=at(d_add, words - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap d_addend"):
        call(addend=d_o.ptr, rescale=True)
    with pytest.raises(capi.AbcHipError, match="must not overlap a ciphertext term"):
        call(out=ca[1], rescale=True)
    with pytest.raises(capi.AbcHipError, match="2\\^62"):
        g.const_words(1.0, 2.0 ** 62)
    with pytest.raises(capi.AbcHipError, match="not finite"):
        g.const_words(float("inf"), 1.0)
    with pytest.raises(capi.AbcHipError, match="limb count out of range"):
        g.const_words(1.0, 1.0, L + 1)
    g.sync()
    _same("refused calls wrote nothing", g.download(d_o, sentinel.shape), sentinel)
    for x, h in zip(d_a + [d_add], list(a[:2]) + [a[2]]):
        _same("... nor to an operand", g.download(x, h.shape), h)
    assert g.held_buffers() == held

    # a BFV context
    gb = capi.Context.bfv_default(4096)
    try:
        f_a = gb.upload(np.zeros((1, 2, gb.L, gb.n), dtype=np.uint64))
        f_o = gb.upload(np.full((1, 2, gb.L, gb.n), SENTINEL, dtype=np.uint64))
        for rs in (False, True):
            with pytest.raises(capi.AbcHipError, match="is a CKKS operation"):
                _call(gb, [f_a.ptr], None, np.zeros((1, gb.L), dtype=np.uint64), None, None, f_o.ptr, 2, gb.L, 1, rescale=rs)
        with pytest.raises(capi.AbcHipError, match="is a CKKS operation"):
            gb.const_words(1.0, 1.0)
        gb.sync()
        assert (gb.download(f_o, (1, 2, gb.L, gb.n)) == SENTINEL).all()
    finally:
        gb.close()

    # and the context still works
    call()
    _same("after the refusals", g.download(d_o, sentinel.shape), sums[2])
    for x in d_a + [d_o, d_add, big]:
        x.free()


# ---- other rings ----
@pytest.mark.parametrize("n,bits,nl,K", [(16384, [50, 40, 40, 40, 50], 3, 9), (32768, FP_CHAIN, 2, 5)], ids=["2^14", "2^15"])
def test_other_rings(oracle_mod, capi, n, bits, nl, K):
    om = oracle_mod
    o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
    g = capi.Context(capi.CKKS, n, o.primes)
    try:
        rng = np.random.default_rng(n)
        a, w, cst = _data("random", rng, o.primes, nl + 1, 2, K, 2, n)  # every other term one level up
        cts = [a[k] if k % 2 else np.ascontiguousarray(a[k][:, :, :nl]) for k in range(K)]
        want = np.stack([spec.multiply_const_sum(o, [c[i] for c in cts], w[:, :nl], const=cst[:nl], addend=cts[0][i]) for i in range(2)])
        _same("N=%d nl=%d K=%d" % (n, nl, K), g.multiply_const_sum(cts, w[:, :nl], const=cst[:nl], addend=cts[0], nl=nl), want)
    finally:
        g.close()


# ---- recorded circuits ----
@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}], ids=["kernel", "composed"])
def test_recorded_call_follows_its_inputs(rigs, env):
    """the call in a recording (eagerly once first: the arenas get their size), replayed twice on rewritten inputs; K = 9 is two
    launches; the weights are part of the record"""
    r = rigs(FP_CHAIN)
    g, o, n, nl, size, K = r.g, r.o, r.n, 2, 2, 9
    a3, w3, cst3, _ = r.case("random", 3, size)
    a, w, cst = a3, np.ascontiguousarray(w3[:, :nl]), np.ascontiguousarray(cst3[:nl])
    count = a.shape[1]
    low = lambda x: np.ascontiguousarray(x[..., :nl, :])  # noqa: E731
    levels = [3 if k % 2 else nl for k in range(K)]
    with _env(g, env):
        d_a = [g.upload(a[k] if levels[k] == 3 else low(a[k])) for k in range(K)]
        d_add, d_o = g.upload(low(a[K])), g.alloc(low(a[K]).nbytes)
        held = g.held_buffers()

        def circuit():
            _call(g, [x.ptr for x in d_a], levels, w[:K], cst, d_add.ptr, d_o.ptr, size, nl, count)

        circuit()
        g.sync()
        g.graph_begin()
        circuit()
        exe = g.graph_end()
        try:
            for turn, order in enumerate(([0, 1, 2], [2, 0, 1], [1, 2, 0])):
                a2 = np.ascontiguousarray(a[:K + 1][::-1][:, order])
                hosts = [a2[k] if levels[k] == 3 else low(a2[k]) for k in range(K)] + [low(a2[K])]
                for d, h in zip(d_a + [d_add], hosts):
                    _fill(g, d, h)
                _fill(g, d_o, np.full(hosts[K].shape, SENTINEL, dtype=np.uint64))
                if turn:
                    g.graph_launch(exe)
                else:
                    circuit()
                want = np.stack([spec.multiply_const_sum(o, [h[i] for h in hosts[:K]], w[:K], const=cst, addend=hosts[K][i]) for i in range(count)])
                _same("turn %d" % turn, g.download(d_o, want.shape), want)
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for x in d_a + [d_add, d_o]:
            x.free()


# ---- the sum with one rescale ----
def _rescaled(o, cts):
    return np.stack([o.rescale(c) for c in cts])


@pytest.mark.parametrize("env", [{}, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}, {"ABC_HIP_NO_FUSED": "1"}, {"ABC_HIP_NO_ISPLIT": "1"}],
                         ids=["kernel", "composed", "no_fused", "no_isplit"])
@pytest.mark.parametrize("bits,nl", [(FP_CHAIN, 3), (FP_CHAIN, 2), (MIXED_CHAIN, 3), (WIDE_CHAIN, 2)], ids=["fp-3", "fp-2", "mixed-3", "wide-2"])
def test_rescaled_sum_is_the_sum_then_rescale(rigs, bits, nl, env):
    r = rigs(bits)
    g, o = r.g, r.o
    with _env(g, env):
        route = g.route("const_sum_rescale", nl, 3)
        assert route == g.route("rescale", nl, 3) + " constsum=separate"
        for size in (2, 3):
            a, w, cst, sums = r.case("random", nl, size)
            count = a.shape[1]
            for K in (0, 1, 2, 4, 5, 9):
                want = _rescaled(o, _plus_const(o, sums[K], cst))
                _same("%s size %d K=%d" % (route, size, K), g.multiply_const_sum_rescale(list(a[:K]), w[:K], const=cst, size=size, nl=nl, count=count), want)
            addend = np.ascontiguousarray(a[20])
            want = _rescaled(o, [o.add(addend[i], sums[3][i]) for i in range(count)])
            _same("with an addend", g.multiply_const_sum_rescale(list(a[:3]), w[:3], addend=addend), want)
            _same("the addend alone", g.multiply_const_sum_rescale([], None, addend=addend), _rescaled(o, addend))
            assert not g.multiply_const_sum_rescale([], None, size=size, nl=nl, count=2).any()
            # K = 1, nothing else: the words of multiply_plain_rescale with the constant plaintext
            _same("K = 1 is multiply_plain_rescale", g.multiply_const_sum_rescale([a[0]], w[:1]), g.multiply_plain_rescale(a[0], spec.const_plain(w[0], r.n)))


FUSED, SEPARATE = {"ABC_HIP_CONST_SUM_RESCALE_FUSED": "1"}, {"ABC_HIP_CONST_SUM_RESCALE_FUSED": "0"}


@pytest.mark.parametrize("bits,nl", [(FP_CHAIN, 3), (FP_CHAIN, 2), (MIXED_CHAIN, 3), (MIXED_CHAIN, 2), (WIDE_CHAIN, 2)], ids=["fp-3", "fp-2", "mixed-3", "mixed-2", "wide-2"])
def test_both_forced_routes_give_the_words_of_the_sum_then_rescale(rigs, bits, nl):
    """ABC_HIP_CONST_SUM_RESCALE_FUSED=1 / =0 at a batch of 3, route strings asserted: K = 1 .. 4 in the fused pair (fp64, mixed with the
    dropped limb on either arithmetic, all-integer), with and without constant and addend, sizes 2 and 3, every data kind; K = 5 and
    a term above nl are refused by the fused route -- they take the separate one, same words"""
    r = rigs(bits)
    g, o, n = r.g, r.o, r.n
    base = g.route("rescale", nl, 3)
    for env, tail in ((FUSED, " constsum=fused"), (SEPARATE, " constsum=separate")):
        with _env(g, env):
            assert g.route("const_sum_rescale", nl, 3) == base + tail
            for size in (2, 3):
                for kind in ("random", "max", "pattern"):
                    a, w, cst, sums = r.case(kind, nl, size)
                    count = a.shape[1]
                    addend = np.ascontiguousarray(a[20])
                    for K in (1, 2, 3, 4, 5):
                        what = "%s size %d %s K=%d" % (tail, size, kind, K)
                        _same(what, g.multiply_const_sum_rescale(list(a[:K]), w[:K]), _rescaled(o, sums[K]))
                        _same(what + " + const", g.multiply_const_sum_rescale(list(a[:K]), w[:K], const=cst), _rescaled(o, _plus_const(o, sums[K], cst)))
                        want = _rescaled(o, _plus_const(o, [o.add(addend[i], sums[K][i]) for i in range(count)], cst))
                        _same(what + " + addend + const", g.multiply_const_sum_rescale(list(a[:K]), w[:K], const=cst, addend=addend), want)
            # K = 1: the words of multiply_plain_rescale with the constant plaintext
            a, w, _, _ = r.case("random", nl, 2)
            _same("K = 1 is multiply_plain_rescale", g.multiply_const_sum_rescale([a[0]], w[:1]), g.multiply_plain_rescale(a[0], spec.const_plain(w[0], n)))
    if nl < r.L:  # a raised term: the fused route refuses it whatever the switch says
        rng = np.random.default_rng(5)
        up = np.stack([rng.integers(0, q, size=(3, 2, n), dtype=np.uint64) for q in r.primes[: nl + 1]], axis=2)
        a, w, cst, _ = r.case("random", nl, 2)
        want = np.stack([spec.multiply_const_sum_rescale(o, [a[0, i], up[i]], w[:2], const=cst, nl=nl) for i in range(3)])
        for env in (FUSED, SEPARATE, {}):
            with _env(g, env):
                _same("a raised term under %s" % env, g.multiply_const_sum_rescale([a[0], up], w[:2], const=cst, nl=nl), want)


@pytest.mark.parametrize("env", [{"ABC_HIP_NO_FUSED": "1"}, {"ABC_HIP_NO_ISPLIT": "1"}, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}], ids=["no_fused", "no_isplit", "no_const_mac_sum"])
def test_nothing_sends_a_call_to_the_fused_pair_where_it_cannot_run(rigs, env):
    """forced on, yet separate: the generic rescale (NO_FUSED; NO_ISPLIT on a chain with a 60-bit prime) and the composed sum"""
    for bits, nl in ((MIXED_CHAIN, 3), (FP_CHAIN, 3)):
        r = rigs(bits)
        g, o = r.g, r.o
        with _env(g, dict(env, **FUSED)):
            route = g.route("const_sum_rescale", nl, 512)
            fused_ok = env == {"ABC_HIP_NO_ISPLIT": "1"} and bits == FP_CHAIN  # no prime above 2^50: the switch does not apply
            assert route.endswith(" constsum=fused" if fused_ok else " constsum=separate"), route
            a, w, cst, sums = r.case("random", nl, 2)
            _same("%s %s" % (env, route), g.multiply_const_sum_rescale(list(a[:3]), w[:3], const=cst), _rescaled(o, _plus_const(o, sums[3], cst)))


def test_default_route_rule_on_a_batch_of_3_and_of_512(rigs):
    """the measured rule (abc_route.hpp, route_const_sum_rescale): at least 64 polynomials and 2^20 coefficients -- at N = 2^10 a batch of
    512 size-2 ciphertexts is exactly 2^20; terms above nl stay separate at either batch"""
    r = rigs(FP_CHAIN)
    g, o, n, nl = r.g, r.o, r.n, 2
    rng = np.random.default_rng(77)
    assert g.route("const_sum_rescale", nl, 3) == "fp constsum=separate" and g.route("const_sum_rescale", nl, 511) == "fp constsum=separate"
    assert g.route("const_sum_rescale", nl, 512) == "fp constsum=fused"
    for count in (3, 512):
        cts = [np.stack([rng.integers(0, q, size=(count, 2, n), dtype=np.uint64) for q in r.primes[:l]], axis=2) for l in (2, 2, 3)]
        w = np.stack([rng.integers(0, q, size=3, dtype=np.uint64) for q in r.primes[:nl]], axis=1)
        cst = np.array([rng.integers(0, q, dtype=np.uint64) for q in r.primes[:nl]], dtype=np.uint64)
        for terms in (2, 3):  # all at nl (fused at 512) / the third one level up (separate)
            got = g.multiply_const_sum_rescale(cts[:terms], w[:terms], const=cst, nl=nl)
            for i in (0, count // 2, count - 1):
                _same("count %d, %d terms, ciphertext %d" % (count, terms, i), got[i], spec.multiply_const_sum_rescale(o, [c[i] for c in cts[:terms]], w[:terms], const=cst, nl=nl))
            _same("count %d: the device's own sum and rescale" % count, got, g.rescale(g.multiply_const_sum(cts[:terms], w[:terms], const=cst, nl=nl)))


def test_recorded_fused_call_follows_its_inputs(rigs):
    r = rigs(MIXED_CHAIN)
    g, o, nl, size, K = r.g, r.o, 3, 2, 3
    a, w, cst, _ = r.case("random", nl, size)
    count = a.shape[1]
    with _env(g, FUSED):
        assert g.route("const_sum_rescale", nl, count).endswith(" constsum=fused")
        d_a = [g.upload(a[k]) for k in range(K)]
        d_add = g.upload(a[K])
        oshape = (count, size, nl - 1, r.n)
        d_o = g.alloc(int(np.prod(oshape)) * 8)
        held = g.held_buffers()

        def circuit():
            _call(g, [x.ptr for x in d_a], None, w[:K], cst, d_add.ptr, d_o.ptr, size, nl, count, rescale=True)

        circuit()
        g.sync()
        g.graph_begin()
        circuit()
        exe = g.graph_end()
        try:
            for turn, order in enumerate(([0, 1, 2], [2, 0, 1], [1, 2, 0])):
                a2 = np.ascontiguousarray(a[:K + 1][::-1][:, order])
                for d, h in zip(d_a + [d_add], list(a2)):
                    _fill(g, d, h)
                _fill(g, d_o, np.full(oshape, SENTINEL, dtype=np.uint64))
                if turn:
                    g.graph_launch(exe)
                else:
                    circuit()
                want = np.stack([spec.multiply_const_sum_rescale(o, list(a2[:K, i]), w[:K], const=cst, addend=a2[K, i]) for i in range(count)])
                _same("turn %d" % turn, g.download(d_o, oshape), want)
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for x in d_a + [d_add, d_o]:
            x.free()


@pytest.mark.parametrize("n,bits,nl", [(4096, FP_CHAIN, 3), (16384, [50, 40, 40, 40, 50], 4), (16384, [50, 40, 40, 40, 50], 2), (16384, [60, 40, 40, 60], 3),
                                       (32768, FP_CHAIN, 3)], ids=["2^12", "2^14-4", "2^14-2", "2^14-mixed", "2^15"])
def test_rescaled_sum_on_other_rings(oracle_mod, capi, n, bits, nl):
    """both forced routes on every ring with a fused pair; N = 2^15 has none: separate even when forced on"""
    om = oracle_mod
    o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
    g = capi.Context(capi.CKKS, n, o.primes)
    try:
        rng = np.random.default_rng(n + nl)
        a, w, cst = _data("random", rng, o.primes, nl, 2, 3, 2, n)
        want = np.stack([spec.multiply_const_sum_rescale(o, list(a[:, i]), w, const=cst) for i in range(2)])
        for env, tail in ((FUSED, " constsum=fused" if n < 32768 else " constsum=separate"), (SEPARATE, " constsum=separate")):
            with _env(g, env):
                assert g.route("const_sum_rescale", nl, 2).endswith(tail)
                _same("N=%d nl=%d%s" % (n, nl, tail), g.multiply_const_sum_rescale(list(a), w, const=cst), want)
    finally:
        g.close()
