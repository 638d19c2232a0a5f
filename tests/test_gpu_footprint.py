"""Every base call of the C ABI held to its footprint, on poisoned memory.

The parity tests ask whether the downloaded output equals the oracle's.  That can be right by luck: abc_hip_malloc recycles blocks
by exact size and the scratch arenas keep their contents, so a kernel that skips part of its output, or reads a half-done limb it
never wrote, can find a previous call's words there; and a write past the output, in front of it or into an operand lands where
nobody looks.  Here contexts are created under ABC_HIP_POISON=1 (recycled blocks and arenas hold 0xFF bytes), ABC_HIP_CHUNK=2 and
ABC_HIP_LANES=2 / 1, and every call runs inside a footprint.Frame: operands, plaintexts and output in one allocation, separated by
sentinel zones.  Per call:
  * the output equals the oracle's call word for word, and no sentinel survives in it;
  * every zone is intact, and so is every operand and plaintext of an out-of-place call;
  * in place (the forms the header and the existing tests establish) the zones and the other operand are intact;
and once per context, at the end, the relinearisation key and every Galois key used read back as loaded.

One context per kernel sequence, at the smallest shape that selects it, the route string asserted: the seven cases of
test_gpu_ks_operand_slices.py, lds_fp's chain under ABC_HIP_NO_FUSED=1 (generic), BFVDefault(4096) (generic mul=behz),
BFVDefault(8192) (bmul) and the smallest N = 2^15 BFV chain that multiplies through bmul_big.  Inputs are residues
(fuzz_parity.random_ct), three ciphertexts -- a chunk of two and a ragged chunk of one -- and one.

The two references that are not the oracle's call, and why: abc_hip_ckks_encode is compared with tests/ckks_codec_spec.py's exact
integers on inputs whose every coefficient is further from a tie than the spec's margin (the oracle's fp64 encoder cannot decide a
rounding: test_gpu_ckks_codec.py); abc_hip_ckks_decode, floating point on both sides and no bit-parity target for the same reason,
is compared word for word with the same call outside the frame, which test_gpu_ckks_codec_exact.py holds to the exact reference.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_codec_spec as codec  # noqa: E402
import footprint as fp  # noqa: E402
from fuzz_parity import random_ct  # noqa: E402
from test_gpu_ks_operand_slices import CASES as KS_CASES  # noqa: E402

pytestmark = pytest.mark.gpu

COUNT = 3
KEYED_STEP, NAF_STEP = 1, 7  # 7 = 8 - 1: two hops through an arena
# name: (scheme, N, prime widths or None for BFVDefault(N), further switches, {route op: string})
CONTEXTS = {name: (scheme, n, bits, {}, {"relinearize": route}) for name, (scheme, n, bits, route) in KS_CASES.items()}
CONTEXTS.update({
    "generic": ("ckks", 1 << 12, KS_CASES["lds_fp"][2], {"ABC_HIP_NO_FUSED": "1"},
                {"relinearize": "generic front=plain", "mul_relin": "generic mul=tensor ks=generic front=plain"}),
    "bfv4096": ("bfv", 1 << 12, None, {}, {"mul_relin": "generic mul=behz ks=lds_fp", "multiply": "behz"}),
    "bfv8192": ("bfv", 1 << 13, None, {}, {"mul_relin": "bmul", "multiply": "bmul_big", "relinearize": "bsplit_big"}),
    "bfv32768": ("bfv", 1 << 15, [49] * 8 + [50], {}, {"mul_relin": "generic mul=bmul_big ks=bsplit_big", "multiply": "bmul_big"}),
})
RUNS = [(2, 3), (1, 3), (2, 1)]  # (ABC_HIP_LANES, count)
SWITCHES = ("ABC_HIP_POISON", "ABC_HIP_CHUNK", "ABC_HIP_LANES", "ABC_HIP_NO_FUSED")
SCALE = 2.0 ** 20


class World:
    """one context's oracle, keys, inputs and -- computed once, on first use, for all COUNT rows -- expected outputs"""

    def __init__(self, name, om):
        scheme, n, bits, _, _ = CONTEXTS[name]
        self.name, self.n, self.bfv = name, n, scheme == "bfv"
        primes = om.default_bfv_primes(n) if bits is None else om.create_primes(n, bits)
        self.t = om.plain_modulus_batching(n, 20) if self.bfv else 0
        self.o = o = om.Oracle(om.BFV, n, primes, self.t) if self.bfv else om.Oracle(om.CKKS, n, primes)
        self.primes, self.L = [int(p) for p in primes], o.L
        self.conj = 2 * n - 1
        self.elts = [o.elt_from_step(s) for s in (KEYED_STEP, 8, -1)] + [self.conj]
        o.keygen(0xF0070000 + sorted(CONTEXTS).index(name), elts=self.elts)
        self.keys = {"sk": o.secret_key(), "pk": o.public_key(), "relin": o.relin_key(), "galois": {e: o.galois_key(e) for e in self.elts}}
        self.levels = [self.L] if self.bfv or self.L == 1 else [self.L, 1]
        self.rng = np.random.default_rng(n + len(name))
        self._in, self._ref = {}, {}

    def ct(self, tag, nl, size=2):
        """input ciphertexts [COUNT][size][nl][N] of residues; one draw per (tag, nl, size)"""
        return self.input((tag, nl, size), lambda: random_ct(self.rng, self.primes, nl, self.n, COUNT, size))

    def input(self, key, make):
        if key not in self._in:
            self._in[key] = np.ascontiguousarray(make())
            self._in[key].setflags(write=False)
        return self._in[key]

    def ref(self, key, make):
        if key not in self._ref:
            self._ref[key] = np.ascontiguousarray(make())
            self._ref[key].setflags(write=False)
        return self._ref[key]

    def rows(self, key, f, *operands):
        """f applied to row i of every operand, for all COUNT rows"""
        return self.ref(key, lambda: np.stack([f(*[x[i] for x in operands]) for i in range(COUNT)]))


@pytest.fixture(scope="module")
def worlds(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = World(name, oracle_mod)
        return cache[name]
    return get


def _context(capi, W, lanes, monkeypatch):
    scheme, n, _, extra, _ = CONTEXTS[W.name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ABC_HIP_POISON", "1")  # all read when the context is created
    monkeypatch.setenv("ABC_HIP_CHUNK", "2")
    monkeypatch.setenv("ABC_HIP_LANES", str(lanes))
    for k, v in extra.items():
        monkeypatch.setenv(k, v)
    g = capi.Context(capi.BFV, n, W.primes, W.t) if scheme == "bfv" else capi.Context(capi.CKKS, n, W.primes)
    g.load_keys(**W.keys)
    return g


class Runner:
    """runs one call inside a Frame and collects everything that is wrong with it"""

    def __init__(self, g, W, count):
        self.g, self.W, self.count, self.problems, self.calls = g, W, count, [], 0

    def __call__(self, label, op, parts, args, written, expect, zone_shapes=None, host_expect=None):
        """parts: [(name, array or word count)]; args: the call's arguments after the context, a part's name standing for its
        pointer; written: the parts the call may write; expect: {part: array}, compared word for word"""
        W = self.W
        shapes = [np.shape(v) for _, v in parts if isinstance(v, np.ndarray)] if zone_shapes is None else zone_shapes
        frame = fp.Frame(self.g, parts, fp.zone_words_for(W.n, *shapes))
        try:
            names = dict(parts)
            self.g.op(op, *[frame.ptr(a) if isinstance(a, str) and a in names else a for a in args])
            res = frame.check(written=written)
        finally:
            frame.close()
        self.calls += 1
        where = "%s %s count=%d" % (W.name, label, self.count)
        for name, (cnt, first) in res.changed.items():
            kind = "operand" if name in frame.parts else "zone (%s)" % self._neighbours(frame, name)
            self.problems.append("%s: %s %s changed: %d words, first at offset %d" % (where, kind, name, cnt, first))
        for name, (cnt, first) in res.unwritten.items():
            self.problems.append("%s: %d words of %s still hold the sentinel, first at offset %d" % (where, cnt, name, first))
        for name, want in expect.items():
            want = np.ascontiguousarray(want)
            assert want.dtype.itemsize == 8 and want.size == frame.parts[name][1], "%s: the reference of %s has another shape" % (where, name)
            bad = np.flatnonzero(res.part(name) != want.reshape(-1).view(np.uint64))  # bit for bit, doubles included
            if len(bad):
                self.problems.append("%s: %s differs from the reference in %d/%d words, first at %d" % (where, name, len(bad), want.size, bad[0]))
        if host_expect is not None and not np.array_equal(*host_expect):
            self.problems.append("%s: host output %s, want %s" % (where, host_expect[0], host_expect[1]))

    @staticmethod
    def _neighbours(frame, zone):
        k = int(zone[4:])
        return "behind %s" % frame.order[k - 1] if k else "in front of %s" % frame.order[0]


def _words(o, coeffs, nl):
    """integer coefficients (|c| < 2^63) -> NTT-form words of limbs 0 .. nl-1"""
    c = np.array([int(x) for x in coeffs], dtype=np.int64)
    return np.stack([o.ntt(j, np.mod(c, np.int64(o.primes[j])).astype(np.uint64)) for j in range(nl)])


def _ciphertext_calls(run, W, cnt):
    o, n, sz = W.o, W.n, C.c_size_t(cnt)
    for nl in W.levels:
        tag = "nl=%d" % nl
        for size in (2, 3):
            a, b = W.ct("a", nl, size), W.ct("b", nl, size)
            for op in ("add", "sub"):
                want = W.rows((op, nl, size), getattr(o, op), a, b)[:cnt]
                run("%s size=%d %s" % (op, size, tag), op, [("a", a[:cnt]), ("b", b[:cnt]), ("out", a[:cnt].size)],
                    ("a", "b", "out", size, nl, sz), {"out"}, {"out": want})
                if size == 2:
                    for dst in ("a", "b"):
                        run("%s %s out=%s" % (op, tag, dst), op, [("a", a[:cnt]), ("b", b[:cnt])], ("a", "b", dst, size, nl, sz), {dst}, {dst: want})
            want = W.rows(("negate", nl, size), o.negate, a)[:cnt]
            run("negate size=%d %s" % (size, tag), "negate", [("a", a[:cnt]), ("out", a[:cnt].size)], ("a", "out", size, nl, sz), {"out"}, {"out": want})
            if size == 2:
                run("negate %s out=a" % tag, "negate", [("a", a[:cnt])], ("a", "a", size, nl, sz), {"a"}, {"a": want})
            # decrypt
            want = W.rows(("decrypt", nl, size), o.decrypt, a)[:cnt]
            run("decrypt size=%d %s" % (size, tag), "decrypt", [("ct", a[:cnt]), ("out", want.size)], ("ct", size, nl, "out", sz), {"out"}, {"out": want})
            if not W.bfv and nl >= 2:
                for op in ("rescale", "mod_switch"):
                    want = W.rows((op, nl, size), getattr(o, op), a)[:cnt]
                    run("%s size=%d %s" % (op, size, tag), op, [("in", a[:cnt]), ("out", want.size)], ("in", "out", size, nl, sz), {"out"}, {"out": want})
            if W.bfv:
                want = W.ref(("noise_budget", size), lambda: np.array([o.noise_budget(r) for r in a], dtype=np.int32))[:cnt]
                got = np.full(cnt, -7, dtype=np.int32)
                run("noise_budget size=%d" % size, "noise_budget", [("ct", a[:cnt])], ("ct", size, nl, got.ctypes.data_as(C.POINTER(C.c_int)), sz), set(), {},
                    host_expect=(got, want))
        a, b, a3 = W.ct("a", nl), W.ct("b", nl), W.ct("a", nl, 3)
        ab = [("a", a[:cnt]), ("b", b[:cnt])]
        want3 = W.rows(("multiply", nl), o.multiply, a, b)[:cnt]
        run("multiply " + tag, "multiply", ab + [("out", want3.size)], ("a", "b", "out", nl, sz), {"out"}, {"out": want3})
        want = W.rows(("relinearize", nl), o.relinearize, a3)[:cnt]
        run("relinearize " + tag, "relinearize", [("ct3", a3[:cnt]), ("out", want.size)], ("ct3", "out", nl, sz), {"out"}, {"out": want})
        want = W.rows(("mul_relin", nl), o.mul_relin, a, b)[:cnt]
        run("mul_relin " + tag, "mul_relin", ab + [("out", want.size)], ("a", "b", "out", nl, sz), {"out"}, {"out": want})
        for dst in ("a", "b"):
            run("mul_relin %s out=%s" % (tag, dst), "mul_relin", ab, ("a", "b", dst, nl, sz), {dst}, {dst: want})
        for step in (KEYED_STEP, NAF_STEP):
            want = W.rows(("rotate", nl, step), lambda r: o.rotate(r, step), a)[:cnt]
            run("rotate %d %s" % (step, tag), "rotate", [("in", a[:cnt]), ("out", want.size)], ("in", "out", nl, step, sz), {"out"}, {"out": want})
            run("rotate %d %s out=in" % (step, tag), "rotate", [("in", a[:cnt])], ("in", "in", nl, step, sz), {"in"}, {"in": want})
        want = W.rows(("conj", nl), lambda r: o.apply_galois(r, W.conj), a)[:cnt]
        run("apply_galois(2N-1) " + tag, "apply_galois", [("in", a[:cnt]), ("out", want.size)], ("in", "out", nl, C.c_uint32(W.conj), sz), {"out"}, {"out": want})
        target = a3[:, 2]  # one polynomial per ciphertext
        want = W.rows(("keyswitch", nl), lambda r: o.keyswitch(r, W.keys["relin"]), target)[:cnt]
        run("keyswitch " + tag, "keyswitch", [("target", np.ascontiguousarray(target[:cnt])), ("out", want.size)],
            ("target", C.c_uint32(0), "out", nl, sz), {"out"}, {"out": want}, zone_shapes=[want.shape])
        # plaintext operations: broadcast and one plaintext per ciphertext
        pw = n if W.bfv else nl * n
        plains = W.input(("plain", nl), lambda: random_ct(W.rng, [W.t] if W.bfv else W.primes, 1 if W.bfv else nl, n, COUNT, size=1).reshape(COUNT, pw))
        for size in (2, 3):
            ct = W.ct("a", nl, size)
            for op in ("multiply_plain", "add_plain", "sub_plain"):
                for form, plain, stride, prow in (("bcast", plains[0], 0, lambda i: plains[0]), ("per", plains[:cnt], pw, lambda i: plains[i])):
                    shaped = (lambda p: p) if W.bfv else (lambda p: p.reshape(nl, n))
                    want = W.ref((op, nl, size, form), lambda: np.stack([getattr(o, op)(ct[i], shaped(prow(i))) for i in range(COUNT)]))[:cnt]
                    parts = [("ct", ct[:cnt]), ("plain", plain), ("out", want.size)]
                    run("%s size=%d %s %s" % (op, size, form, tag), op, parts, ("ct", "plain", C.c_size_t(stride), "out", size, nl, sz), {"out"}, {"out": want})
                    if size == 2:
                        run("%s %s %s out=ct" % (op, form, tag), op, parts[:2], ("ct", "plain", C.c_size_t(stride), "ct", size, nl, sz), {"ct"}, {"ct": want},
                            zone_shapes=[ct.shape])


def _codec_and_transform_calls(run, W, cnt, g):
    o, n, L, sz = W.o, W.n, W.L, C.c_size_t(cnt)
    # seeded encrypt of three different plaintexts: ciphertext i draws from stream seed + i
    per = (n,) if W.bfv else (L, n)
    plains = W.input("enc_plain", lambda: random_ct(W.rng, [W.t] if W.bfv else W.primes, 1 if W.bfv else L, n, COUNT, size=1).reshape((COUNT,) + per))
    want = W.ref("encrypt", lambda: np.stack([o.encrypt(plains[i], 77 + i) for i in range(COUNT)]))[:cnt]
    run("encrypt", "encrypt", [("plain", plains[:cnt]), ("out", want.size)], ("plain", C.c_uint64(77), "out", sz), {"out"}, {"out": want}, zone_shapes=[want.shape])
    # the stand-alone transforms, in place: the data part is the only one written
    polys = W.input("ntt_in", lambda: random_ct(W.rng, W.primes, L, n, COUNT, size=2))
    for inverse in (0, 1):
        f = o.intt if inverse else o.ntt
        want = W.ref(("ntt_limbs", inverse), lambda: np.stack([[[f(j, polys[i, p, j]) for j in range(L)] for p in range(2)] for i in range(COUNT)]))[:cnt]
        run("ntt_limbs inverse=%d" % inverse, "ntt_limbs", [("data", polys[:cnt])], ("data", L, C.c_size_t(2 * cnt), inverse), {"data"}, {"data": want})
        j = L - 1  # one key-level prime, `2 * cnt` polynomials
        want = W.ref(("ntt", inverse), lambda: np.stack([[f(j, polys[i, p, j]) for p in range(2)] for i in range(COUNT)]))[:cnt]
        run("ntt_%s" % ("inverse" if inverse else "forward"), "ntt_inverse" if inverse else "ntt_forward",
            [("data", np.ascontiguousarray(polys[:cnt, :, j]))], ("data", 0, j, C.c_size_t(2 * cnt)), {"data"}, {"data": want}, zone_shapes=[(1, 2 * n)])
    if W.bfv:
        values = W.input("slots", lambda: W.rng.integers(-(W.t // 2), W.t // 2, size=(COUNT, n), dtype=np.int64))
        plain = W.rows("batch_encode", o.encode, values)[:cnt]
        run("batch_encode", "batch_encode", [("values", values[:cnt]), ("out", plain.size)], ("values", "out", sz), {"out"}, {"out": plain})
        back = W.rows("batch_decode", o.decode, W.rows("batch_encode", o.encode, values))[:cnt]
        run("batch_decode", "batch_decode", [("plain", plain), ("out", back.size)], ("plain", "out", sz), {"out"}, {"out": back})
        return
    # CKKS codec, a short row: complex, real, complex (one im array: the real row's is zero)
    logn = n.bit_length() - 1
    cases = [codec.encode_case_reference(logn, cplx, True, 20) for cplx in (True, False, True)]
    for v, _, dist in cases:
        assert dist.min() > codec.encode_margin(logn, 20), "an input of the encode case sits too close to a tie for an exact reference"
    values = np.stack([np.asarray(v, dtype=np.complex128) for v, _, _ in cases])
    values[2] = values[2].conj()  # a third row of its own: the conjugate slots encode the mirrored polynomial, as far from a tie
    re, im = np.ascontiguousarray(values.real[:cnt]), np.ascontiguousarray(values.imag[:cnt])

    def third():
        r, _, d = codec.encode_exact(values[2], SCALE, n, [])
        assert d.min() > codec.encode_margin(logn, 20), "the conjugated row sits too close to a tie for an exact reference"
        return np.array([int(x) for x in r], dtype=np.int64)
    ints = [cases[0][1], cases[1][1], W.ref("ckks_encode third row", third)]
    for nl in W.levels:
        want = W.ref(("ckks_encode", nl), lambda: np.stack([_words(o, c, nl) for c in ints]))[:cnt]
        run("ckks_encode nl=%d" % nl, "ckks_encode", [("re", re), ("im", im), ("out", want.size)],
            ("re", "im", C.c_size_t(values.shape[1]), C.c_double(SCALE), nl, "out", sz), {"out"}, {"out": want}, zone_shapes=[want.shape])
        plain = W.ct("a", nl)[:, 0]  # random residues [COUNT][nl][N]
        dec = g.ckks_decode(np.ascontiguousarray(plain[:cnt]), SCALE)  # the same call outside the frame (module docstring)
        run("ckks_decode nl=%d" % nl, "ckks_decode", [("plain", np.ascontiguousarray(plain[:cnt])), ("re", cnt * n // 2), ("im", cnt * n // 2)],
            ("plain", nl, C.c_double(SCALE), "re", "im", sz), {"re", "im"},
            {"re": np.ascontiguousarray(dec.real), "im": np.ascontiguousarray(dec.imag)}, zone_shapes=[(1, nl * n)])


@pytest.mark.parametrize("lanes,count", RUNS, ids=["lanes%d-count%d" % r for r in RUNS])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_base_calls_keep_to_their_footprint(name, lanes, count, worlds, capi, monkeypatch):
    W = worlds(name)
    g = _context(capi, W, lanes, monkeypatch)
    try:
        for op, route in CONTEXTS[name][4].items():
            assert g.route(op, W.L, COUNT) == route, "%s: %s takes another sequence" % (name, op)
        run = Runner(g, W, count)
        _ciphertext_calls(run, W, count)
        _codec_and_transform_calls(run, W, count, g)
        # the keys the calls above read are the words that were loaded
        if not np.array_equal(g.get_key("relin"), W.keys["relin"]):
            run.problems.append("%s: the relinearisation key changed" % name)
        for e in W.elts:
            if not np.array_equal(g.get_key("galois", e), W.keys["galois"][e]):
                run.problems.append("%s: the Galois key of element %d changed" % (name, e))
        print("%s lanes=%d count=%d: %d framed calls" % (name, lanes, count, run.calls))
        assert not run.problems, "%d problems:\n%s" % (len(run.problems), "\n".join(run.problems[:40]))
    finally:
        g.close()


# ---- the frame and the switch themselves, on the device ----
@pytest.fixture
def small(capi, monkeypatch):
    made = []

    def make(poison):
        monkeypatch.delenv("ABC_HIP_POISON", raising=False)
        if poison:
            monkeypatch.setenv("ABC_HIP_POISON", "1")
        n = 1 << 12
        made.append(capi.Context(capi.CKKS, n, capi.create_primes(n, [40, 40, 40])))
        return made[-1]
    yield make
    for g in made:
        g.close()


def test_frame_reports_a_copy_one_word_too_long(small):
    """abc_hip_memcpy_d2d of out_words + 1 words into the output part trips exactly the first word of the zone behind it"""
    g = small(True)
    words = 2 * 4096
    src = np.arange(words + 2, dtype=np.uint64)
    frame = fp.Frame(g, [("src", src), ("out", words)], 2 * 4096)
    try:
        g.op("memcpy_d2d", frame.ptr("out"), frame.ptr("src"), C.c_size_t((words + 1) * 8))
        res = frame.check(written={"out"})
    finally:
        frame.close()
    assert res.changed == {frame.zone_after("out"): (1, 0)} and res.unwritten == {}
    assert np.array_equal(res.part("out"), src[:words])


def test_poison_fills_fresh_and_recycled_blocks(small):
    g = small(True)
    nbytes = 3 * 4096 * 8 + 8  # a size no other call of this context asks for: the second alloc below is a cache hit
    poison = np.full(nbytes // 8, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    buf = g.alloc(nbytes)
    assert np.array_equal(g.download(buf, poison.shape), poison), "a fresh block is not poisoned"
    ptr = buf.ptr.value
    g.op("memcpy_h2d", buf.ptr, np.zeros_like(poison).ctypes.data_as(C.c_void_p), C.c_size_t(nbytes))
    assert not g.download(buf, poison.shape).any()
    buf.free()
    again = g.alloc(nbytes)
    try:
        assert again.ptr.value == ptr, "the block was not recycled: the check below would not be of a cache hit"
        assert np.array_equal(g.download(again, poison.shape), poison), "a recycled block is not poisoned"
    finally:
        again.free()


def test_poison_leaves_eager_and_recorded_results_alone(small, capi):
    """a rotation through an arena gives the words it gives with the switch off, eagerly (the arena poisoned when the call begins)
    and replayed from a recording made while the switch is on"""
    g_on, g_off = small(True), small(False)
    rng = np.random.default_rng(3)
    x = random_ct(rng, g_on.primes, 2, 4096, 3)
    for g in (g_on, g_off):
        g.keygen(5)
    want = g_off.rotate(x, NAF_STEP)
    assert np.array_equal(g_on.rotate(x, NAF_STEP), want)  # through an arena, poisoned when the call begins
    xb, out = g_on.upload(x), g_on.alloc(x.nbytes)
    try:
        g_on.op("rotate", xb.ptr, out.ptr, 2, NAF_STEP, C.c_size_t(3))  # the eager pass every recording needs
        g_on.graph_begin()
        g_on.op("rotate", xb.ptr, out.ptr, 2, NAF_STEP, C.c_size_t(3))
        graph = g_on.graph_end()
        g_on.op("memcpy_h2d", out.ptr, np.zeros_like(x).ctypes.data_as(C.c_void_p), C.c_size_t(x.nbytes))
        g_on.graph_launch(graph)
        assert np.array_equal(g_on.download(out, x.shape), want)
        g_on.graph_destroy(graph)
    finally:
        xb.free(); out.free()
