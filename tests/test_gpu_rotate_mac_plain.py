"""Fused rotate, multiply-plain and add on the device (abc_hip_rotate_mac_plain / abc_hip_apply_galois_mac_plain /
abc_hip_diag_matvec): d_out = d_addend + d_plain (.) rotate(d_in), plaintext and addend being operands of the key switch's last kernel
where route("rotate_mac_plain") says "fold+mac", and a rotation into an arena, multiply_plain on it and the add kernel everywhere
else.  All three steps are exact modular arithmetic, so every comparison is word for word against
o.add(addend, o.multiply_plain(o.rotate(x, s), p)) / o.apply_galois, per row.  Rows: two of random residues and one of extremes (0, 1,
(q+-1)/2, q-2, q-1 and a quarter-ring run of q-1) in input, addend and plaintext at once, so acc + p r reaches (q-1) + (q-1)^2.
Plaintext forms: one for the batch, one per ciphertext nl * N apart, and rows of L limbs L * N apart at nl < L.  The oracle generates
Galois keys for the elements a test uses only; every fused shape asserts its route string, so a silent fall-back fails."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N14, N15 = 1 << 14, 1 << 15
CONJ = None  # as a step: the element 2N - 1 (conjugation)
SENTINEL = 0xDEADBEEFDEADBEEF
FORMS = ("bcast", "per", "wide")


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


def _random_poly(primes, nl, n, rng, polys):
    return np.stack([rng.integers(0, q, size=(polys, n), dtype=np.uint64) for q in primes[:nl]], axis=1)


def _extreme_poly(primes, nl, n, rng, polys):
    """residues from {0, 1, (q-1)/2, (q+1)/2, q-2, q-1} and random values, and a quarter-ring run of q-1 in every polynomial"""
    out = np.empty((polys, nl, n), dtype=np.uint64)
    for j in range(nl):
        q = primes[j]
        pool = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
        pick = rng.integers(0, 8, size=(polys, n))
        rnd = rng.integers(0, q, size=(polys, n), dtype=np.uint64)
        out[:, j, :] = np.where(pick < 6, pool[np.minimum(pick, 5)], rnd)
    out[:, :, : n // 4] = np.array(primes[:nl], dtype=np.uint64)[None, :, None] - 1
    return out


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


class Rig:
    """one CKKS oracle with Galois keys for `steps`, a device context with the same keys; at every level three inputs, three addends
    and three plaintexts (rows 0, 1 random, row 2 extremes in all three), and the references computed so far (shared by the tests of
    a module, never changed).  The broadcast plaintext is row 2, the extremes."""

    def __init__(self, om, capi, n, bits, steps, seed=0x3AC):
        primes = om.create_primes(n, bits)
        self.o = o = om.Oracle(om.CKKS, n, primes)
        self.n, self.primes = n, list(primes)
        o.keygen(seed, elts=sorted({self.elt(s) for s in steps if s != 0}))
        self.g = capi.Context(capi.CKKS, n, o.primes)
        self.g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
        self.L = L = o.L
        rng = np.random.default_rng(n + len(primes) + 1)
        mk = lambda polys: np.stack([_random_poly(primes, L, n, rng, polys), _random_poly(primes, L, n, rng, polys),  # noqa: E731
                                     _extreme_poly(primes, L, n, rng, polys)])
        self._in = {L: (mk(2), mk(2))}
        self.plain = mk(1)[:, 0]  # [3][L][N]: limb j modulo q_j at every level
        for v in self._in[L] + (self.plain,):
            v.setflags(write=False)
        self._rot, self._want = {}, {}

    def elt(self, s):
        return 2 * self.n - 1 if s is CONJ else self.o.elt_from_step(s)

    def inputs(self, level):
        """(x, a): [3][2][level][N] each"""
        if level not in self._in:
            x, a = self.inputs(level + 1)
            self._in[level] = tuple(np.stack([self.o.mod_switch(ct) for ct in v]) for v in (x, a))
            for v in self._in[level]:
                v.setflags(write=False)
        return self._in[level]

    def rot(self, level, s):
        """[3][2][level][N]: rotate(x[row], s), cached per (level, step)"""
        k = (level, s)
        if k not in self._rot:
            x, _ = self.inputs(level)
            o = self.o
            self._rot[k] = np.stack([x[r] if s == 0 else o.apply_galois(x[r], self.elt(CONJ)) if s is CONJ else o.rotate(x[r], s) for r in range(3)])
            self._rot[k].setflags(write=False)
        return self._rot[k]

    def want(self, level, s, form="per", addend="a"):
        """[3][2][level][N]: addend[row] + plain (.) rotate(x[row], s); addend "a", "x" (the rotated ciphertext itself) or None"""
        k = (level, s, form == "bcast", addend)
        if k not in self._want:
            x, a = self.inputs(level)
            o = self.o
            out = []
            for r in range(3):
                p = np.ascontiguousarray(self.plain[2 if form == "bcast" else r, :level])
                prod = o.multiply_plain(self.rot(level, s)[r], p)
                out.append(prod if addend is None else o.add(a[r] if addend == "a" else x[r], prod))
            self._want[k] = np.stack(out)
            self._want[k].setflags(write=False)
        return self._want[k]

    def plain_for(self, level, form, count=3):
        """(host array, stride in words)"""
        if form == "bcast":
            return np.ascontiguousarray(self.plain[2, :level]), 0
        if form == "per":
            return np.ascontiguousarray(self.plain[:count, :level]), level * self.n
        return np.ascontiguousarray(self.plain[:count]), self.L * self.n  # rows encoded for the top level

    def run(self, level, s, form="per", alias=None, addend=True, count=3):
        """one device call on the first `count` rows.  alias: None (three buffers), "out=addend", "addend=in", "out=in", "all"."""
        g = self.g
        x, a = (v[:count] for v in self.inputs(level))
        p, stride = self.plain_for(level, form, count)
        d_x, d_p = g.upload(x), g.upload(p)
        d_a = None if not addend else d_x if alias in ("addend=in", "all") else g.upload(a)
        d_o = d_a if alias in ("out=addend", "all") else d_x if alias == "out=in" else g.upload(np.full(x.shape, SENTINEL, dtype=np.uint64))
        try:
            pa = d_a.ptr if d_a is not None else None
            if s is CONJ:
                g.op("apply_galois_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(stride), pa, d_o.ptr, level, C.c_uint32(self.elt(CONJ)), C.c_size_t(count))
            else:
                g.op("rotate_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(stride), pa, d_o.ptr, level, int(s), C.c_size_t(count))
            got = g.download(d_o, x.shape)
            if d_o is not d_x:
                _same("the input is left alone", g.download(d_x, x.shape), x)
            if d_a is not None and d_o is not d_a and d_a is not d_x:
                _same("the addend is left alone", g.download(d_a, a.shape), a)
            _same("the plaintext is left alone", g.download(d_p, p.shape), p)
            return got
        finally:
            for b in {id(b): b for b in (d_x, d_p, d_a, d_o) if b is not None}.values():
                b.free()

    def check(self, tag, level, steps, forms=FORMS, alias=None, addend=True, count=3):
        """every step, the plaintext forms in turn (each of `forms` at the first step)"""
        forms = [f for f in forms if f != "wide" or level < self.L]
        for i, s in enumerate(steps):
            for form in (forms if i == 0 else [forms[i % len(forms)]]):
                got = self.run(level, s, form, alias, addend, count)
                want = self.want(level, s, form, None if not addend else "x" if alias in ("addend=in", "all") else "a")
                for row in range(count):
                    _same("%s nl=%d step %s plain %s alias %s row %d" % (tag, level, "conj" if s is CONJ else s, form, alias, row), got[row], want[row])

    def close(self):
        self.g.close()


def _split14(level, front="lean", pack=None, main=None):
    main = main or ("split4" if level <= 5 else "split3")
    pack = (1 if main == "split4" else 0) if pack is None else pack
    return "split14 front=%s pack=%d main=%s" % (front, pack, main)


# ---- CKKS, N = 2^14, every prime below 2^50: k_split4_main_fp (HALVES up to four limbs, one piece at five), k_split3_main_fp above ----
STEPS14 = (1, -1, N14 // 4, CONJ, 3)  # 3 = 4 - 1 has no key of its own: a NAF chain whose last hop takes the plaintext and the addend


@pytest.fixture(scope="module")
def deep14(oracle_mod, capi):
    """a 14-prime chain (13 data limbs); the lower levels by mod_switch"""
    r = Rig(oracle_mod, capi, N14, [50] + [40] * 12 + [50], (1, -1, N14 // 4, CONJ, 4))
    yield r
    r.close()


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7, 12])
def test_ckks14_fused_every_main_kernel(deep14, level):
    for count in (1, 3):
        assert deep14.g.route("rotate_mac_plain", level, count) == "fold+mac " + _split14(level)
    deep14.check("split14", level, STEPS14)


def test_ckks14_ragged_chunks(deep14):
    """chunks of two: a full chunk and a ragged one; the per-ciphertext plaintexts follow the chunk"""
    for env in ({"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "2"}, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "1"}):
        with _env(deep14.g, env):
            assert deep14.g.route("rotate_mac_plain", 3, 3) == "fold+mac " + _split14(3)
            deep14.check(" ".join(env), 3, (1, 3))


@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_PACK": "1"}, lambda lv: _split14(lv, pack=0)),
    ({"ABC_HIP_NO_KEY_TWIN": "1"}, lambda lv: _split14(lv)),
    ({"ABC_HIP_MAIN_TWO_PER_CU": "1"}, lambda lv: _split14(lv)),  # the one-piece pair phase at three and four limbs
    ({"ABC_HIP_NO_SPLIT4": "1"}, lambda lv: _split14(lv, main="split3")),  # k_split3_main_fp<.., 3> and <.., 4>
    ({"ABC_HIP_LEAN_LIMIT": "0"}, lambda lv: _split14(lv, front="fat")),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else "")
def test_ckks14_fused_switch_variants(deep14, env, route):
    with _env(deep14.g, env):
        for level in (3, 4):
            assert deep14.g.route("rotate_mac_plain", level, 3) == "fold+mac " + route(level)
            deep14.check(" ".join(env), level, (1, CONJ))


# ---- CKKS, N = 2^15: k_gsplit_main up to seven limbs, the deep kernel (unfused) above ----
@pytest.fixture(scope="module")
def deep15(oracle_mod, capi):
    r = Rig(oracle_mod, capi, N15, [50] + [40] * 8 + [50], (1, -1024))
    yield r
    r.close()


@pytest.mark.parametrize("level", [1, 3, 7])
def test_ckks15_fused(deep15, level):
    assert deep15.g.route("rotate_mac_plain", level, 3) == "fold+mac gsplit15"
    deep15.check("gsplit15", level, (1, -1024))


def test_ckks15_deep_kernel_takes_the_separate_sequence(deep15):
    assert deep15.g.route("rotate_mac_plain", 8, 3) == "fold mac=separate gsplit15"
    deep15.check("gsplit15 deep", 8, (1, -1024))


def test_ckks15_aliasing(deep15):
    for alias in ("out=addend", "out=in"):
        deep15.check("aliasing", 3, (1,), forms=("per",), alias=alias)
    deep15.check("no addend", 3, (1,), forms=("bcast",), addend=False)


# ---- fall-backs: the route says separate, the results are the same ----
@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_ROTATE_MAC_FUSION": "1"}, "fold mac=separate " + _split14(4)),
    ({"ABC_HIP_NO_GALOIS_FUSION": "1"}, "permute mac=separate " + _split14(4)),
    ({"ABC_HIP_NO_SPLIT": "1"}, "permute mac=separate lds_fp"),
    ({"ABC_HIP_NO_FUSED": "1"}, "permute mac=separate generic front=plain"),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else "")
def test_ckks14_fallback_switches(deep14, env, route):
    with _env(deep14.g, env):
        assert deep14.g.route("rotate_mac_plain", 4, 3) == route
        deep14.check(" ".join(env), 4, (1, CONJ, 3))
        deep14.check(" ".join(env) + " out=addend", 4, (-1,), forms=("per",), alias="out=addend")
        deep14.check(" ".join(env) + " no addend", 4, (-1,), forms=("bcast",), addend=False)
    assert deep14.g.route("rotate_mac_plain", 4, 3) == "fold+mac " + _split14(4)


def test_fallback_isplit(oracle_mod, capi):
    """a 60-bit prime at N = 2^14: the integer split sequence has no fused last kernel"""
    rig = Rig(oracle_mod, capi, N14, [60, 40, 40, 60], (1, CONJ))
    try:
        route = "fold mac=separate isplit14 guard=1 fpmask=0x6"
        assert rig.g.route("rotate_mac_plain", 3, 3) == route
        rig.check(route, 3, (1, CONJ), forms=("bcast", "per"))
        rig.check(route, 3, (1,), forms=("per",), alias="all")
    finally:
        rig.close()


# ---- aliasing, a missing addend and step 0 at one fused shape; out == in is never fused ----
DIAG_STEPS = (0, 1, -1, 2, N14 // 4)


@pytest.fixture(scope="module")
def small14(oracle_mod, capi):
    """{50,40,40,40,50} at N = 2^14 (four data limbs, used at three) with keys for the diagonals' steps, 4 (the chain of 3) and the
    conjugation"""
    r = Rig(oracle_mod, capi, N14, [50, 40, 40, 40, 50], (1, -1, 2, 4, N14 // 4, CONJ))
    yield r
    r.close()


@pytest.mark.parametrize("alias", ["out=addend", "addend=in", "out=in", "all"])
def test_aliasing(small14, alias):
    g = small14.g
    assert g.route("rotate_mac_plain", 3, 3) == "fold+mac " + _split14(3)
    assert g.route("rotate_mac_plain", 3, 3, in_place=True) == "fold mac=separate " + _split14(3)
    small14.check("aliasing", 3, (1, CONJ, 3), alias=alias)
    small14.check("aliasing, top level", 4, (1,), forms=("per",), alias=alias)


def test_no_addend(small14):
    small14.check("no addend", 3, (1, CONJ, 3), addend=False)
    small14.check("no addend, in place", 3, (1,), forms=("per",), alias="out=in", addend=False)
    with _env(small14.g, {"ABC_HIP_MAIN_TWO_PER_CU": "1"}):
        small14.check("no addend, one piece", 3, (1,), forms=("per",), addend=False)
    with _env(small14.g, {"ABC_HIP_NO_SPLIT4": "1"}):
        small14.check("no addend, split3", 3, (1,), forms=("per",), addend=False)


def test_step_zero(small14):
    """no key switch: multiply_plain, then add"""
    for alias in (None, "out=addend", "addend=in", "out=in", "all"):
        small14.check("step 0", 3, (0,), alias=alias)
    small14.check("step 0, no addend", 3, (0,), addend=False)
    small14.check("step 0, no addend, in place", 3, (0,), forms=("per",), alias="out=in", addend=False)


def test_numpy_front_ends(small14):
    g = small14.g
    x, a = small14.inputs(3)
    p, _ = small14.plain_for(3, "per")
    _same("one plaintext per ciphertext", g.rotate_mac_plain(x, p, a, 1), small14.want(3, 1))
    _same("rows of L limbs", g.rotate_mac_plain(x, small14.plain, a, 1), small14.want(3, 1))
    _same("broadcast, no addend", g.rotate_mac_plain(x, p[2], None, -1), small14.want(3, -1, "bcast", None))
    _same("one ciphertext", g.rotate_mac_plain(x[1], p[2], a[1], 1), small14.want(3, 1, "bcast")[1])
    _same("one element", g.apply_galois_mac_plain(x, p, a, small14.elt(CONJ)), small14.want(3, CONJ))


# ---- refused and empty calls: nothing is written ----
def test_refused_and_empty_calls(small14, capi):
    g, n = small14.g, small14.n
    x, a = small14.inputs(3)
    p, stride = small14.plain_for(3, "per")
    sentinel = np.full(x.shape, SENTINEL, dtype=np.uint64)
    d_x, d_a, d_p, d_o = g.upload(x), g.upload(a), g.upload(p), g.upload(sentinel)
    held = g.held_buffers()
    rm = lambda nl, s, count=3, st=stride, pl=None, out=None: g.op(  # noqa: E731
        "rotate_mac_plain", d_x.ptr, pl or d_p.ptr, C.c_size_t(st), d_a.ptr, out or d_o.ptr, nl, s, C.c_size_t(count))
    gm = lambda nl, e, count=3: g.op(  # noqa: E731
        "apply_galois_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(stride), d_a.ptr, d_o.ptr, nl, C.c_uint32(e), C.c_size_t(count))
    for bad in (1, 3 * n - 1, n):
        with pytest.raises(capi.AbcHipError, match="plain_stride must be 0 or at least nl"):
            rm(3, 1, st=bad)
        with pytest.raises(capi.AbcHipError, match="plain_stride must be 0 or at least nl"):
            rm(3, 0, st=bad)
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        rm(3, -2)  # no key, and a NAF form of one term
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        rm(3, -7)  # -8 + 1: no key for -8, whatever the last hop has
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        gm(3, 5)
    with pytest.raises(capi.AbcHipError, match="step count too large"):
        rm(3, n // 2)
    for nl in (0, 5, -1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            rm(nl, 1)
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            gm(nl, small14.elt(1))
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            g.route("rotate_mac_plain", nl, 3)
    # the plaintext inside d_out, at its start and over its last words; broadcast and per ciphertext
    words = x.size
    for off, st in ((0, 0), (words - 3 * n, 0), (words - 1, 0), (0, stride), (words - 8, stride)):
        with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):
            rm(3, 1, st=st, pl=C.c_void_p(d_o.ptr.value + 8 * off))
        with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):
            rm(3, 0, st=st, pl=C.c_void_p(d_o.ptr.value + 8 * off))
    with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):  # d_out inside the plaintexts
        g.op("rotate_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(stride), d_a.ptr, C.c_void_p(d_p.ptr.value + 8 * (p.size - 1)), 3, 1, C.c_size_t(3))
    rm(3, 1, 0)  # nothing to do: success, nothing enqueued
    rm(3, 0, 0)
    gm(3, small14.elt(1), 0)
    g.sync()
    _same("refused and empty calls wrote nothing", g.download(d_o, x.shape), sentinel)
    _same("... nor to the plaintexts", g.download(d_p, p.shape), p)
    assert g.held_buffers() == held
    for b in (d_x, d_a, d_p, d_o):
        b.free()


def test_bfv_context_is_refused(capi):
    """a BFV plaintext product needs transforms and is no fold of anything: the three calls say so and write nothing"""
    g = capi.Context.bfv_default(4096)
    try:
        g.keygen(7)
        L, n = g.L, g.n
        rng = np.random.default_rng(5)
        x = np.stack([rng.integers(0, q, size=(3, 2, n), dtype=np.uint64) for q in g.primes[:L]], axis=2)
        sentinel = np.full(x.shape, SENTINEL, dtype=np.uint64)
        d_x, d_p, d_o = g.upload(x), g.upload(np.zeros((5, L, n), dtype=np.uint64)), g.upload(sentinel)
        step1 = g.elt_from_step(1)
        with pytest.raises(capi.AbcHipError, match="rotate_mac_plain: CKKS only"):
            g.op("rotate_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(0), d_x.ptr, d_o.ptr, L, 1, C.c_size_t(3))
        with pytest.raises(capi.AbcHipError, match="rotate_mac_plain: CKKS only"):
            g.op("rotate_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(0), None, d_o.ptr, L, 0, C.c_size_t(3))
        with pytest.raises(capi.AbcHipError, match="apply_galois_mac_plain: CKKS only"):
            g.op("apply_galois_mac_plain", d_x.ptr, d_p.ptr, C.c_size_t(0), d_x.ptr, d_o.ptr, L, C.c_uint32(step1), C.c_size_t(3))
        with pytest.raises(capi.AbcHipError, match="diag_matvec: CKKS only"):
            g.op("diag_matvec", d_x.ptr, d_p.ptr, C.c_size_t(L * n), (C.c_int * 2)(0, 1), 2, d_o.ptr, L, C.c_size_t(3))
        g.sync()
        _same("a refused call wrote nothing", g.download(d_o, x.shape), sentinel)
        assert g.route("rotate_mac_plain", L, 3).endswith("mac=separate lds_fp")  # the table never fuses there
        for b in (d_x, d_p, d_o):
            b.free()
    finally:
        g.close()


# ---- diag_matvec ----
def _diag_reference(rig, level, steps, diags):
    """the oracle's composed sum, per row, in the order given; diags [len(steps)][>= level][N]"""
    o = rig.o
    out = []
    for row in range(3):
        acc = None
        for r, s in enumerate(steps):
            prod = o.multiply_plain(rig.rot(level, s)[row], np.ascontiguousarray(diags[r][:level]))
            acc = prod if acc is None else o.add(acc, prod)
        out.append(acc)
    return np.stack(out)


def _three_calls(rig, level, steps, diags):
    """the device's own sequence: rotate, multiply_plain, add per term"""
    g = rig.g
    x, _ = rig.inputs(level)
    acc = None
    for r, s in enumerate(steps):
        prod = g.multiply_plain(x if s == 0 else g.rotate(x, s), np.ascontiguousarray(diags[r][:level]))
        acc = prod if acc is None else g.add(acc, prod)
    return acc


@pytest.fixture(scope="module")
def diags14(small14):
    """five diagonals [5][L][N] encoded for the top level: random residues, the third the extremes"""
    rng = np.random.default_rng(99)
    d = _random_poly(small14.primes, small14.L, N14, rng, 5)
    d[2] = small14.plain[2]
    d.setflags(write=False)
    return d


def test_diag_matvec_five_diagonals(small14, diags14):
    g = small14.g
    x, _ = small14.inputs(3)
    want = _diag_reference(small14, 3, DIAG_STEPS, diags14)
    with _env(g, {"ABC_HIP_CHUNK": "2"}):
        assert g.route("rotate_mac_plain", 3, 3) == "fold+mac " + _split14(3)
        _same("rows of nl limbs", g.diag_matvec(x, diags14[:, :3], DIAG_STEPS), want)
        _same("rows of L limbs at nl < L", g.diag_matvec(x, diags14, DIAG_STEPS), want)
        _same("the device's three-call sequence", _three_calls(small14, 3, DIAG_STEPS, diags14), want)
        _same("one ciphertext", g.diag_matvec(x[2], diags14, DIAG_STEPS), want[2])
    with _env(g, {"ABC_HIP_NO_ROTATE_MAC_FUSION": "1"}):
        _same("separate sequence", g.diag_matvec(x, diags14, DIAG_STEPS), want)
    # duplicate steps, a NAF chain, and step 0 in the middle: the running sum is the addend of a plain product
    steps = (1, 1, 0, 3, 1)
    _same("duplicate steps", g.diag_matvec(x, diags14, steps), _diag_reference(small14, 3, steps, diags14))
    _same("one term, step 0", g.diag_matvec(x, diags14[:1], (0,)), _diag_reference(small14, 3, (0,), diags14))
    _same("top level", g.diag_matvec(small14.inputs(4)[0], diags14[:2], (1, 0)), _diag_reference(small14, 4, (1, 0), diags14))
    _same("no steps: zeros", g.diag_matvec(x, diags14[:0], ()), np.zeros_like(x))


def test_diag_matvec_refused_and_empty_calls(small14, diags14, capi):
    g, n = small14.g, small14.n
    x, _ = small14.inputs(3)
    sentinel = np.full(x.shape, SENTINEL, dtype=np.uint64)
    d_x, d_d, d_o = g.upload(x), g.upload(diags14), g.upload(sentinel)
    L = small14.L
    held = g.held_buffers()

    def dm(steps, stride=L * n, nl=3, count=3, d_in=None, diags=None, out=None, arr=True):
        a = (C.c_int * max(len(steps), 1))(*steps) if arr else None
        g.op("diag_matvec", d_in or d_x.ptr, diags or d_d.ptr, C.c_size_t(stride), a, len(steps), out or d_o.ptr, nl, C.c_size_t(count))

    for bad, msg in ((16, "Galois key not present"), (-2, "Galois key not present"), (n // 2, "step count too large")):
        with pytest.raises(capi.AbcHipError, match=msg):
            dm((1, -1, bad, 2, n // 4))  # the third of five
    for stride in (0, 1, 3 * n - 1):
        with pytest.raises(capi.AbcHipError, match="diag_stride must be at least nl"):
            dm(DIAG_STEPS, stride=stride)
    with pytest.raises(capi.AbcHipError, match="bad step list"):
        dm((1, 2), arr=False)
    with pytest.raises(capi.AbcHipError, match="bad step list"):
        g.op("diag_matvec", d_x.ptr, d_d.ptr, C.c_size_t(L * n), None, -1, d_o.ptr, 3, C.c_size_t(3))
    for nl in (0, 5):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            dm(DIAG_STEPS, nl=nl)
    words = x.size
    for off in (0, words - 1):  # a diagonal inside d_out
        with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):
            dm((1, 0), diags=C.c_void_p(d_o.ptr.value + 8 * off), stride=3 * n)
    with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):  # d_out inside the diagonals: the last row's last read word
        dm(DIAG_STEPS, out=C.c_void_p(d_d.ptr.value + 8 * (4 * L * n + 3 * n - 1)))
    for off in (0, words - 1):  # d_in inside d_out, and d_out == d_in
        with pytest.raises(capi.AbcHipError, match="d_out must not overlap d_in"):
            dm((1, 0), d_in=C.c_void_p(d_o.ptr.value + 8 * off))
    dm((1, 0), count=0)  # nothing to do: success, nothing enqueued
    dm((), count=0)
    g.sync()
    _same("refused and empty calls wrote nothing", g.download(d_o, x.shape), sentinel)
    _same("... nor to the diagonals", g.download(d_d, diags14.shape), diags14)
    assert g.held_buffers() == held
    for b in (d_x, d_d, d_o):
        b.free()


def test_recorded_diag_matvec_follows_its_input(small14, diags14):
    """record a diag_matvec (eagerly once first: the arenas get their size), overwrite the input, replay: the result is that of the
    new input.  Destroying the graph lets go of everything it held."""
    g = small14.g
    x, _ = small14.inputs(3)
    steps = (0, 1, 3, -1)  # a plain product, a fused term, a NAF chain, a fused term
    arr = (C.c_int * len(steps))(*steps)
    d_x, d_d, d_o = g.upload(x), g.upload(diags14), g.alloc(x.nbytes)
    held = g.held_buffers()
    want = _diag_reference(small14, 3, steps, diags14)

    def circuit():
        g.op("diag_matvec", d_x.ptr, d_d.ptr, C.c_size_t(small14.L * N14), arr, len(steps), d_o.ptr, 3, C.c_size_t(3))

    circuit()
    g.sync()
    g.graph_begin()
    circuit()
    exe = g.graph_end()
    try:
        _same("eager", g.download(d_o, x.shape), want)
        x2 = np.ascontiguousarray(x[::-1])  # the same rows in another order: new input, same buffers
        g.op("memcpy_h2d", d_x.ptr, x2.ctypes.data_as(C.c_void_p), C.c_size_t(x2.nbytes))
        g.op("memcpy_h2d", d_o.ptr, np.full(x.shape, SENTINEL, dtype=np.uint64).ctypes.data_as(C.c_void_p), C.c_size_t(x.nbytes))
        g.graph_launch(exe)
        _same("replayed", g.download(d_o, x.shape), want[::-1])
    finally:
        g.graph_destroy(exe)
    assert g.held_buffers() == held
    for b in (d_x, d_d, d_o):
        b.free()


# ---- end to end: a 4 x 4 matrix times a vector, by diagonals ----
def test_matrix_vector_end_to_end(small14):
    """Encode the diagonals of a 4 x 4 matrix and a vector (period 4 over the slots, so a rotation of the slots is a rotation of the
    vector), encrypt, diag_matvec, rescale, decrypt, decode.  The pin: the decoded slots are identical to those of the device's
    three-call sequence.  Against numpy's product the bound is the number of diagonals times the 1e-5 tests/test_gpu_parity.py allows
    for one CKKS product of entries in [-1, 1]: a sanity check of the encoding and the rotation's direction, not a precision claim."""
    g, o, n = small14.g, small14.o, small14.n
    L, slots, scale = small14.L, small14.n // 2, 2.0 ** 40
    assert L == 4
    rng = np.random.default_rng(44)
    M, v = rng.uniform(-1, 1, (4, 4)), rng.uniform(-1, 1, 4)
    steps = (0, 1, 2, -1)  # the diagonal of step s holds M[i][(i + s) % 4]
    idx = np.arange(slots) % 4
    diag_slots = np.stack([M[idx, (idx + s) % 4] for s in steps])
    diags = g.ckks_encode(diag_slots, scale)  # [4][L][N]
    ct = g.encrypt(g.ckks_encode(v[idx], scale), 0xE2E)  # [2][L][N]
    fused = g.diag_matvec(ct, diags, steps)
    acc = None
    for r, s in enumerate(steps):
        prod = g.multiply_plain(ct if s == 0 else g.rotate(ct, s), diags[r])
        acc = prod if acc is None else g.add(acc, prod)
    out_scale = scale * scale / o.primes[L - 1]
    dec = [g.ckks_decode(g.decrypt(g.rescale(c)), out_scale) for c in (fused, acc)]
    assert np.array_equal(dec[0], dec[1]), "decoded slots differ from the three-call sequence"
    _same("and so do the ciphertexts", fused, acc)
    want = (M @ v)[idx]
    err = np.abs(dec[0] - want).max()
    print("matrix x vector by diagonals: max |error| = %.3g" % err)
    assert err < len(steps) * 1e-5
