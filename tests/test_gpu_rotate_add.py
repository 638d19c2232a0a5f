"""Fused rotate-and-add on the device (abc_hip_rotate_add / abc_hip_apply_galois_add / abc_hip_rotate_sum): d_out = d_addend +
rotate(d_in), the addend being one more operand of the key switch's last kernel where route("rotate_add") says "fold+add", and a
rotation into an arena followed by the add kernel everywhere else.  A modular add is exact, so every comparison is bit-exact against
o.add(addend, o.rotate(ct, s)) / o.apply_galois, per row.  Inputs: two rows of random residues and one of extremes (0, 1, (q+-1)/2,
q-2, q-1 and a long run of q-1), the extremes as input and as addend at once, so the three-term sum reaches its largest magnitude.
The oracle generates Galois keys for the elements a test uses only; every fused shape asserts its route string, so a silent fall-back
to the separate sequence fails."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N13, N14, N15, N16 = 1 << 13, 1 << 14, 1 << 15, 1 << 16
CONJ = None  # as a step: the element 2N - 1 (conjugation / column swap)


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


def _random_ct(primes, nl, n, rng):
    return np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in primes[:nl]], axis=1)


def _extreme_ct(primes, nl, n, rng):
    """residues from {0, 1, (q-1)/2, (q+1)/2, q-2, q-1} and random values, and a long run of q-1 (as tests/test_gpu_configs.py)"""
    ct = np.empty((2, nl, n), dtype=np.uint64)
    for j in range(nl):
        q = primes[j]
        pool = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
        pick = rng.integers(0, 8, size=(2, n))
        rnd = rng.integers(0, q, size=(2, n), dtype=np.uint64)
        ct[:, j, :] = np.where(pick < 6, pool[np.minimum(pick, 5)], rnd)
    ct[:, :, : n // 4] = np.array(primes[:nl], dtype=np.uint64)[None, :, None] - 1  # either component: the addend's c1 is added too
    return ct


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
    """one oracle with Galois keys for `steps`, a device context with the same keys, three inputs and three addends at every level
    (rows 0, 1 random, row 2 extremes in both) and the references computed so far (shared by the tests of a module, never changed)"""

    def __init__(self, om, capi, scheme, n, primes, steps, t=0, seed=0x5ADD):
        self.o = om.Oracle(scheme, n, primes, t)
        self.ckks = scheme == om.CKKS
        self.n, self.primes = n, list(primes)
        self.o.keygen(seed, elts=sorted({self.elt(s) for s in steps}))
        o = self.o
        self.g = capi.Context(capi.CKKS if self.ckks else capi.BFV, n, o.primes, o.t)
        self.g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
        self.L = o.L
        rng = np.random.default_rng(n + len(primes))
        mk = lambda: np.stack([_random_ct(primes, self.L, n, rng), _random_ct(primes, self.L, n, rng), _extreme_ct(primes, self.L, n, rng)])  # noqa: E731
        self._in = {self.L: (mk(), mk())}
        self._want = {}

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

    def rot(self, ct, s):
        return self.o.apply_galois(ct, self.elt(CONJ)) if s is CONJ else self.o.rotate(ct, s)

    def want(self, level, s, addend="a"):
        """[3][2][level][N]: addend[row] + rotate(x[row], s); addend "a" (the second input) or "x" (the rotated ciphertext itself)"""
        k = (level, s, addend)
        if k not in self._want:
            x, a = self.inputs(level)
            ad = a if addend == "a" else x
            self._want[k] = np.stack([self.o.add(ad[r], self.rot(x[r], s)) for r in range(3)])
            self._want[k].setflags(write=False)
        return self._want[k]

    def run(self, level, s, alias=None, count=3):
        """one device call on the first `count` rows.  alias: None (three buffers), "out=addend", "addend=in", "out=in", "all"."""
        g = self.g
        x, a = (v[:count] for v in self.inputs(level))
        d_x = g.upload(x)
        d_a = d_x if alias in ("addend=in", "all") else g.upload(a)
        d_o = d_a if alias in ("out=addend", "all") else d_x if alias == "out=in" else g.upload(np.full(x.shape, 0xDEADBEEFDEADBEEF, dtype=np.uint64))
        try:
            if s is CONJ:
                g.op("apply_galois_add", d_x.ptr, d_a.ptr, d_o.ptr, level, C.c_uint32(self.elt(CONJ)), C.c_size_t(count))
            else:
                g.op("rotate_add", d_x.ptr, d_a.ptr, d_o.ptr, level, int(s), C.c_size_t(count))
            got = g.download(d_o, x.shape)
            if d_o is not d_x and d_a is not d_x:
                _same("the input is left alone", g.download(d_x, x.shape), x)
            if d_o is not d_a and d_a is not d_x:
                _same("the addend is left alone", g.download(d_a, a.shape), a)
            return got
        finally:
            for b in {id(b): b for b in (d_x, d_a, d_o)}.values():
                b.free()

    def check(self, tag, level, steps, alias=None, count=3):
        for s in steps:
            got = self.run(level, s, alias, count)
            want = self.want(level, s, "x" if alias in ("addend=in", "all") else "a")
            for row in range(count):
                _same("%s nl=%d step %s alias %s row %d" % (tag, level, "conj" if s is CONJ else s, alias, row), got[row], want[row])

    def close(self):
        self.g.close()


def _ckks(om, capi, n, bits, steps):
    return Rig(om, capi, om.CKKS, n, om.create_primes(n, bits), steps)


def _bfv(om, capi, n, bits, steps):
    primes = om.default_bfv_primes(n) if bits is None else om.create_primes(n, bits)
    return Rig(om, capi, om.BFV, n, primes, steps, t=om.plain_modulus_batching(n, 20))


# ---- CKKS, N = 2^14, every prime below 2^50: k_split4_main_fp (HALVES up to four limbs, one piece at five), k_split3_main_fp above ----
STEPS14 = (1, -1, N14 // 4, CONJ, 3)  # 3 = 4 - 1 has no key of its own: a NAF chain whose last hop takes the addend


@pytest.fixture(scope="module")
def deep14(oracle_mod, capi):
    """a 13-prime chain; the lower levels by mod_switch"""
    r = _ckks(oracle_mod, capi, N14, [50] + [40] * 11 + [50], (1, -1, N14 // 4, CONJ, 4))
    yield r
    r.close()


def _split14(level, front="lean", pack=None, main=None):
    main = main or ("split4" if level <= 5 else "split3")
    pack = (1 if main == "split4" else 0) if pack is None else pack
    return "split14 front=%s pack=%d main=%s" % (front, pack, main)


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7, 12])
def test_ckks14_fused_every_main_kernel(deep14, level):
    for count in (1, 3):
        assert deep14.g.route("rotate_add", level, count) == "fold+add " + _split14(level)
    deep14.check("split14", level, STEPS14)


def test_ckks14_ragged_chunks(deep14):
    """chunks of two: a full chunk and a ragged one (up to eight ciphertexts a call stays on one lane whatever ABC_HIP_LANES says)"""
    for env in ({"ABC_HIP_CHUNK": "2"}, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "1"}, {"ABC_HIP_LANES": "1"}):
        with _env(deep14.g, env):
            assert deep14.g.route("rotate_add", 3, 3) == "fold+add " + _split14(3)
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
            assert deep14.g.route("rotate_add", level, 3) == "fold+add " + route(level)
            deep14.check(" ".join(env), level, (1, CONJ))


# ---- CKKS, N = 2^15: k_gsplit_main up to seven limbs, the deep kernel (unfused) above ----
@pytest.fixture(scope="module")
def deep15(oracle_mod, capi):
    r = _ckks(oracle_mod, capi, N15, [50] + [40] * 7 + [50], (1, -1024))
    yield r
    r.close()


@pytest.mark.parametrize("level", [1, 3, 7])
def test_ckks15_fused(deep15, level):
    assert deep15.g.route("rotate_add", level, 3) == "fold+add gsplit15"
    deep15.check("gsplit15", level, (1, -1024))


def test_ckks15_deep_kernel_takes_the_separate_sequence(deep15):
    assert deep15.g.route("rotate_add", 8, 3) == "fold add=separate gsplit15"
    deep15.check("gsplit15 deep", 8, (1, -1024))


# ---- BFV (coefficient form: the gathered c0 changes sign, the second addend does not) ----
BFV_STEPS = (1, -1, CONJ)
BFV_FUSED = {  # name: (N, chain bits or None for BFVDefault(N), level, env, route)
    "bfv16384_per_target": (N14, None, 8, {}, "fold+add bsplit14 pass0=per_target"),
    "bfv16384_per_limb": (N14, None, 8, {"ABC_HIP_PASS0_TARGET_LIMIT": "0"}, "fold+add bsplit14 pass0=per_limb"),
    "bfv8192": (N13, None, 4, {}, "fold+add bsplit_big"),                  # k_bsplit_finish_big<13>
    "bfv32768_50bit": (N15, [49, 49, 50], 2, {}, "fold+add bsplit_big"),   # k_bsplit_finish_lds<15>
    "bfv65536_50bit": (N16, [49, 49, 50], 2, {}, "fold+add bsplit_big"),   # k_bsplit_finish_lds<16>
}


@pytest.fixture(scope="module")
def bfv_rigs(oracle_mod, capi):
    cache = {}

    def get(n, bits):
        k = (n, tuple(bits or ()))
        if k not in cache:
            cache[k] = _bfv(oracle_mod, capi, n, bits, BFV_STEPS)
        return cache[k]
    yield get
    for r in cache.values():
        r.close()


@pytest.mark.parametrize("name", list(BFV_FUSED))
def test_bfv_fused(name, bfv_rigs):
    n, bits, level, env, route = BFV_FUSED[name]
    rig = bfv_rigs(n, bits)
    assert rig.L == level
    with _env(rig.g, env):
        assert rig.g.route("rotate_add", level, 3) == route
        rig.check(name, level, BFV_STEPS)
        with _env(rig.g, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": "1"}):
            rig.check(name + " chunks of 2", level, (1,))


# ---- fall-backs: the route says separate, the results are the same ----
@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_ROTATE_ADD_FUSION": "1"}, "fold add=separate " + _split14(4)),
    ({"ABC_HIP_NO_GALOIS_FUSION": "1"}, "permute add=separate " + _split14(4)),
    ({"ABC_HIP_NO_SPLIT": "1"}, "permute add=separate lds_fp"),
    ({"ABC_HIP_NO_FUSED": "1"}, "permute add=separate generic front=plain"),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else "")
def test_ckks14_fallback_switches(deep14, env, route):
    with _env(deep14.g, env):
        assert deep14.g.route("rotate_add", 4, 3) == route
        deep14.check(" ".join(env), 4, (1, CONJ, 3))
        deep14.check(" ".join(env) + " out=addend", 4, (-1,), alias="out=addend")
    assert deep14.g.route("rotate_add", 4, 3) == "fold+add " + _split14(4)


def test_fallback_other_sequences(oracle_mod, capi):
    """isplit (a 60-bit prime at N = 2^14) and the LDS-resident BFV key switch (BFVDefault(4096)) have no fused last kernel"""
    for make, level, steps, route in [
        (lambda: _ckks(oracle_mod, capi, N14, [60, 40, 40, 60], (1, CONJ)), 3, (1, CONJ), "fold add=separate isplit14 guard=1 fpmask=0x6"),
        (lambda: _bfv(oracle_mod, capi, 4096, None, (1, CONJ)), 2, (1, CONJ), "permute add=separate lds_fp"),
    ]:
        rig = make()
        try:
            assert rig.g.route("rotate_add", level, 3) == route
            rig.check(route, level, steps)
            rig.check(route, level, steps[:1], alias="all")
        finally:
            rig.close()


# ---- aliasing, at one fused shape per scheme; out == in is never fused ----
@pytest.fixture(scope="module")
def small14(oracle_mod, capi):
    """{50,40,40,50} at N = 2^14 with a key for every power of two up to N/4 (the rotate-and-sum tree), -1 and the conjugation"""
    r = _ckks(oracle_mod, capi, N14, [50, 40, 40, 50], [1 << k for k in range(13)] + [-1, CONJ])
    yield r
    r.close()


@pytest.mark.parametrize("alias", ["out=addend", "addend=in", "out=in", "all"])
def test_aliasing_ckks(small14, alias):
    g = small14.g
    assert g.route("rotate_add", 3, 3) == "fold+add " + _split14(3)
    assert g.route("rotate_add", 3, 3, in_place=True) == "fold add=separate " + _split14(3)
    small14.check("aliasing", 3, (1, CONJ, 3), alias=alias)


@pytest.mark.parametrize("alias", ["out=addend", "addend=in", "out=in", "all"])
def test_aliasing_bfv(bfv_rigs, alias):
    rig = bfv_rigs(N13, None)
    assert rig.g.route("rotate_add", 4, 3) == "fold+add bsplit_big"
    assert rig.g.route("rotate_add", 4, 3, in_place=True) == "fold add=separate bsplit_big"
    rig.check("aliasing", 4, (1, CONJ), alias=alias)


def test_aliasing_ckks15(deep15):
    for alias in ("out=addend", "out=in"):
        deep15.check("aliasing", 3, (1,), alias=alias)


# ---- step 0, empty and refused calls ----
def test_step_zero_empty_and_refused_calls(small14, capi):
    g, n = small14.g, small14.n
    x, a = small14.inputs(3)
    got = g.rotate_add(x, a, 0)
    for row in range(3):
        _same("step 0 is addend + in", got[row], small14.o.add(a[row], x[row]))
    _same("numpy front end, one ciphertext", g.rotate_add(x[1], a[1], 1), small14.want(3, 1)[1])
    _same("numpy front end, one element", g.apply_galois_add(x, a, small14.elt(CONJ)), small14.want(3, CONJ))
    sentinel = np.full(x.shape, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    d_x, d_a, d_o = g.upload(x), g.upload(a), g.upload(sentinel)
    held = g.held_buffers()
    ra = lambda nl, s, count=3: g.op("rotate_add", d_x.ptr, d_a.ptr, d_o.ptr, nl, s, C.c_size_t(count))  # noqa: E731
    ga = lambda nl, e, count=3: g.op("apply_galois_add", d_x.ptr, d_a.ptr, d_o.ptr, nl, C.c_uint32(e), C.c_size_t(count))  # noqa: E731
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        ra(3, -2)  # no key, and a NAF form of one term
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        ra(3, -7)  # -8 + 1: no key for -8, whatever the last hop has
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        ga(3, 5)
    with pytest.raises(capi.AbcHipError, match="step count too large"):
        ra(3, n // 2)
    for nl in (0, 4, -1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            ra(nl, 1)
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            ga(nl, small14.elt(1))
        for op in ("rotate_add", "rotate"):  # route op 5 refuses a level as op 2 does
            with pytest.raises(capi.AbcHipError, match="limb count out of range"):
                g.route(op, nl, 3)
    ra(3, 1, 0)  # nothing to do: success, nothing enqueued
    ra(3, 0, 0)
    ga(3, small14.elt(1), 0)
    g.sync()
    _same("refused and empty calls wrote nothing", g.download(d_o, x.shape), sentinel)
    assert g.held_buffers() == held
    for b in (d_x, d_a, d_o):
        b.free()


# ---- the rotate-and-sum tree ----
def _tree(rig, level, steps):
    """the oracle's loop, per row: acc = acc + rotate(acc, s)"""
    x, _ = rig.inputs(level)
    out = []
    for row in range(3):
        acc = x[row]
        for s in steps:
            acc = rig.o.add(acc, rig.o.rotate(acc, s))
        out.append(acc)
    return x, np.stack(out)


def _check_tree(rig, level, steps, route):
    g = rig.g
    assert g.route("rotate_add", level, 3) == route
    x, want = _tree(rig, level, steps)
    _same("rotate_sum", g.rotate_sum(x, steps), want)
    d = g.upload(x)  # d_out == d_in: only the last sum lands there
    arr = (C.c_int * len(steps))(*steps)
    g.op("rotate_sum", d.ptr, d.ptr, level, arr, len(steps), C.c_size_t(3))
    _same("rotate_sum in place", g.download(d, x.shape), want)
    d.free()
    return x


def test_rotate_sum_ckks14(small14, capi):
    steps = [N14 // 4 >> k for k in range(13)]  # N/4 .. 1: config 3's tree
    x = _check_tree(small14, 3, steps, "fold+add " + _split14(3))
    g = small14.g
    _same("no steps: a copy", g.rotate_sum(x, []), x)
    _same("one step", g.rotate_sum(x, [1]), small14.want(3, 1, "x"))
    _same("two steps, one a NAF chain", g.rotate_sum(x[:1], [3, 0]),
          [small14.o.add(t, t) for t in [small14.o.add(x[0], small14.o.rotate(x[0], 3))]])
    # a step without a key in the middle of the list: refused before the first launch
    sentinel = np.full(x.shape, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    d_x, d_o = g.upload(x), g.upload(sentinel)
    for bad, msg in ((-2, "Galois key not present"), (N14 // 2, "step count too large")):
        arr = (C.c_int * 3)(1, bad, 2)
        with pytest.raises(capi.AbcHipError, match=msg):
            g.op("rotate_sum", d_x.ptr, d_o.ptr, 3, arr, 3, C.c_size_t(3))
    with pytest.raises(capi.AbcHipError, match="bad step list"):
        g.op("rotate_sum", d_x.ptr, d_o.ptr, 3, None, 2, C.c_size_t(3))
    g.op("rotate_sum", d_x.ptr, d_o.ptr, 3, (C.c_int * 1)(1), 1, C.c_size_t(0))
    g.sync()
    _same("refused and empty calls wrote nothing", g.download(d_o, x.shape), sentinel)
    d_x.free(); d_o.free()


def test_rotate_sum_ckks15(oracle_mod, capi):
    steps = (1, 2, 4, 64, 128, 256)  # config 4's box sum
    rig = _ckks(oracle_mod, capi, N15, [50, 40, 40, 50], steps)
    try:
        _check_tree(rig, 3, list(steps), "fold+add gsplit15")
    finally:
        rig.close()


def test_rotate_sum_bfv8192(oracle_mod, capi):
    steps = [N13 // 4 >> k for k in range(12)]
    rig = _bfv(oracle_mod, capi, N13, None, steps)
    try:
        _check_tree(rig, 4, steps, "fold+add bsplit_big")
    finally:
        rig.close()


# ---- recorded circuits ----
def test_recorded_rotate_sum_and_rotate_add_follow_their_input(small14):
    """record a rotate_sum and a rotate_add (eagerly once first: the arenas get their size), overwrite the input, replay: the results
    are those of the new input.  Destroying the graph lets go of everything it held."""
    g, o = small14.g, small14.o
    x, a = small14.inputs(3)
    steps = [4, 2, 1]
    arr = (C.c_int * 3)(*steps)
    d_x, d_a = g.upload(x), g.upload(a)
    d_sum, d_ra = g.alloc(x.nbytes), g.alloc(x.nbytes)
    held = g.held_buffers()

    def circuit():
        g.op("rotate_sum", d_x.ptr, d_sum.ptr, 3, arr, 3, C.c_size_t(3))
        g.op("rotate_add", d_sum.ptr, d_a.ptr, d_ra.ptr, 3, -1, C.c_size_t(3))
        g.op("rotate_add", d_ra.ptr, d_ra.ptr, d_ra.ptr, 3, 3, C.c_size_t(3))  # a NAF chain from and into one buffer: its last hop reads an arena

    def reference(xs):
        out = []
        for row in range(3):
            acc = xs[row]
            for s in steps:
                acc = o.add(acc, o.rotate(acc, s))
            r = o.add(a[row], o.rotate(acc, -1))
            out.append((acc, o.add(r, o.rotate(r, 3))))
        return out

    circuit()
    g.sync()
    g.graph_begin()
    circuit()
    exe = g.graph_end()
    try:
        for row, (s, r) in enumerate(reference(x)):
            _same("eager rotate_sum row %d" % row, g.download(d_sum, x.shape)[row], s)
            _same("eager rotate_add row %d" % row, g.download(d_ra, x.shape)[row], r)
        x2 = np.ascontiguousarray(x[::-1])  # the same rows in another order: new input, same buffers
        g.op("memcpy_h2d", d_x.ptr, x2.ctypes.data_as(C.c_void_p), C.c_size_t(x2.nbytes))
        g.graph_launch(exe)
        for row, (s, r) in enumerate(reference(x2)):
            _same("replayed rotate_sum row %d" % row, g.download(d_sum, x.shape)[row], s)
            _same("replayed rotate_add row %d" % row, g.download(d_ra, x.shape)[row], r)
    finally:
        g.graph_destroy(exe)
    assert g.held_buffers() == held
    for b in (d_x, d_a, d_sum, d_ra):
        b.free()
