"""Hoisted rotations on the device (abc_hip_apply_galois_hoisted / abc_hip_rotate_hoisted): several Galois elements of one input
in one call, in the hoisted form of DESIGN.md section 4.  The kernels do not share the decomposition between the elements yet: each
element runs the plain key switch of its level with the permuted mirror of its key, then the permutation, so what is under test is the
definition, the mirror and its lifetime, and the dispatch around kernels that existed.  Every comparison is bit-exact against tests/hoisted_spec.py, the definition composed from oracle calls -- never
against o.apply_galois, which is a different ciphertext (tests/test_hoisted_spec.py).  The oracle generates Galois keys for the
elements a test uses only (keygen(seed, elts=...)) and the device loads them, which keeps key generation short."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hoisted_spec import hoisted_reference, permuted_key  # noqa: E402

pytestmark = pytest.mark.gpu

N14 = 1 << 14
HEAD = [50, 40, 40, 40, 50]
LEAN = "split14 front=lean pack=1 main=split4"  # the key switch a hoisted call runs per element: the plain one, never a rotation's fold


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


def _random_cts(primes, nl, n, count, rng):
    return np.stack([np.stack([rng.integers(0, q, size=(2, n), dtype=np.uint64) for q in primes[:nl]], axis=1) for _ in range(count)])


def _extreme_ct(primes, nl, n, rng):
    """residues from {0, 1, (q-1)/2, (q+1)/2, q-2, q-1} and random values, and a long run of q-1 (as tests/test_gpu_configs.py)"""
    ct = np.empty((2, nl, n), dtype=np.uint64)
    for j in range(nl):
        q = primes[j]
        pool = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
        pick = rng.integers(0, 8, size=(2, n))
        rnd = rng.integers(0, q, size=(2, n), dtype=np.uint64)
        ct[:, j, :] = np.where(pick < 6, pool[np.minimum(pick, 5)], rnd)
    ct[0, :, : n // 4] = np.array(primes[:nl], dtype=np.uint64)[:, None] - 1
    return ct


def _load(capi, o):
    g = capi.Context(capi.CKKS if o.scheme == 2 else capi.BFV, o.n, o.primes, o.t)
    g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
    return g


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
    """one oracle with Galois keys for `steps` (None: the conjugation / column swap), a device context holding the same keys, inputs
    at every level and the references computed so far (shared by the tests of the module, never changed)"""

    def __init__(self, om, capi, scheme, n, primes, steps, t=0, seed=0x401, count=5):
        self.o = om.Oracle(scheme, n, primes, t)
        self.elts = [2 * n - 1 if s is None else self.o.elt_from_step(s) for s in steps]
        self.o.keygen(seed, elts=self.elts)
        self.g = _load(capi, self.o)
        self.L, self.n, self.primes = self.o.L, n, list(primes)
        rng = np.random.default_rng(n + len(primes))
        self._in = {self.L: _random_cts(primes, self.L, n, count, rng)}
        self._keys, self._want = {}, {}

    def inputs(self, level):
        if level not in self._in:
            self._in[level] = np.stack([self.o.mod_switch(ct) for ct in self.inputs(level + 1)])
            self._in[level].setflags(write=False)
        return self._in[level]

    def key(self, elt):
        if elt not in self._keys:
            self._keys[elt] = permuted_key(self.o, elt)
        return self._keys[elt]

    def want(self, level, row, elt):
        k = (level, row, elt)
        if k not in self._want:
            self._want[k] = hoisted_reference(self.o, self.inputs(level)[row], elt, self.key(elt))
            self._want[k].setflags(write=False)
        return self._want[k]

    def check(self, tag, level, count, elts, rows=None):
        """one call on the first `count` inputs of the level; rows (default: all) of every slab against the reference"""
        got = self.g.apply_galois_hoisted(self.inputs(level)[:count], elts)
        assert got.shape == (len(elts), count, 2, level, self.n)
        for r, elt in enumerate(elts):
            for row in (range(count) if rows is None else rows):
                _same("%s nl=%d count=%d slab %d (elt %d) row %d" % (tag, level, count, r, elt, row), got[r, row], self.want(level, row, elt))
        return got

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def rig14(oracle_mod, capi):
    """the headline chain {50,40,40,40,50} at N = 2^14: steps 1, -1, 64, N/4 and the conjugation"""
    r = Rig(oracle_mod, capi, oracle_mod.CKKS, N14, oracle_mod.create_primes(N14, HEAD), (1, -1, 64, N14 // 4, None))
    yield r
    r.close()


# ---- the N = 2^14 split key switch under a hoisted call ----
@pytest.mark.parametrize("level", [4, 3, 2, 1])
def test_split14_every_level(rig14, level):
    g, e = rig14.g, rig14.elts
    assert g.route("keyswitch", level, 1) == LEAN and g.route("keyswitch", level, 3) == LEAN
    rig14.check("five elements", level, 1, e)
    rig14.check("two elements and a duplicate", level, 3, [e[0], e[2], e[0]])
    one = g.apply_galois_hoisted(rig14.inputs(level)[1], [e[4], e[1]])  # a single ciphertext without the batch dimension
    assert one.shape == (2, 2, level, rig14.n)
    _same("unbatched, conjugation", one[0], rig14.want(level, 1, e[4]))
    _same("unbatched, step -1", one[1], rig14.want(level, 1, e[1]))


def test_split14_three_chunks_ragged_last_both_lanes(rig14):
    e = rig14.elts
    with _env(rig14.g, {"ABC_HIP_CHUNK": "2"}):
        assert rig14.g.route("keyswitch", 4, 5) == LEAN
        rig14.check("chunks of 2", 4, 5, [e[2], e[1]])


def test_split14_fat_front_every_row(rig14, oracle_mod):
    """25 ciphertexts in one chunk (one lane): cc * nl = 100 > 96, the 139 KiB operand kernel.  Three rows against the reference, and
    every row against the same rows through the block-wise front in calls of five."""
    e = [rig14.elts[0], rig14.elts[3]]
    rng = np.random.default_rng(25)
    big = np.concatenate([rig14.inputs(4), _random_cts(rig14.primes, 4, rig14.n, 20, rng)])
    with _env(rig14.g, {"ABC_HIP_LANES": "1"}):
        assert rig14.g.route("keyswitch", 4, 25) == "split14 front=fat pack=1 main=split4"
        got = rig14.g.apply_galois_hoisted(big, e)
    for r, elt in enumerate(e):
        for row in (0, 4):
            _same("fat front slab %d row %d" % (r, row), got[r, row], rig14.want(4, row, elt))
        _same("fat front slab %d row 24" % r, got[r, 24], hoisted_reference(rig14.o, big[24], elt, rig14.key(elt)))
    assert rig14.g.route("keyswitch", 4, 5) == LEAN
    for off in range(0, 25, 5):
        _same("rows %d..%d, fat against lean" % (off, off + 4), got[:, off:off + 5], rig14.g.apply_galois_hoisted(big[off:off + 5], e))


def test_split14_fat_front_on_both_lanes(rig14):
    """50 ciphertexts: two lanes, chunks of 25, cc * nl = 100 > 96 on each.  Three rows against the reference, every row against the
    same rows in calls of five (block-wise front, one lane)."""
    e = [rig14.elts[1], rig14.elts[2]]
    big = np.concatenate([rig14.inputs(4), _random_cts(rig14.primes, 4, rig14.n, 45, np.random.default_rng(50))])
    assert rig14.g.route("keyswitch", 4, 50) == "split14 front=fat pack=1 main=split4"
    got = rig14.g.apply_galois_hoisted(big, e)
    for r, elt in enumerate(e):
        _same("two-lane fat slab %d row 1" % r, got[r, 1], rig14.want(4, 1, elt))
        for row in (24, 49):  # the last row of either chunk
            _same("two-lane fat slab %d row %d" % (r, row), got[r, row], hoisted_reference(rig14.o, big[row], elt, rig14.key(elt)))
    for off in range(0, 50, 5):
        _same("rows %d..%d, fat against lean" % (off, off + 4), got[:, off:off + 5], rig14.g.apply_galois_hoisted(big[off:off + 5], e))


@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_PACK": "1"}, "split14 front=lean pack=0 main=split4"),
    ({"ABC_HIP_NO_KEY_TWIN": "1"}, LEAN),  # the permuted key is semantics: it exists whatever this switch says
    ({"ABC_HIP_MAIN_TWO_PER_CU": "1"}, LEAN),
    ({"ABC_HIP_LEAN_LIMIT": "0"}, "split14 front=fat pack=1 main=split4"),
    ({"ABC_HIP_NO_SPLIT4": "1"}, "split14 front=lean pack=0 main=split3"),
    ({"ABC_HIP_NO_SPLIT": "1"}, "lds_fp"),
    ({"ABC_HIP_NO_FUSED": "1"}, "generic front=plain"),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else None)
def test_split14_switch_variants(rig14, env, route):
    e = rig14.elts
    with _env(rig14.g, env):
        for level in (4, 3):
            assert rig14.g.route("keyswitch", level, 3) == route
            rig14.check(" ".join(env), level, 3, [e[0], e[2], e[0]])


def test_split14_extreme_residues(rig14):
    rng = np.random.default_rng(14)
    ex = np.stack([_extreme_ct(rig14.primes, 4, rig14.n, rng) for _ in range(2)])
    got = rig14.g.apply_galois_hoisted(ex, rig14.elts[:2] + rig14.elts[4:])
    for r, elt in enumerate(rig14.elts[:2] + rig14.elts[4:]):
        for row in range(2):
            _same("extreme residues elt %d row %d" % (elt, row), got[r, row], hoisted_reference(rig14.o, ex[row], elt, rig14.key(elt)))


def test_one_element(rig14):
    assert rig14.g.route("keyswitch", 4, 2) == LEAN
    rig14.check("one element", 4, 2, [rig14.elts[1]])


# ---- every other scheme, ring and chain the key switch supports ----
OTHERS = {  # name: (scheme, N, chain bits or None for BFVDefault(N), steps, level, route)
    "ckks14_7limbs": ("ckks", N14, [50] + [40] * 5 + [50], (1, None), 6, "split14 front=lean pack=0 main=split3"),
    "ckks14_60bit": ("ckks", N14, [60, 40, 40, 60], (1, -1), 3, "isplit14 guard=1 fpmask=0x6"),
    "ckks15": ("ckks", 1 << 15, [50, 40, 40, 50], (1, None), 3, "gsplit15"),
    "ckks10": ("ckks", 1 << 10, [50, 40, 40, 50], (1, -3), 3, "lds_fp"),
    "bfv4096": ("bfv", 4096, None, (1, -2, None), 2, "lds_fp"),
    "bfv16384": ("bfv", N14, None, (1, None), 8, "bsplit14 pass0=per_target"),  # coefficient form: sign flips
}


@pytest.mark.parametrize("name", list(OTHERS))
def test_other_rings_and_chains(name, oracle_mod, capi):
    scheme, n, bits, steps, level, route = OTHERS[name]
    if scheme == "ckks":
        rig = Rig(oracle_mod, capi, oracle_mod.CKKS, n, oracle_mod.create_primes(n, bits), steps, count=2)
    else:
        rig = Rig(oracle_mod, capi, oracle_mod.BFV, n, oracle_mod.default_bfv_primes(n), steps, t=oracle_mod.plain_modulus_batching(n, 20), count=2)
    try:
        assert rig.L == level
        assert rig.g.route("keyswitch", level, 2) == route
        rig.check(name, level, 2, rig.elts)
        if scheme == "ckks" and level > 1:
            rig.check(name + " one level down", level - 1, 2, rig.elts[:2])
    finally:
        rig.close()


def test_bfv_hoisted_rotation_decrypts_to_the_rotated_slots(oracle_mod, capi):
    """a real encryption: the hoisted ciphertext decodes to the rotated rows and keeps the regular rotation's noise budget within 1 bit"""
    n = 4096
    rig = Rig(oracle_mod, capi, oracle_mod.BFV, n, oracle_mod.default_bfv_primes(n), (1, -2, None), t=oracle_mod.plain_modulus_batching(n, 20), count=1)
    try:
        o = rig.o
        vals = np.random.default_rng(3).integers(-1000, 1000, size=n)
        ct = o.encrypt(o.encode(vals), 11)
        got = rig.g.apply_galois_hoisted(ct, rig.elts)
        rows = vals.reshape(2, n // 2)
        for r, want in enumerate([np.roll(rows, -1, axis=1), np.roll(rows, 2, axis=1), rows[::-1]]):
            assert np.array_equal(o.decode(o.decrypt(got[r])).reshape(2, n // 2), want), r
            assert abs(o.noise_budget(got[r]) - o.noise_budget(o.apply_galois(ct, rig.elts[r]))) <= 1
    finally:
        rig.close()


# ---- rotation steps ----
def test_rotate_hoisted_steps_zero_and_missing_key(rig14, capi):
    g, x = rig14.g, rig14.inputs(3)[:2]
    assert g.elt_from_step(1) == rig14.elts[0] and g.elt_from_step(-1) == rig14.elts[1]
    got = g.rotate_hoisted(x, [1, 0, -1])
    _same("step 1", got[0], g.apply_galois_hoisted(x, [rig14.elts[0]])[0])
    _same("step 1, reference", got[0, 1], rig14.want(3, 1, rig14.elts[0]))
    _same("step 0 copies the input", got[1], x)
    _same("step -1", got[2, 0], rig14.want(3, 0, rig14.elts[1]))
    # step 3 has no key of its own: nothing of the call is enqueued, whatever comes before it in the list
    sentinel = np.full((3,) + x.shape, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    d_in, d_out = g.upload(x), g.upload(sentinel)
    steps = (C.c_int * 3)(1, 0, 3)
    with pytest.raises(capi.AbcHipError, match="Galois key not present"):
        g.op("rotate_hoisted", d_in.ptr, d_out.ptr, 3, steps, 3, C.c_size_t(2))
    g.sync()
    _same("output untouched", g.download(d_out, sentinel.shape), sentinel)
    with pytest.raises(capi.AbcHipError, match="step count too large"):
        g.rotate_hoisted(x, [1, rig14.n // 2])
    d_in.free(); d_out.free()


# ---- refused calls, empty calls ----
def test_refused_and_empty_calls(rig14, capi):
    g, n, e = rig14.g, rig14.n, rig14.elts
    x = rig14.inputs(4)[:2]
    words = x.size
    sentinel = np.full((2,) + x.shape, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    d_in, d_out = g.upload(x), g.upload(sentinel)
    held = g.held_buffers()

    def call(d_i, d_o, nl, elts, count):
        arr = (C.c_uint32 * max(len(elts), 1))(*elts)
        g.op("apply_galois_hoisted", d_i, d_o, nl, arr, len(elts), C.c_size_t(count))

    for what, elts, msg in [("even", [e[0], 4], "odd and below 2N"), ("too large", [e[0], 2 * n + 1], "odd and below 2N"),
                            ("no key", [e[0], 5], "Galois key not present")]:
        with pytest.raises(capi.AbcHipError, match=msg):
            call(d_in.ptr, d_out.ptr, 4, elts, 2)
    for nl in (0, 5, -1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            call(d_in.ptr, d_out.ptr, nl, e[:2], 2)
        with pytest.raises(capi.AbcHipError):
            g.route("keyswitch", nl, 2)
    # overlap: the same buffer; an output that starts inside the input; an input inside the output's second slab
    both = g.alloc(3 * words * 8)
    at = lambda k: C.c_void_p(both.ptr.value + k * 8)  # noqa: E731
    for d_i, d_o in [(at(0), at(0)), (at(0), at(words - 1)), (at(words + 1), at(0)), (at(2 * words - 1), at(0))]:
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(d_i, d_o, 4, e[:2], 2)
    g.op("memcpy_d2d", at(2 * words), d_in.ptr, C.c_size_t(words * 8))
    call(at(2 * words), at(0), 4, e[:2], 2)  # adjacent, not overlapping: input right behind the two slabs
    got = g.download(both, (3,) + x.shape)
    _same("adjacent buffers, slab 0", got[0, 1], rig14.want(4, 1, e[0]))
    _same("adjacent buffers, slab 1", got[1, 0], rig14.want(4, 0, e[1]))
    _same("adjacent buffers, input", got[2], x)
    # nothing to do: success, nothing written
    call(d_in.ptr, d_out.ptr, 4, [], 2)
    call(d_in.ptr, d_out.ptr, 4, e[:2], 0)
    g.sync()
    _same("refused and empty calls wrote nothing", g.download(d_out, sentinel.shape), sentinel)
    assert g.apply_galois_hoisted(x, []).shape == (0,) + x.shape
    assert g.held_buffers() == held
    for b in (d_in, d_out, both):
        b.free()


# ---- recorded circuits ----
def _record(g, d_in, d_out, level, elts, count):
    arr = (C.c_uint32 * len(elts))(*elts)

    def circuit():
        g.op("apply_galois_hoisted", d_in.ptr, d_out.ptr, level, arr, len(elts), C.c_size_t(count))
    circuit()  # eager pass first: sizes the scratch, builds the permuted keys and their mirrors
    g.sync()
    g.graph_begin()
    circuit()
    return g.graph_end()


def test_recorded_call_follows_reloaded_keys(rig14, oracle_mod):
    """capture one hoisted call, replay; load new keys for the same elements into the same device buffers, replay: the permuted
    keys and their fp64 twins were rewritten in place, and the recorded circuit reads them"""
    g, e = rig14.g, [rig14.elts[0], rig14.elts[4], rig14.elts[2]]
    x = rig14.inputs(4)[:2]
    d_in, d_out = g.upload(x), g.alloc(3 * x.nbytes)
    held = g.held_buffers()
    exe = _record(g, d_in, d_out, 4, e, 2)
    eager = g.download(d_out, (3,) + x.shape)
    for r in range(3):
        _same("eager slab %d" % r, eager[r, 1], rig14.want(4, 1, e[r]))
    g.op("memcpy_h2d", d_out.ptr, np.zeros_like(eager).ctypes.data_as(C.c_void_p), C.c_size_t(eager.nbytes))
    g.graph_launch(exe)
    _same("replay", g.download(d_out, eager.shape), eager)
    o2 = oracle_mod.Oracle(oracle_mod.CKKS, rig14.n, rig14.primes)
    o2.keygen(0x402, elts=rig14.elts)
    try:
        g.load_keys(galois={el: o2.galois_key(el) for el in e})
        g.graph_launch(exe)
        got = g.download(d_out, eager.shape)
        for r in range(3):
            for row in range(2):
                _same("replay under the new keys, slab %d row %d" % (r, row), got[r, row], hoisted_reference(o2, x[row], e[r]))
    finally:
        g.graph_destroy(exe)
        g.load_keys(galois={el: rig14.o.galois_key(el) for el in e})  # the module's rig goes on with its own keys
    assert g.held_buffers() == held
    rig14.check("after the keys came back", 4, 2, e)
    d_in.free(); d_out.free()


def test_recorded_call_follows_keygen(oracle_mod, capi):
    """the same with keys generated on the device: keygen(seed) rewrites every key and every mirror in place.  BFVDefault(4096), whose
    default key set the oracle generates quickly; the first three default elements are 2N - 1, 3 and 3^-1."""
    n = 4096
    o = oracle_mod.Oracle.bfv_default(n)
    e = [2 * n - 1, o.elt_from_step(1), o.elt_from_step(-1)]
    o.keygen(0x501, elts=e)  # the device's default list starts with these three, in this order
    g = capi.Context.bfv_default(n)
    try:
        g.keygen(0x501)
        x = _random_cts(o.primes, o.L, n, 2, np.random.default_rng(5))
        d_in, d_out = g.upload(x), g.alloc(3 * x.nbytes)
        held = g.held_buffers()
        exe = _record(g, d_in, d_out, o.L, e, 2)
        eager = g.download(d_out, (3,) + x.shape)
        for r in range(3):
            _same("eager slab %d" % r, eager[r, 0], hoisted_reference(o, x[0], e[r]))
        g.graph_launch(exe)
        _same("replay", g.download(d_out, eager.shape), eager)
        g.keygen(0x502)
        o.keygen(0x502, elts=e)
        g.graph_launch(exe)
        got = g.download(d_out, eager.shape)
        for r in range(3):
            for row in range(2):
                _same("replay after keygen, slab %d row %d" % (r, row), got[r, row], hoisted_reference(o, x[row], e[r]))
        g.graph_destroy(exe)
        assert g.held_buffers() == held
        d_in.free(); d_out.free()
    finally:
        g.close()
