"""GPU parity at every limb count a chain can reach: both sides of every limb-count boundary of the route table (abc_route.hpp).

abc_hip_ctx_create accepts 2 .. 16 primes, and the rows of the route table are cut by limb count: N = 2^14 CKKS takes split4 up to
five limbs, split3 (the runtime-nl kernels, 12 / 13 wavefronts) up to twelve and the LDS-resident kernels above; a prime above 2^50
moves the cut to seven; N = 2^15 runs nl + 1 wavefronts in its deep main kernel; BFV instantiates its split key switch per digit
count.  test_gpu_paths.py runs the shapes of the benchmark configurations (at most nine limbs); this file sweeps the rest.

Conventions of test_gpu_paths.py: word-for-word comparison (_same), inputs with runs of q-1, (q+-1)/2 and 0 next to random residues
(_extreme_ct), the expected route strings written out here (never computed by the library) and asserted before any parity check,
keys loaded from the oracle.  The oracle makes Galois keys only for the steps used (rotations by 1 and 7 = 8 - 1; BFV: 1 and
-5 = -4 - 1), and its results are cached per (chain, level), so a variant costs device time only.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s: got %d want %d" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _extreme_ct(primes, nl, n, rng):
    """a 2-component 'ciphertext' whose residues are drawn from {0, 1, (q-1)/2, (q+1)/2, q-2, q-1} and random values"""
    ct = np.empty((2, nl, n), dtype=np.uint64)
    for j in range(nl):
        q = primes[j]
        pool = np.array([0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
        pick = rng.integers(0, 8, size=(2, n))
        rnd = rng.integers(0, q, size=(2, n), dtype=np.uint64)
        ct[:, j, :] = np.where(pick < 6, pool[np.minimum(pick, 5)], rnd)
    ct[0, :, : n // 4] = np.array(primes[:nl], dtype=np.uint64)[:, None] - 1  # long runs of q-1
    return ct


CKKS_STEPS = (1, 8, -1)   # rotate 1; rotate 7 = 8 - 1 (NAF)
BFV_STEPS = (1, -4, -1)   # rotate 1; rotate -5 = -4 - 1

CHAINS = {  # name: (N, key-prime widths)
    "A": (1 << 14, [50] + [40] * 14 + [50]),   # every prime below 2^50: split4 / split3 / lds_fp
    "B": (1 << 14, [60] + [45] * 14 + [60]),   # guarded integer butterflies, fp64 middle limbs up to seven limbs
    "C": (1 << 14, [55] + [52] * 14 + [55]),   # unguarded, lazy 128-bit inner product over up to 15 digits
    "D": (1 << 14, [57] + [45] * 14 + [57]),   # unguarded, inner product reduced per term
    "E": (1 << 15, [50] + [40] * 14 + [50]),   # gsplit15: the deep main kernel at 16 wavefronts
    "F": (1 << 15, [60] + [40] * 14 + [60]),   # isplit15
    "S40-1024": (1 << 10, [40] * 15 + [41]),   # the LDS-resident templates at LB = 10 and 12
    "S58-1024": (1 << 10, [58] * 15 + [59]),
    "S40-4096": (1 << 12, [40] * 15 + [41]),
    "S58-4096": (1 << 12, [58] * 15 + [59]),
}


class _Chain:
    """one oracle with keys, the two inputs (random residues, extreme residues) at every level, and its cached results"""

    def __init__(self, om, name):
        self.name = name
        self.n, bits = CHAINS[name]
        self.primes = om.create_primes(self.n, bits)
        self.o = om.Oracle(om.CKKS, self.n, self.primes)
        self.o.keygen(0xDEE9 + len(name), elts=[self.o.elt_from_step(s) for s in CKKS_STEPS])
        self.L = len(self.primes) - 1
        rng = np.random.default_rng(self.n + sum(bits))
        x = np.stack([rng.integers(0, q, size=(2, self.n), dtype=np.uint64) for q in self.primes[:self.L]], axis=1)
        self._in = {self.L: (x, _extreme_ct(self.primes, self.L, self.n, rng))}
        self._want = {}

    def inputs(self, level):
        if level not in self._in:
            x, y = self.inputs(level + 1)
            self._in[level] = (self.o.mod_switch(x), self.o.mod_switch(y))
        return self._in[level]

    def want(self, level, what):
        key = (level, what)
        if key not in self._want:
            o, (x, y) = self.o, self.inputs(level)
            if what == "mul_xy":
                r = o.relinearize(self.want(level, "tensor_xy"))
            elif what == "tensor_xy":
                r = o.multiply(x, y)
            elif what == "mul_yy":
                r = o.mul_relin(y, y)
            elif what == "rot1_y":
                r = o.rotate(y, 1)
            elif what == "rot7_x":
                r = o.rotate(x, 7)
            elif what == "rot1_x":
                r = o.rotate(x, 1)
            elif what == "rescale_y":
                r = o.rescale(y)
            elif what == "rescale_x":
                r = o.rescale(x)
            elif what == "ks_y1":
                r = o.keyswitch(y[1], o.relin_key())
            else:
                raise KeyError(what)
            r.setflags(write=False)
            self._want[key] = r
        return self._want[key]


@pytest.fixture(scope="module")
def chains(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Chain(oracle_mod, name)
        return cache[name]
    yield get
    cache.clear()


@contextlib.contextmanager
def _env(settings):
    old = {k: os.environ.get(k) for k in settings}
    os.environ.update(settings)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def device(capi):
    """the device context of (chain, switches): the last one stays open, so the levels of one variant share one key upload.  The
    ABC_HIP_* switches are read when a context is created."""
    live = {}

    def get(ch, env=()):
        key = (ch.name, tuple(sorted(dict(env).items())))
        if live.get("key") != key:
            if live.get("g") is not None:
                live.pop("g").close()
            with _env(dict(env)):
                g = capi.Context(capi.CKKS, ch.n, ch.primes)
            o = ch.o
            g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
            live["key"], live["g"] = key, g
        return live["g"]
    yield get
    if live.get("g") is not None:
        live["g"].close()


def _check_routes(g, level, routes, counts=(1, 3)):
    mul, rot, resc, ks = routes
    for count in counts:
        assert g.route("mul_relin", level, count) == mul, (level, count)
        assert g.route("rotate", level, count) == rot, (level, count)
        assert g.route("keyswitch", level, count) == ks, (level, count)
        if level >= 2 and resc is not None:
            assert g.route("rescale", level, count) == resc, (level, count)


def _check_level(g, ch, level, routes, tag, every_op=True):
    """routes first, then the operations of one level against the oracle"""
    _check_routes(g, level, routes)
    x, y = ch.inputs(level)
    tag = "%s %s nl=%d" % (ch.name, tag, level)
    _same(tag + " mul_relin random x extreme", g.mul_relin(x, y), ch.want(level, "mul_xy"))
    _same(tag + " mul_relin extreme x extreme", g.mul_relin(y, y), ch.want(level, "mul_yy"))
    _same(tag + " rotate 1", g.rotate(y, 1), ch.want(level, "rot1_y"))
    _same(tag + " rotate 7 (NAF)", g.rotate(x, 7), ch.want(level, "rot7_x"))
    if level >= 2 and routes[2] is not None:
        _same(tag + " rescale", g.rescale(y), ch.want(level, "rescale_y"))
    if not every_op:
        return
    _same(tag + " relinearize", g.relinearize(ch.want(level, "tensor_xy")), ch.want(level, "mul_xy"))
    _same(tag + " keyswitch", g.keyswitch(y[1], 0), ch.want(level, "ks_y1"))
    got = g.mul_relin(np.stack([x, y, x]), np.stack([y, y, y]))
    for row, what in enumerate(("mul_xy", "mul_yy", "mul_xy")):
        _same(tag + " batch of 3, row %d" % row, got[row], ch.want(level, what))
    if level >= 2 and routes[2] is not None:
        _same(tag + " batch of 3 rescale, middle row", g.rescale(np.stack([x, y, x]))[1], ch.want(level, "rescale_y"))


# ---------------------------------------------------------------------------------------------------------------------
# chain A (CKKS, N = 2^14, every prime below 2^50): (mul_relin, rotate, rescale, keyswitch / relinearize), for 1 and 3 ciphertexts
# ---------------------------------------------------------------------------------------------------------------------
_S4 = "split14 front=%s pack=1 main=split4"
_S3 = "split14 front=%s pack=0 main=split3"


def _routes_split(level, front="lean"):
    if level <= 5:
        return (_S4 % front, "fold " + _S4 % front, "fp", _S4 % front)
    if level <= 12:
        return (_S3 % front, "fold " + _S3 % front, "fp", _S3 % front)
    return ("lds_fp", "permute lds_fp", "fp", "lds_fp")  # the LDS-resident kernels have no gather: the permutation runs first


def _routes_int(level):
    if level <= 7:
        return ("isplit14 guard=0 fpmask=0x0", "fold isplit14 guard=0 fpmask=0x0", "mixed fpmask=0x0", "isplit14 guard=0 fpmask=0x0")
    return ("lds_int guard=0 lazy=1", "permute lds_int guard=0 lazy=1", "mixed fpmask=0x0", "lds_int guard=0 lazy=1")


A_VARIANTS = {  # switches, routes at a level
    "no_split": ({"ABC_HIP_NO_SPLIT": "1"}, lambda level: ("lds_fp", "permute lds_fp", "fp", "lds_fp")),
    "no_fp64": ({"ABC_HIP_NO_FP64": "1"}, _routes_int),
    "no_fused": ({"ABC_HIP_NO_FUSED": "1"}, lambda level: ("generic mul=tensor ks=generic front=plain", "permute generic front=plain",
                                                            "generic", "generic front=plain")),
    "no_key_twin": ({"ABC_HIP_NO_KEY_TWIN": "1"}, _routes_split),  # differs in the key mirror, not in the route
    "no_lean_front": ({"ABC_HIP_NO_LEAN_FRONT": "1"}, lambda level: _routes_split(level, "fat")),
}
A_VARIANT_LEVELS = (15, 13, 12, 8, 7, 6, 5, 1)


@pytest.mark.parametrize("level", range(15, 0, -1))
def test_ckks14_chain_a_every_level(level, chains, device):
    """N = 2^14, [50] + [40]*14 + [50], levels 15 .. 1: split4 (<= 5), split3 with the runtime-nl special / main kernels (6 .. 12),
    LDS-resident above -- where the rotation must permute first"""
    ch = chains("A")
    _check_level(device(ch), ch, level, _routes_split(level), "default")


def test_ckks14_chain_a_rotate_in_place_above_the_split(chains, device):
    ch = chains("A")
    g = device(ch)
    assert g.route("rotate", 13, 1, in_place=True) == "permute lds_fp"
    assert g.route("rotate", 12, 1, in_place=True) == "permute " + _S3 % "lean"
    for level in (13, 12):
        y = ch.inputs(level)[1]
        d = g.upload(y[None])
        g.op("rotate", d.ptr, d.ptr, level, 1, C.c_size_t(1))
        got = g.download(d, (1,) + y.shape)[0]
        d.free()
        _same("A in-place rotate 1 nl=%d" % level, got, ch.want(level, "rot1_y"))


@pytest.mark.parametrize("level,count", [(12, 18), (6, 34)])
def test_ckks14_chain_a_fat_front_deep(level, count, chains, device):
    """more than 96 (ciphertext, limb) pairs per chunk (two lanes: 9 x 12 = 108, 17 x 6 = 102): the 139 KiB tensor / operand kernel
    in front of the runtime-nl kernels"""
    ch = chains("A")
    g = device(ch)
    _check_routes(g, level, (_S3 % "fat", "fold " + _S3 % "fat", None, _S3 % "fat"), counts=(count,))
    x, y = ch.inputs(level)
    a = np.stack([x if i % 2 == 0 else y for i in range(count)])
    got = g.mul_relin(a, np.stack([y] * count))
    rot = g.rotate(a, 1)
    for row in (0, count // 2, count - 1):  # first chunk, the first row of the second lane's chunk, the last row
        odd = row % 2
        _same("A fat front nl=%d mul_relin row %d" % (level, row), got[row], ch.want(level, "mul_yy" if odd else "mul_xy"))
        _same("A fat front nl=%d rotate row %d" % (level, row), rot[row], ch.want(level, "rot1_y" if odd else "rot1_x"))


@pytest.mark.parametrize("level", A_VARIANT_LEVELS)
@pytest.mark.parametrize("variant", list(A_VARIANTS))
def test_ckks14_chain_a_variants(variant, level, chains, device):
    ch = chains("A")
    env, routes = A_VARIANTS[variant]
    _check_level(device(ch, env), ch, level, routes(level), variant, every_op=False)


@pytest.mark.parametrize("level", [12, 13])
def test_ckks14_chain_a_ragged_chunks(level, chains, device):
    """seven ciphertexts in chunks of two (2, 2, 2, 1 on one lane), on both sides of the split3 / lds_fp cut; every row"""
    ch = chains("A")
    g = device(ch, {"ABC_HIP_CHUNK": "2"})
    _check_routes(g, level, _routes_split(level), counts=(7,))
    x, y = ch.inputs(level)
    a = np.stack([x if i % 2 == 0 else y for i in range(7)])
    got = g.mul_relin(a, np.stack([y] * 7))
    rot = g.rotate(a, 1)
    for row in range(7):
        odd = row % 2
        _same("A chunked nl=%d mul_relin row %d" % (level, row), got[row], ch.want(level, "mul_yy" if odd else "mul_xy"))
        _same("A chunked nl=%d rotate row %d" % (level, row), rot[row], ch.want(level, "rot1_y" if odd else "rot1_x"))


# ---------------------------------------------------------------------------------------------------------------------
# N = 2^14 with a prime above 2^50: the integer split kernels up to seven limbs, the LDS-resident integer kernels above
# ---------------------------------------------------------------------------------------------------------------------
_MID_FP = {15: "0x7ffe", 12: "0xffe", 8: "0xfe", 7: "0x7e"}  # limbs 1 .. nl-1 take the fp64 butterflies


def _routes_wide(name, level):
    guard, lazy, mask = {"B": (1, 0, _MID_FP[level]), "C": (0, 1, "0x0"), "D": (0, 0, _MID_FP[level])}[name]
    resc = "mixed fpmask=" + mask
    if level <= 7:
        s = "isplit14 guard=%d fpmask=%s" % (guard, mask)
        return (s, "fold " + s, resc, s)
    s = "lds_int guard=%d lazy=%d" % (guard, lazy)
    return (s, "permute " + s, resc, s)


@pytest.mark.parametrize("level", [15, 12, 8, 7])
@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_ckks14_wide_chains_deep(name, level, chains, device):
    ch = chains(name)
    _check_level(device(ch), ch, level, _routes_wide(name, level), "default", every_op=False)


# ---------------------------------------------------------------------------------------------------------------------
# the same LDS-resident templates on small rings
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [15, 9, 1])
@pytest.mark.parametrize("name", ["S40-1024", "S58-1024", "S40-4096", "S58-4096"])
def test_ckks_small_rings_deep(name, level, chains, device):
    ch = chains(name)
    if name.startswith("S40"):
        routes = ("lds_fp", "permute lds_fp", "fp", "lds_fp")
    else:
        routes = ("lds_int guard=1 lazy=0", "permute lds_int guard=1 lazy=0", "mixed fpmask=0x0", "lds_int guard=1 lazy=0")
    _check_level(device(ch), ch, level, routes, "default", every_op=False)


# ---------------------------------------------------------------------------------------------------------------------
# N = 2^15
# ---------------------------------------------------------------------------------------------------------------------
_F_MASK = {15: "0x7ffe", 12: "0xffe", 10: "0x3fe", 8: "0xfe", 7: "0x7e"}


def _check_level15(g, ch, level, routes, tag):
    _check_routes(g, level, routes)
    x, y = ch.inputs(level)
    tag = "%s %s nl=%d" % (ch.name, tag, level)
    _same(tag + " mul_relin random x extreme", g.mul_relin(x, y), ch.want(level, "mul_xy"))
    _same(tag + " rotate 1", g.rotate(y, 1), ch.want(level, "rot1_y"))
    _same(tag + " rotate 7 (NAF)", g.rotate(x, 7), ch.want(level, "rot7_x"))
    if level == ch.L:
        _check_routes(g, level, routes, counts=(5,))
        got = g.mul_relin(np.stack([x, y, x, y, x]), np.stack([y] * 5))
        for row in range(5):
            _same(tag + " batch of 5, row %d" % row, got[row], ch.want(level, "mul_yy" if row % 2 else "mul_xy"))


@pytest.mark.parametrize("level", [15, 12, 10, 8, 7])
@pytest.mark.parametrize("name", ["E", "F"])
def test_ckks15_deep(name, level, chains, device):
    """E: k_gsplit_main_deep runs nl + 1 wavefronts (16 at nl = 15, its 1024-thread limit); F: the integer deep kernels"""
    ch = chains(name)
    s = "gsplit15" if name == "E" else "isplit15 guard=1 fpmask=" + _F_MASK[level]
    _check_level15(device(ch), ch, level, (s, "fold " + s, None, s), "default")


@pytest.mark.parametrize("level", [15, 10])
def test_ckks15_deep_generic(level, chains, device):
    ch = chains("E")
    routes = ("generic mul=tensor ks=generic front=fp", "permute generic front=fp", None, "generic front=fp")
    _check_level15(device(ch, {"ABC_HIP_NO_GSPLIT": "1"}), ch, level, routes, "no_gsplit")


# ---------------------------------------------------------------------------------------------------------------------
# BFV (top level only: the ABI requires nl = L): the per-digit-count instantiations of the split key switch, the LDS-resident key
# switch above eight digits, the BEHZ multiply at limb counts other than 4, 8 and 15
# ---------------------------------------------------------------------------------------------------------------------
_B14 = "bsplit14 pass0=per_target"
BFV_CASES = {  # id: (N, widths, (mul_relin, rotate, multiply, relinearize))
    "N16384-wide-55x12-56": (1 << 14, [55] * 12 + [56],  # 56 > 55: not lazy
                             ("generic mul=behz ks=lds_int guard=0 lazy=0", "permute lds_int guard=0 lazy=0", "behz", "lds_int guard=0 lazy=0")),
    "N16384-wide-58x15-59": (1 << 14, [58] * 15 + [59],
                             ("generic mul=behz ks=lds_int guard=1 lazy=0", "permute lds_int guard=1 lazy=0", "behz", "lds_int guard=1 lazy=0")),
}
for _L in (1, 2, 3, 5, 6, 7):
    BFV_CASES["N16384-L%d" % _L] = (1 << 14, [48] * _L + [49], ("generic mul=behz ks=" + _B14, "fold " + _B14, "behz", _B14))
    BFV_CASES["N8192-L%d" % _L] = (1 << 13, [48] * _L + [49], ("generic mul=behz ks=bsplit_big", "fold bsplit_big", "behz", "bsplit_big"))
for _L in (9, 12, 15):
    BFV_CASES["N16384-L%d" % _L] = (1 << 14, [48] * _L + [49], ("generic mul=behz ks=lds_fp", "permute lds_fp", "behz", "lds_fp"))
BFV_CASES["N8192-L9"] = (1 << 13, [48] * 9 + [49], ("generic mul=behz ks=lds_fp", "permute lds_fp", "behz", "lds_fp"))
for _n, _L in ((1 << 15, 3), (1 << 15, 7), (1 << 16, 5)):
    BFV_CASES["N%d-L%d" % (_n, _L)] = (_n, [48] * _L + [49], ("generic mul=behz ks=bsplit_big", "fold bsplit_big", "behz", "bsplit_big"))


def _bfv_pair(oracle_mod, capi, n, bits, env=()):
    primes = oracle_mod.create_primes(n, bits)
    t = oracle_mod.plain_modulus_batching(n, 20)
    o = oracle_mod.Oracle(oracle_mod.BFV, n, primes, t)
    o.keygen(0xBF5 + len(bits), elts=[o.elt_from_step(s) for s in BFV_STEPS])
    with _env(dict(env)):
        g = capi.Context(capi.BFV, n, primes, t)
    g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
    rng = np.random.default_rng(n + len(bits))
    c1 = o.encrypt(o.encode(oracle_mod.expand_vector([3, 1, 4, 1, 5], n)), 9)
    c2 = o.encrypt(o.encode(oracle_mod.expand_vector([2, 7, 1, 8, 2], n)), 10)
    return o, g, c1, c2, _extreme_ct(primes, len(bits) - 1, n, rng)


@pytest.mark.parametrize("case", list(BFV_CASES))
def test_bfv_digit_counts(case, oracle_mod, capi):
    n, bits, routes = BFV_CASES[case]
    L = len(bits) - 1
    o, g, c1, c2, ex = _bfv_pair(oracle_mod, capi, n, bits)
    for count in (1, 3):
        assert (g.route("mul_relin", L, count), g.route("rotate", L, count), g.route("multiply", L, count),
                g.route("relinearize", L, count)) == routes, (case, count)
    t3 = o.multiply(c1, c2)
    want = o.relinearize(t3)
    got = g.mul_relin(c1, c2)
    _same(case + " bfv mul_relin", got, want)
    if L >= 2:  # the chain itself: enough room for one product of 20-bit plaintexts
        assert list(o.decode(o.decrypt(got))[:5]) == [6, 7, 4, 8, 10]
    _same(case + " bfv mul_relin extreme x fresh", g.mul_relin(ex, c1), o.mul_relin(ex, c1))
    _same(case + " bfv multiply (size 3)", g.multiply(c1, c2), t3)
    _same(case + " bfv relinearize", g.relinearize(t3), want)
    _same(case + " bfv rotate 1 extreme", g.rotate(ex, 1), o.rotate(ex, 1))
    _same(case + " bfv rotate -5 (NAF) extreme", g.rotate(ex, -5), o.rotate(ex, -5))
    g.close()


@pytest.mark.parametrize("lanes", ["two_lanes", "one_lane"])
def test_bfv14_five_digits_batch_of_30(lanes, oracle_mod, capi):
    """30 ciphertexts of five digits.  On two lanes that is 15 per chunk, 75 (ciphertext, digit) pairs: pass 0 per target; on one
    lane one chunk of 150 pairs, above the limit of 128: pass 0 per limb."""
    n, bits = 1 << 14, [48] * 5 + [49]
    o, g, c1, c2, ex = _bfv_pair(oracle_mod, capi, n, bits, {"ABC_HIP_LANES": "1"} if lanes == "one_lane" else {})
    pass0 = "bsplit14 pass0=per_limb" if lanes == "one_lane" else "bsplit14 pass0=per_target"
    assert g.route("mul_relin", 5, 30) == "generic mul=behz ks=" + pass0
    assert g.route("rotate", 5, 30) == "fold " + pass0
    big = np.stack([c1 if i % 3 else ex for i in range(30)])
    rot = g.rotate(big, -5)
    mr = g.mul_relin(big, np.stack([c2] * 30))
    want = {"rot_ex": o.rotate(ex, -5), "rot_c1": o.rotate(c1, -5), "mul_ex": o.mul_relin(ex, c2), "mul_c1": o.mul_relin(c1, c2)}
    for row in (0, 1, 14, 15, 29):
        kind = "c1" if row % 3 else "ex"
        _same("bfv batch of 30 rotate row %d" % row, rot[row], want["rot_" + kind])
        _same("bfv batch of 30 mul_relin row %d" % row, mr[row], want["mul_" + kind])
    g.close()
