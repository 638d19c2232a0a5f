"""abc_hip_diag_matvec_bsgs_rescale on the device, word for word against tests/plain_sum_rescale_spec.py: the CPU oracle's rotate for the
baby steps at nl, its multiply_plain, add and ONE rescale for every inner sum, its rotate and add for the giant steps at nl - 1, in
the order the header gives.  The inputs are random residues: every step is exact modular arithmetic, the oracle's own rescale or its
own key switch, so random words check as much as encryptions do, and the rows of D are taken as they come (the last test goes from
encode to decode with pre-rotated rows).  Every routed shape asserts its route string."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plain_sum_rescale_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
FP_CHAIN, HEAD14, MIXED_CHAIN = [50, 40, 40, 50], [50, 40, 40, 40, 50], [60, 40, 40, 60]
POW2_STEPS = (1, 2, 4, 8, 16, -1, -4)  # enough of the default key set for the NAF chains of 3 = 4 - 1 and 12 = 16 - 4
SPLIT14 = "split14 front=lean pack=1 main=split4"
LDS = "permute lds_fp sumrescale=fused permute lds_fp add=separate"


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


def _ints(v):
    return (C.c_int * max(len(v), 1))(*[int(x) for x in v])


class Rig:
    """one CKKS oracle and a device context with the oracle's keys: the default Galois key set (steps None) or keys for `steps` only;
    random ciphertext words per level, 20 rows of random plaintext words encoded for the whole chain, and the references computed so
    far (shared by the tests of a module, never changed)"""

    def __init__(self, om, capi, n, bits, steps=None, seed=0xB565, rows=12):
        primes = om.create_primes(n, bits)
        self.o = o = om.Oracle(om.CKKS, n, primes)
        o.keygen(seed, elts=None if steps is None else sorted({o.elt_from_step(s) for s in steps}))
        self.g = capi.Context(capi.CKKS, n, o.primes)
        self.g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
        self.n, self.primes, self.L = n, list(primes), o.L
        self.rng = np.random.default_rng(n + len(primes))
        self.diags = np.stack([self.rng.integers(0, q, size=(20, n), dtype=np.uint64) for q in primes[: o.L]], axis=1)  # [20][L][N]
        self.diags.setflags(write=False)
        self.rows = rows
        self._x, self._want = {}, {}

    def x(self, nl):
        """[rows][2][nl][N]"""
        if nl not in self._x:
            self._x[nl] = np.stack([self.rng.integers(0, q, size=(self.rows, 2, self.n), dtype=np.uint64) for q in self.primes[:nl]], axis=2)
            self._x[nl].setflags(write=False)
        return self._x[nl]

    def want(self, nl, baby, giant, count):
        k = (nl, tuple(baby), tuple(giant))
        have = self._want.get(k, np.zeros((0, 2, nl - 1, self.n), dtype=np.uint64))
        if len(have) < count:
            more = [spec.diag_matvec_bsgs_rescale(self.o, self.x(nl)[r], self.diags, baby, giant) for r in range(len(have), count)]
            have = np.concatenate([have, np.stack(more)])
            have.setflags(write=False)
            self._want[k] = have
        return have[:count]

    def check(self, tag, nl, baby, giant, count=2):
        got = self.g.diag_matvec_bsgs_rescale(self.x(nl)[:count], self.diags[: len(baby) * len(giant)], baby, giant)
        _same("%s nl=%d baby %s giant %s" % (tag, nl, list(baby), list(giant)), got, self.want(nl, baby, giant, count))

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

    def get(n, bits, steps=None, rows=12):
        k = (n, tuple(bits), steps)
        if k not in made:
            made[k] = Rig(oracle_mod, capi, n, bits, steps, rows=rows)
        return made[k]

    yield get
    for r in made.values():
        r.close()


BABY, GIANT = (0, 1, 2, 3), (0, 4, 8, 12)


# ---- routes ----
@pytest.mark.parametrize("n", [1024, 4096])
def test_lds_rings_default_keys(rigs, n):
    """the default key set: 3 = 4 - 1 and 12 = 16 - 4 are NAF chains, on the baby side at nl and on the giant side at nl - 1"""
    r = rigs(n, FP_CHAIN)
    assert r.g.route("diag_matvec_bsgs_rescale", 3, 3) == LDS
    r.check("lds_fp", 3, BABY, GIANT, 3)
    r.check("lds_fp, rows of L limbs at nl < L", 2, BABY, GIANT, 2)


@pytest.mark.parametrize("nl", [3, 2])
def test_split14(rigs, nl):
    r = rigs(16384, HEAD14, POW2_STEPS, rows=2)
    assert r.g.route("diag_matvec_bsgs_rescale", nl, 2) == "fold " + SPLIT14 + " sumrescale=fused fold " + SPLIT14 + " add=fused"
    r.check("split14", nl, (0, 1, 3), (0, 4, 12))


@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_ROTATE_ADD_FUSION": "1"}, "fold " + SPLIT14 + " sumrescale=fused fold " + SPLIT14 + " add=separate"),
    ({"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"}, "fold " + SPLIT14 + " sumrescale=separate fold " + SPLIT14 + " add=fused"),
    ({"ABC_HIP_NO_PLAIN_MAC_SUM": "1"}, "fold " + SPLIT14 + " sumrescale=separate fold " + SPLIT14 + " add=fused"),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else "")
def test_split14_switches(rigs, env, route):
    r = rigs(16384, HEAD14, POW2_STEPS, rows=2)
    with _env(r.g, env):
        assert r.g.route("diag_matvec_bsgs_rescale", 3, 2) == route
        r.check(" ".join(env), 3, (0, 1, 3), (0, 4, 12))
    assert r.g.route("diag_matvec_bsgs_rescale", 3, 2) == "fold " + SPLIT14 + " sumrescale=fused fold " + SPLIT14 + " add=fused"


def test_mixed_chain(rigs):
    r = rigs(16384, MIXED_CHAIN, (1, 4, -1), rows=2)
    assert r.g.route("diag_matvec_bsgs_rescale", 3, 2) == \
        "fold isplit14 guard=1 fpmask=0x6 sumrescale=fused fold isplit14 guard=1 fpmask=0x2 add=separate"
    r.check("isplit14", 3, (0, 1, 3), (4, 0))


def test_gsplit15(rigs):
    r = rigs(32768, FP_CHAIN, POW2_STEPS, rows=2)
    assert r.g.route("diag_matvec_bsgs_rescale", 3, 2) == "fold gsplit15 sumrescale=separate fold gsplit15 add=fused"
    r.check("gsplit15", 3, (0, 1, 3), (0, 4, 12))


# ---- grids and step lists ----
@pytest.fixture(scope="module")
def keyed10(rigs):
    """N = 2^10 with a key of its own, from the oracle, for every step the lists below use: no NAF chain"""
    return rigs(1024, FP_CHAIN, tuple(range(1, 16)) + (-1, -2, -3, -5, 20, 100))


@pytest.mark.parametrize("baby,giant", [
    (BABY, GIANT),                      # 4 x 4
    ((0, 1, 2, 3, 4, 5, 6), (0,)),      # 7 x 1: one inner sum written straight to d_out, no giant rotation
    ((0,), (0, 1, 2, 3, 4, 5, 6)),      # 1 x 7: no baby rotation
    ((5,), (7,)),                       # 1 x 1 without step 0
    ((0, 1, 2), (0, 3, 6, 9, 12)),      # 3 x 5
    ((1, 2, 3), (4, 8)),                # no step 0 on either side
    ((-1, 0, 1, -3), (-5, 5, 0)),       # negative steps, step 0 in the middle and last: the add kernel
    ((1, 1, 0, 0, 2), (4, 4, 0, 0)),    # duplicates, a repeated giant step of 0
    ((0, 1, 2, 3, 4, 5, 6, 7, 8), (100, 20)),  # nine baby steps: one term through the streaming kernel, eight in the fused pair
], ids=["4x4", "7x1", "1x7", "1x1", "3x5", "no-zero", "negative", "duplicates", "9x2"])
def test_grids_and_step_lists(keyed10, baby, giant):
    assert keyed10.g.route("diag_matvec_bsgs_rescale", 3, 3) == LDS
    keyed10.check("grid", 3, baby, giant, 3)
    with _env(keyed10.g, {"ABC_HIP_NO_PLAIN_SUM_RESCALE_FUSION": "1"}):
        keyed10.check("grid separate", 3, baby, giant, 2)


def test_the_measured_rule_sends_a_small_batch_to_the_separate_route(keyed10):
    with _env(keyed10.g, {FORCE: None}):
        assert keyed10.g.route("diag_matvec_bsgs_rescale", 3, 3) == "permute lds_fp sumrescale=separate permute lds_fp add=separate"
        keyed10.check("rule", 3, BABY, GIANT, 3)
        assert keyed10.g.route("diag_matvec_bsgs_rescale", 3, 1024).startswith("permute lds_fp sumrescale=fused ")


def test_a_naf_step_and_a_step_with_a_key_of_its_own_differ(rigs, keyed10):
    """step 3: a chain 4 - 1 under the default key set, one key switch where the oracle made a key for it; each against its own oracle"""
    default10 = rigs(1024, FP_CHAIN)
    assert default10.o.elt_from_step(3) not in default10.g.galois_elts() and keyed10.o.elt_from_step(3) in keyed10.g.galois_elts()
    default10.check("NAF", 3, (0, 3), (3, 0))
    keyed10.check("own key", 3, (0, 3), (3, 0))


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_groups_and_ragged_last_group(keyed10, lanes):
    """ABC_HIP_CHUNK=2: groups of chunk * lanes ciphertexts -- two up to a batch of eight, which runs on one lane whatever
    ABC_HIP_LANES says, four at eleven on two lanes -- the last one ragged"""
    with _env(keyed10.g, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": lanes}):
        for count in (5, 11):
            keyed10.check("count %d" % count, 3, (0, 1, 2), (0, 3, 6), count)


# ---- device parity ----
def test_the_devices_own_sequence_gives_the_same_words(keyed10):
    """abc_hip_rotate per baby step at nl, abc_hip_multiply_plain_sum_rescale per giant step, abc_hip_rotate_add / abc_hip_add at nl - 1"""
    g, n, nl, L, count = keyed10.g, keyed10.n, 3, keyed10.L, 3
    baby, giant = (0, 1, 2, -3), (4, 0, 8)
    x = np.ascontiguousarray(keyed10.x(nl)[:count])
    oshape = (count, 2, nl - 1, n)
    obytes = int(np.prod(oshape)) * 8
    rows = len(baby) * len(giant)
    d_x, d_d = g.upload(x), g.upload(keyed10.diags[:rows])
    d_rot = [d_x if b == 0 else g.alloc(x.nbytes) for b in baby]
    d_inner, d_acc, d_out = g.alloc(obytes), g.alloc(obytes), g.alloc(obytes)
    try:
        for b, d in zip(baby, d_rot):
            if b:
                g.op("rotate", d_x.ptr, d.ptr, nl, b, C.c_size_t(count))
        for j, s in enumerate(giant):
            plains = [C.c_void_p(d_d.ptr.value + 8 * (j * len(baby) + i) * L * n) for i in range(len(baby))]
            g.op("multiply_plain_sum_rescale", g.term_pointers([d.ptr for d in d_rot]), g.term_pointers(plains), C.c_size_t(0), len(baby), None,
                 d_inner.ptr, 2, nl, C.c_size_t(count))
            if j == 0:
                g.op("rotate", d_inner.ptr, d_acc.ptr, nl - 1, s, C.c_size_t(count))
            elif s == 0:
                g.op("add", d_acc.ptr, d_inner.ptr, d_acc.ptr, 2, nl - 1, C.c_size_t(count))
            else:
                g.op("rotate_add", d_inner.ptr, d_acc.ptr, d_acc.ptr, nl - 1, s, C.c_size_t(count))
        g.op("diag_matvec_bsgs_rescale", d_x.ptr, d_d.ptr, C.c_size_t(L * n), _ints(baby), len(baby), _ints(giant), len(giant), d_out.ptr, nl,
             C.c_size_t(count))
        _same("one call against the sequence of calls", g.download(d_out, oshape), g.download(d_acc, oshape))
        _same("... and the spec", g.download(d_out, oshape), keyed10.want(nl, baby, giant, count))
        _same("the input is left alone", g.download(d_x, x.shape), x)
    finally:
        for b in {id(b): b for b in [d_x, d_d, d_inner, d_acc, d_out] + d_rot}.values():
            b.free()


# ---- refused and empty calls: nothing is written ----
def test_refused_and_empty_calls(rigs, capi):
    r = rigs(1024, FP_CHAIN, (1, 4))  # step 2 has neither a key nor a chain of keys
    g, n, nl, L, count = r.g, r.n, 3, r.L, 2
    x = np.ascontiguousarray(r.x(nl)[:count])
    oshape = (count, 2, nl - 1, n)
    sentinel = np.full(x.shape, SENTINEL, dtype=np.uint64)  # as large as the input: nothing behind the output may be written either
    d_x, d_d, d_o = g.upload(x), g.upload(r.diags[:4]), g.upload(sentinel)
    held = g.held_buffers()
    owords = int(np.prod(oshape))

    def call(baby=(0, 1), giant=(0, 4), src=None, diags=None, stride=L * n, out=None, level=nl, cnt=count, nb=None, ng=None, pb=True, pg=True):
        g.op("diag_matvec_bsgs_rescale", src or d_x.ptr, diags or d_d.ptr, C.c_size_t(stride), _ints(baby) if pb else None,
             len(baby) if nb is None else nb, _ints(giant) if pg else None, len(giant) if ng is None else ng, out or d_o.ptr, level, C.c_size_t(cnt))

    for level in (0, L + 1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            call(level=level)
    with pytest.raises(capi.AbcHipError, match="no limb left to drop"):
        call(level=1)
    with pytest.raises(capi.AbcHipError, match="diag_stride must be at least"):
        call(stride=nl * n - 1)
    with pytest.raises(capi.AbcHipError, match="negative count"):
        call(cnt=-1)
    for kw in (dict(pb=False), dict(pg=False), dict(nb=-1), dict(ng=-1)):
        with pytest.raises(capi.AbcHipError, match="bad step list"):
            call(**kw)
    for kw in (dict(baby=(0, 2)), dict(giant=(4, 2)), dict(giant=(0, 3))):  # 3 = 4 - 1: no key for -1
        with pytest.raises(capi.AbcHipError, match="Galois key not present"):
            call(**kw)
    with pytest.raises(capi.AbcHipError, match="step count too large"):
        call(baby=(0, n // 2))
    with pytest.raises(capi.AbcHipError, match="must not overlap d_in"):
        call(out=C.c_void_p(d_x.ptr.value + 8 * (x.size - 1)))
    with pytest.raises(capi.AbcHipError, match="must not overlap d_in"):
        call(out=d_x.ptr)
    with pytest.raises(capi.AbcHipError, match="must not overlap"):
        call(out=C.c_void_p(d_d.ptr.value + 8 * (3 * L * n + nl * n - 1)))
    g.sync()
    _same("refused calls wrote nothing", g.download(d_o, x.shape), sentinel)
    _same("... nor to the input", g.download(d_x, x.shape), x)
    _same("... nor to the diagonals", g.download(d_d, (4, L, n)), r.diags[:4])
    assert g.held_buffers() == held

    call(cnt=0)
    g.sync()
    _same("count = 0 writes nothing", g.download(d_o, x.shape), sentinel)
    for kw in (dict(baby=(), giant=(0, 4)), dict(baby=(0, 1), giant=()), dict(baby=(), giant=())):
        g.op("memcpy_h2d", d_o.ptr, sentinel.ctypes.data_as(C.c_void_p), C.c_size_t(sentinel.nbytes))
        call(**kw)
        back = g.download(d_o, x.shape).ravel()
        assert not back[:owords].any() and (back[owords:] == SENTINEL).all(), "no diagonals: zeros, nl - 1 limbs per polynomial"
    g.op("memcpy_h2d", d_o.ptr, sentinel.ctypes.data_as(C.c_void_p), C.c_size_t(sentinel.nbytes))
    call()
    back = g.download(d_o, x.shape).ravel()
    _same("after the refusals", back[:owords].reshape(oshape), r.want(nl, (0, 1), (0, 4), count))
    assert (back[owords:] == SENTINEL).all()

    gb = capi.Context.bfv_default(4096)
    try:
        f_x, f_d = gb.upload(np.zeros((1, 2, gb.L, gb.n), dtype=np.uint64)), gb.upload(np.zeros((gb.L, gb.n), dtype=np.uint64))
        f_o = gb.upload(np.full((1, 2, gb.L, gb.n), SENTINEL, dtype=np.uint64))
        with pytest.raises(capi.AbcHipError, match="CKKS operation"):
            gb.op("diag_matvec_bsgs_rescale", f_x.ptr, f_d.ptr, C.c_size_t(gb.L * gb.n), _ints((0,)), 1, _ints((0,)), 1, f_o.ptr, gb.L, C.c_size_t(1))
        for op in ("diag_matvec_bsgs_rescale", "plain_sum_rescale"):
            with pytest.raises(capi.AbcHipError, match="need CKKS"):
                gb.route(op, gb.L)
        gb.sync()
        assert (gb.download(f_o, (1, 2, gb.L, gb.n)) == SENTINEL).all()
    finally:
        gb.close()
    with pytest.raises(capi.AbcHipError, match="nl >= 2"):
        g.route("diag_matvec_bsgs_rescale", 1)
    for b in (d_x, d_d, d_o):
        b.free()


# ---- recorded circuits ----
@pytest.mark.parametrize("which", ["lds_fp", "split14"])
def test_recorded_call_follows_its_inputs(rigs, keyed10, which):
    """the call in a recording (eagerly once first: the arenas get their size), replayed twice on rewritten inputs"""
    r = keyed10 if which == "lds_fp" else rigs(16384, HEAD14, POW2_STEPS, rows=2)
    baby, giant = ((0, 1, -3), (4, 0, 8)) if which == "lds_fp" else ((0, 1, 3), (0, 4, 12))
    g, n, nl, L, count = r.g, r.n, 3, r.L, 2
    x = np.ascontiguousarray(r.x(nl)[:count])
    oshape = (count, 2, nl - 1, n)
    rows = len(baby) * len(giant)
    d_x, d_d, d_o = g.upload(x), g.upload(r.diags[:rows]), g.alloc(int(np.prod(oshape)) * 8)
    held = g.held_buffers()

    def circuit():
        g.op("diag_matvec_bsgs_rescale", d_x.ptr, d_d.ptr, C.c_size_t(L * n), _ints(baby), len(baby), _ints(giant), len(giant), d_o.ptr, nl,
             C.c_size_t(count))

    circuit()
    g.sync()
    g.graph_begin()
    circuit()
    exe = g.graph_end()
    try:
        want = r.want(nl, baby, giant, count)
        for turn, order in enumerate(([0, 1], [1, 0], [1, 1])):
            x2 = np.ascontiguousarray(x[order])
            g.op("memcpy_h2d", d_x.ptr, x2.ctypes.data_as(C.c_void_p), C.c_size_t(x2.nbytes))
            fill = np.full(oshape, SENTINEL, dtype=np.uint64)
            g.op("memcpy_h2d", d_o.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes))
            if turn:
                g.graph_launch(exe)
            else:
                circuit()
            _same("turn %d" % turn, g.download(d_o, oshape), want[order])
    finally:
        g.graph_destroy(exe)
    assert g.held_buffers() == held
    for b in (d_x, d_d, d_o):
        b.free()


# ---- end to end ----
def test_a_16_by_16_matrix_times_a_vector(capi):
    """ckks_encode, encrypt, bsgs_diagonals + diag_matvec_bsgs_rescale 4 x 4, decrypt, ckks_decode at scale^2 / q_2 against numpy.  The
    vector is tiled over the 512 slots with period 16, so a rotation of the slots is a cyclic rotation of the vector; entries in
    [-1, 1] at scale 2^40, the bound the project's 1e-4 (tests/test_plain_sum_rescale_spec.py measures 7.5e-8 for this sum on the oracle)"""
    n, scale, dim = 1024, 2.0 ** 40, 16
    g = capi.Context(capi.CKKS, n, capi.create_primes(n, FP_CHAIN))
    try:
        g.keygen(0xB565)  # the default key set: 3, 12 and others are NAF chains
        rng = np.random.default_rng(1616)
        m, v = rng.uniform(-1, 1, (dim, dim)), rng.uniform(-1, 1, dim)
        slots = np.arange(n // 2)
        diags = np.stack([m[slots % dim, (slots + d) % dim] for d in range(dim)])  # diagonal d, tiled
        ct = g.encrypt(g.ckks_encode(np.tile(v, n // 2 // dim), scale), seed=5)
        rows = g.bsgs_diagonals(g.ckks_encode(diags, scale), BABY, GIANT)
        assert g.route("diag_matvec_bsgs_rescale", g.L) == LDS
        out = g.diag_matvec_bsgs_rescale(ct, rows, BABY, GIANT)
        assert out.shape == (2, g.L - 1, n)
        out_scale = scale * scale / g.primes[g.L - 1]
        dec = g.ckks_decode(g.decrypt(out), out_scale)
        err = np.abs(dec.real - np.tile(m @ v, n // 2 // dim)).max()
        print("16 x 16 matvec, BSGS 4 x 4 with the rescale before the giant steps: max |error| = %.3g" % err)
        assert err < 1e-4 and np.abs(dec.imag).max() < 1e-4
        after = g.rescale(g.diag_matvec_bsgs(ct, rows, BABY, GIANT))
        assert np.abs(g.ckks_decode(g.decrypt(after), out_scale).real - dec.real).max() < 1e-4
        assert (after != out).mean() > 0.99  # another ciphertext, the same values
    finally:
        g.close()
