"""CKKS multiply_plain + rescale as one call (abc_hip_multiply_plain_rescale): the plaintext product formed in the loads of the two
LDS-resident rescale kernels where route("multiply_plain_rescale") says "mulplain=fused", and multiply_plain into an arena followed by
the rescale everywhere else.  Both steps are exact modular arithmetic, so every comparison is word for word against
o.rescale(o.multiply_plain(x, p)), per ciphertext.  Batches of three distinct ciphertexts of size 2 and 3; plaintexts one for the
batch, one per ciphertext nl * N apart, and rows of L limbs L * N apart at nl < L, all different, so a wrong row index shows.  Every
case asserts its route string, so a silent fall-back fails."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
FORMS = ("bcast", "per", "wide")
FP_CHAIN, MIXED_CHAIN = [50, 40, 40, 50], [60, 40, 40, 60]


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


class Rig:
    """one CKKS oracle and one device context on the same primes; three ciphertexts of size 3 (size 2: their first two polynomials)
    and three plaintexts of L limbs, random residues; a level nl is their first nl limbs (limb j is modulo q_j at every level).
    References are computed once per (level, size, form) and never changed."""

    def __init__(self, om, capi, n, bits):
        primes = om.create_primes(n, bits)
        self.o = om.Oracle(om.CKKS, n, primes)
        self.g = capi.Context(capi.CKKS, n, self.o.primes)
        self.n, self.primes, self.L = n, list(primes), self.o.L
        rng = np.random.default_rng(n + sum(bits))
        self.x = np.stack([rng.integers(0, q, size=(3, 3, n), dtype=np.uint64) for q in primes[:self.L]], axis=2)  # [3][3][L][N]
        self.plain = np.stack([rng.integers(0, q, size=(3, n), dtype=np.uint64) for q in primes[:self.L]], axis=1)  # [3][L][N]
        self.x.setflags(write=False)
        self.plain.setflags(write=False)
        self._want = {}

    def inputs(self, level, size):
        return np.ascontiguousarray(self.x[:, :size, :level])

    def plain_for(self, level, form):
        """(host array, stride in words); the broadcast plaintext is row 1"""
        if form == "bcast":
            return np.ascontiguousarray(self.plain[1, :level]), 0
        if form == "per":
            return np.ascontiguousarray(self.plain[:, :level]), level * self.n
        return np.ascontiguousarray(self.plain), self.L * self.n  # rows encoded for the top level

    def reference(self, x, p_rows):
        """[count][size][nl-1][N]: the oracle's product, then its rescale, per ciphertext"""
        return np.stack([self.o.rescale(self.o.multiply_plain(x[r], np.ascontiguousarray(p_rows[r]))) for r in range(len(x))])

    def want(self, level, size, form):
        k = (level, size, form == "bcast")
        if k not in self._want:
            rows = [self.plain[1 if form == "bcast" else r, :level] for r in range(3)]
            self._want[k] = self.reference(self.inputs(level, size), rows)
            self._want[k].setflags(write=False)
        return self._want[k]

    def run(self, x, p, stride):
        """one raw call into a buffer filled with a pattern; the inputs are left alone"""
        g = self.g
        count, size, level = x.shape[:3]
        shp = (count, size, level - 1, self.n)
        d_x, d_p, d_o = g.upload(x), g.upload(p), g.upload(np.full(shp, SENTINEL, dtype=np.uint64))
        try:
            g.op("multiply_plain_rescale", d_x.ptr, d_p.ptr, C.c_size_t(stride), d_o.ptr, size, level, C.c_size_t(count))
            got = g.download(d_o, shp)
            _same("the ciphertexts are left alone", g.download(d_x, x.shape), x)
            _same("the plaintexts are left alone", g.download(d_p, p.shape), p)
            return got
        finally:
            for b in (d_x, d_p, d_o):
                b.free()

    def check(self, tag, level, sizes=(2, 3), forms=FORMS):
        for size in sizes:
            for form in forms:
                if form == "wide" and level == self.L:
                    continue
                p, stride = self.plain_for(level, form)
                got = self.run(self.inputs(level, size), p, stride)
                want = self.want(level, size, form)
                for row in range(3):
                    _same("%s nl=%d size %d plain %s row %d" % (tag, level, size, form, row), got[row], want[row])

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def rigs(oracle_mod, capi):
    """rigs by (N, chain), built on first use and shared by the module"""
    made = {}

    def get(n, bits):
        k = (n, tuple(bits))
        if k not in made:
            made[k] = Rig(oracle_mod, capi, n, bits)
        return made[k]

    yield get
    for r in made.values():
        r.close()


# ---- routes and arithmetic ----
@pytest.mark.parametrize("level", [3, 2])
def test_fp_chain(rigs, level):
    r = rigs(4096, FP_CHAIN)
    assert r.g.route("multiply_plain_rescale", level, 3) == "fp mulplain=fused"
    r.check("fp", level)


@pytest.mark.parametrize("level,route", [(3, "mixed fpmask=0x6 mulplain=fused"), (2, "mixed fpmask=0x2 mulplain=fused")])
def test_mixed_chain(rigs, level, route):
    r = rigs(4096, MIXED_CHAIN)
    assert r.g.route("multiply_plain_rescale", level, 3) == route
    r.check("mixed", level)


@pytest.mark.parametrize("level", [3, 2])
def test_mixed_chain_all_integer_step_b(rigs, level):
    r = rigs(4096, MIXED_CHAIN)
    with _env(r.g, {"ABC_HIP_NO_MIXED": "1"}):
        assert r.g.route("multiply_plain_rescale", level, 3) == "mixed fpmask=0x0 mulplain=fused"
        r.check("no_mixed", level)


def test_smallest_ring_and_level(rigs):
    r = rigs(1024, [50, 40, 50])
    assert r.g.route("multiply_plain_rescale", 2, 3) == "fp mulplain=fused"
    r.check("n=1024", 2)


@pytest.mark.parametrize("level", [4, 2])
def test_workload_ring(rigs, level):
    """LB = 14, the benchmark chain's own instantiation"""
    r = rigs(16384, [50, 40, 40, 40, 50])
    assert r.g.route("multiply_plain_rescale", level, 3) == "fp mulplain=fused"
    r.check("n=16384", level, forms=("bcast", "wide") if level < 4 else ("bcast", "per"))


@pytest.mark.parametrize("env,route", [
    ({"ABC_HIP_NO_FUSED": "1"}, "generic mulplain=separate"),
    ({"ABC_HIP_NO_MULPLAIN_RESCALE_FUSION": "1"}, "fp mulplain=separate"),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else "")
def test_separate_by_switch(rigs, env, route):
    r = rigs(4096, FP_CHAIN)
    with _env(r.g, env):
        assert r.g.route("multiply_plain_rescale", 3, 3) == route
        r.check(" ".join(env), 3)
    assert r.g.route("multiply_plain_rescale", 3, 3) == "fp mulplain=fused"


def test_separate_on_the_large_ring(rigs):
    r = rigs(32768, FP_CHAIN)
    assert r.g.route("multiply_plain_rescale", 3, 3) == "generic mulplain=separate"
    r.check("n=32768", 3, sizes=(2,), forms=("per",))
    r.check("n=32768", 3, sizes=(3,), forms=("bcast",))


# ---- extremes ----
def _extreme_rows(r, level, size):
    """(x [4][size][level][N], plain [4][level][N]): q-1 times q-1, 0 times 0 and q-1 times 1 at every coefficient of every limb, and
    a row of random words with those pairs at the ends of the ring and at the first and last position of a workgroup's threads (16
    coefficients each) and wavefronts"""
    n = r.n
    q = np.array(r.primes[:level], dtype=np.uint64)
    x = np.empty((4, size, level, n), dtype=np.uint64)
    p = np.empty((4, level, n), dtype=np.uint64)
    x[0], p[0] = (q - 1)[None, :, None], (q - 1)[:, None]
    x[1], p[1] = 0, 0
    x[2], p[2] = (q - 1)[None, :, None], 1
    x[3], p[3] = r.x[0, :size, :level], r.plain[0, :level]
    spots = np.array([0, 1, 15, 16, 63 * 16, 64 * 16 - 1, n // 2 - 1, n // 2, n - 64 * 16, n - 17, n - 16, n - 2, n - 1])
    spots = spots[(spots >= 0) & (spots < n)]
    for i, s in enumerate(spots):
        kind = i % 3
        x[3][:, :, s] = 0 if kind == 1 else (q - 1)[None, :]
        p[3][:, s] = (q - 1) if kind == 0 else 0 if kind == 1 else 1
    return x, p


@pytest.mark.parametrize("bits,level", [(FP_CHAIN, 3), (FP_CHAIN, 2), (MIXED_CHAIN, 3), (MIXED_CHAIN, 2)],
                         ids=["fp-3", "fp-2", "mixed-3", "mixed-2"])
def test_extremes(rigs, bits, level):
    """limb 0 is the 50-bit prime of the fp chain and the 60-bit prime of the mixed one: (q-1)^2 is the largest product there is"""
    r = rigs(4096, bits)
    assert r.g.route("multiply_plain_rescale", level, 4).endswith("mulplain=fused")
    for size in (2, 3):
        x, p = _extreme_rows(r, level, size)
        want = r.reference(x, p)
        _same("extremes, one plaintext each, size %d" % size, r.run(x, p, level * r.n), want)
        _same("all q-1, one plaintext for the batch", r.run(x[:1], p[0], 0), want[:1])


# ---- against the device's own two calls, and the numpy front end ----
@pytest.mark.parametrize("bits", [FP_CHAIN, MIXED_CHAIN], ids=["fp", "mixed"])
def test_against_the_two_calls(rigs, bits):
    r = rigs(4096, bits)
    g = r.g
    for size in (2, 3):
        x = r.inputs(3, size)
        p, _ = r.plain_for(3, "per")
        two = g.rescale(g.multiply_plain(x, p))
        _same("one call against two, size %d" % size, g.multiply_plain_rescale(x, p), two)
        _same("and the oracle", two, r.want(3, size, "per"))
    x = r.inputs(2, 2)
    _same("rows of L limbs", g.multiply_plain_rescale(x, r.plain), r.want(2, 2, "per"))
    _same("broadcast", g.multiply_plain_rescale(x, r.plain[1, :2]), r.want(2, 2, "bcast"))
    _same("one ciphertext", g.multiply_plain_rescale(x[2], r.plain[1, :2]), r.want(2, 2, "bcast")[2])


# ---- refused and empty calls: nothing is written ----
def test_refused_and_empty_calls(rigs, capi):
    r = rigs(4096, FP_CHAIN)
    g, n = r.g, r.n
    x = r.inputs(3, 3)
    p, stride = r.plain_for(3, "per")
    sentinel = np.full(x.shape, SENTINEL, dtype=np.uint64)  # room for any refused shape
    d_x, d_p, d_o = g.upload(x), g.upload(p), g.upload(sentinel)
    held = g.held_buffers()

    def call(nl=3, size=3, count=3, st=stride, ct=None, pl=None, out=None):
        g.op("multiply_plain_rescale", ct or d_x.ptr, pl or d_p.ptr, C.c_size_t(st), out or d_o.ptr, size, nl, C.c_size_t(count))

    with pytest.raises(capi.AbcHipError, match="no limb left to drop"):
        call(nl=1)
    for nl in (0, 4, -1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            call(nl=nl)
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            g.route("multiply_plain_rescale", nl, 3)
    with pytest.raises(capi.AbcHipError, match="needs CKKS and nl >= 2"):
        g.route("multiply_plain_rescale", 1, 3)
    for bad in (1, n, 3 * n - 1):
        with pytest.raises(capi.AbcHipError, match="plain_stride must be 0 or at least nl"):
            call(st=bad)
    for size in (0, 1, 4, -2):
        with pytest.raises(capi.AbcHipError, match="size must be 2 or 3"):
            call(size=size)
    out_words = 3 * 3 * 2 * n
    for off in (0, out_words - 1):  # the plaintext inside d_out: its first word on d_out's first and on its last
        with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):
            call(st=0, pl=C.c_void_p(d_o.ptr.value + 8 * off))
    with pytest.raises(capi.AbcHipError, match="must not overlap d_out"):  # d_out on the last word the plaintexts have
        call(out=C.c_void_p(d_p.ptr.value + 8 * (p.size - 1)))
    for off in (0, out_words - 1):  # d_ct inside d_out, d_out == d_ct among them
        with pytest.raises(capi.AbcHipError, match="d_out must not overlap d_ct"):
            call(ct=C.c_void_p(d_o.ptr.value + 8 * off))
    with pytest.raises(capi.AbcHipError, match="d_out must not overlap d_ct"):  # d_out on the last word of d_ct
        call(out=C.c_void_p(d_x.ptr.value + 8 * (x.size - 1)))
    call(count=0)  # nothing to do: success, nothing enqueued
    g.sync()
    _same("refused and empty calls wrote nothing", g.download(d_o, x.shape), sentinel)
    _same("... nor to the ciphertexts", g.download(d_x, x.shape), x)
    _same("... nor to the plaintexts", g.download(d_p, p.shape), p)
    assert g.held_buffers() == held
    for b in (d_x, d_p, d_o):
        b.free()


def test_bfv_context_is_refused(capi):
    g = capi.Context.bfv_default(4096)
    try:
        L, n = g.L, g.n
        sentinel = np.full((3, 2, L, n), SENTINEL, dtype=np.uint64)
        d_x, d_p, d_o = g.upload(np.zeros((3, 2, L, n), dtype=np.uint64)), g.upload(np.zeros((L, n), dtype=np.uint64)), g.upload(sentinel)
        with pytest.raises(capi.AbcHipError, match="multiply_plain_rescale is a CKKS operation"):
            g.op("multiply_plain_rescale", d_x.ptr, d_p.ptr, C.c_size_t(0), d_o.ptr, 2, L, C.c_size_t(3))
        with pytest.raises(capi.AbcHipError, match="needs CKKS and nl >= 2"):
            g.route("multiply_plain_rescale", L, 3)
        g.sync()
        _same("a refused call wrote nothing", g.download(d_o, sentinel.shape), sentinel)
        for b in (d_x, d_p, d_o):
            b.free()
    finally:
        g.close()


# ---- recorded ----
@pytest.mark.parametrize("env,route", [
    ({}, "fp mulplain=fused"),
    ({"ABC_HIP_NO_MULPLAIN_RESCALE_FUSION": "1"}, "fp mulplain=separate"),  # the product's arena is part of the recording
], ids=["fused", "separate"])
def test_recorded_call_follows_its_input(rigs, env, route):
    """record one call (eagerly once first: the scratch gets its size), then replay twice with the input rewritten in between"""
    r = rigs(4096, FP_CHAIN)
    g = r.g
    x = r.inputs(3, 2)
    p, stride = r.plain_for(3, "per")
    want = r.want(3, 2, "per")
    shp = want.shape
    with _env(g, env):
        assert g.route("multiply_plain_rescale", 3, 3) == route
        d_x, d_p, d_o = g.upload(x), g.upload(p), g.alloc(want.nbytes)
        held = g.held_buffers()

        def circuit():
            g.op("multiply_plain_rescale", d_x.ptr, d_p.ptr, C.c_size_t(stride), d_o.ptr, 2, 3, C.c_size_t(3))

        circuit()
        g.sync()
        g.graph_begin()
        circuit()
        exe = g.graph_end()
        try:
            _same("eager", g.download(d_o, shp), want)
            for turn, order in enumerate(([2, 0, 1], [1, 2, 0])):
                # the same ciphertexts in another order, each with the plaintext of its new place: new input, same buffers
                x2 = np.ascontiguousarray(x[order])
                want2 = r.reference(x2, [r.plain[i, :3] for i in range(3)])
                g.op("memcpy_h2d", d_x.ptr, x2.ctypes.data_as(C.c_void_p), C.c_size_t(x2.nbytes))
                g.op("memcpy_h2d", d_o.ptr, np.full(shp, SENTINEL, dtype=np.uint64).ctypes.data_as(C.c_void_p), C.c_size_t(want.nbytes))
                g.graph_launch(exe)
                _same("replay %d" % turn, g.download(d_o, shp), want2)
        finally:
            g.graph_destroy(exe)
        assert g.held_buffers() == held
        for b in (d_x, d_p, d_o):
            b.free()


# ---- end to end ----
def test_weights_end_to_end(rigs):
    """encode, encrypt, multiply by an encoded weight vector and rescale in one call, decrypt, decode.  The bound is the one
    tests/test_gpu_ckks_codec.py::test_pipeline_without_host_codec allows a product of entries in [-1, 1] after one rescale."""
    r = rigs(4096, FP_CHAIN)
    g, n, L = r.g, r.n, r.L
    scale = 2.0 ** 40
    rng = np.random.default_rng(17)
    g.keygen(0xE2E)
    v, w = rng.uniform(-1, 1, n // 2), rng.uniform(-1, 1, n // 2)
    ct = g.encrypt(g.ckks_encode(v, scale), seed=5)
    weights = g.ckks_encode(w, scale)
    assert g.route("multiply_plain_rescale", L, 1) == "fp mulplain=fused"
    out = g.multiply_plain_rescale(ct, weights)
    assert out.shape == (2, L - 1, n)
    _same("the two calls", out, g.rescale(g.multiply_plain(ct, weights)))
    dec = g.ckks_decode(g.decrypt(out), scale * scale / r.primes[L - 1])
    print("weights end to end: max |error| = %.3g" % np.abs(dec.real - v * w).max())
    assert np.abs(dec.real - v * w).max() < 1e-4
    assert np.abs(dec.imag).max() < 1e-4
