"""abc_hip_bfv_diag_matvec_bsgs on the device, word for word against tests/bfv_plain_sum_spec.py: the CPU oracle's rotate for the
baby steps, its multiply_plain and add for the inner sums (plaintexts modulo t; the device gets them through
abc_hip_bfv_plain_to_ntt), its rotate and add for the giant steps, in the order the header gives.  The ciphertexts are random
residues and the plaintext rows random values modulo t with t - 1 and the lift threshold among them: every step is exact modular
arithmetic or the oracle's own key switch.  The rolled encoding of the rows is checked end to end in the last test."""
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
STEPS = tuple(range(1, 16)) + (-1, -2, -3, -5, 20, 100)  # a key of its own for every step of the grids below
POW2_STEPS = (1, 2, 4, 8, 16, -1, -4)  # 3 = 4 - 1 and 12 = 16 - 4 are NAF chains
ROUTES = {4096: "permute lds_fp plainsum=fused add=separate", 8192: "fold bsplit_big plainsum=fused add=fused"}


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


def _ints(v):
    return (C.c_int * max(len(v), 1))(*[int(x) for x in v])


class Rig:
    """BFVDefault(n): the oracle and a device context with the oracle's keys for `steps`; random ciphertext words, 20 plaintext rows
    modulo t with their NTT form from the device, and the references computed so far (shared, never changed)"""

    def __init__(self, om, capi, n, steps, rows=11):
        self.o = o = om.Oracle.bfv_default(n)
        o.keygen(0xB5F5 + n, elts=sorted({o.elt_from_step(s) for s in steps}))
        self.g = capi.Context.bfv_default(n)
        self.g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={e: o.galois_key(e) for e in o.galois_elts()})
        self.n, self.L = n, o.L
        rng = np.random.default_rng(n)
        self.x = np.stack([rng.integers(0, q, size=(rows, 2, n), dtype=np.uint64) for q in o.primes[:o.L]], axis=2)  # [rows][2][L][N]
        t, thr = o.t, (o.t + 1) // 2
        self.plains = rng.integers(0, t, size=(20, n), dtype=np.uint64)
        self.plains[0] = t - 1
        self.plains[1] = np.array([0, t - 1, thr - 1, thr], dtype=np.uint64)[np.arange(n) % 4]
        self.diags = self.g.bfv_plain_to_ntt(self.plains)  # [20][L][N]
        for a in (self.x, self.plains, self.diags):
            a.setflags(write=False)
        self._want = {}

    def want(self, baby, giant, count):
        k = (tuple(baby), tuple(giant))
        have = self._want.get(k, np.zeros((0, 2, self.L, self.n), dtype=np.uint64))
        if len(have) < count:
            more = [spec.diag_matvec_bsgs(self.o, self.x[r], list(self.plains), baby, giant) for r in range(len(have), count)]
            have = np.concatenate([have, np.stack(more)])
            have.setflags(write=False)
            self._want[k] = have
        return have[:count]

    def check(self, tag, baby, giant, count=2):
        got = self.g.bfv_diag_matvec_bsgs(self.x[:count], self.diags[: len(baby) * len(giant)], baby, giant)
        _same("%s N=%d baby %s giant %s" % (tag, self.n, list(baby), list(giant)), got, self.want(baby, giant, count))

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def rigs(oracle_mod, capi):
    made = {}

    def get(n, steps=STEPS):
        if (n, steps) not in made:
            made[(n, steps)] = Rig(oracle_mod, capi, n, steps)
        return made[(n, steps)]

    yield get
    for r in made.values():
        r.close()


def test_plain_rows_in_ntt_form_are_the_specs(rigs):
    r = rigs(4096)
    for row in (0, 1, 7):
        _same("row %d" % row, r.diags[row], spec.plain_to_ntt(r.o, r.plains[row]))


@pytest.mark.parametrize("baby,giant", [
    ((0, 1, 2, 3), (0, 4, 8, 12)),      # 4 x 4
    ((0, 1, 2, 3, 4, 5, 6), (0,)),      # n x 1: one inner sum, no giant rotation
    ((0,), (0, 1, 2, 3, 4, 5, 6)),      # 1 x n: no baby rotation, the transformed copy alone
    ((5,), (7,)),                       # 1 x 1 without step 0
    ((0, 1, 2), (0, 3, 6, 9, 12)),      # 3 x 5
    ((1, 2, 3), (4, 8)),                # no step 0 on either side
    ((-1, 0, 1, -3), (-5, 5, 0)),       # negative steps, step 0 in the middle and last
    ((1, 1, 0, 0, 2), (4, 4, 0, 0)),    # duplicates, step 0 twice: two transformed copies; a repeated giant step of 0
    ((0, 1, 2, 3, 4, 5, 6, 7, 8), (100, 20)),  # nine baby steps: two launches of the inner sum, the partial sum in its arena
], ids=["4x4", "7x1", "1x7", "1x1", "3x5", "no-zero", "negative", "duplicates", "9x2"])
@pytest.mark.parametrize("n", [4096, 8192])
def test_grids_and_step_lists(rigs, n, baby, giant):
    r = rigs(n)
    assert r.g.route("bfv_matvec_bsgs", r.L, 2) == ROUTES[n]
    r.check("grid", baby, giant, 2)


@pytest.mark.parametrize("n", [4096, 8192])
def test_a_naf_step_and_the_general_sum(rigs, n):
    """the power-of-two key set: 3 = 4 - 1 is a chain of two hops on the baby and on the giant side; then the same under ABC_HIP_NO_FUSED"""
    r = rigs(n, POW2_STEPS)
    assert r.o.elt_from_step(3) not in r.g.galois_elts()
    r.check("NAF", (0, 3, 1), (3, 0, 12))
    with _env(r.g, {"ABC_HIP_NO_FUSED": "1"}):
        assert " plainsum=ntt_domain " in r.g.route("bfv_matvec_bsgs", r.L, 2)
        r.check("NAF, ntt_domain", (0, 3, 1), (3, 0, 12))


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_groups_and_ragged_last_group(rigs, lanes):
    """ABC_HIP_CHUNK=2: groups of chunk * lanes ciphertexts -- two up to a batch of eight, four at eleven on two lanes -- the last one
    ragged: its slabs are transformed one by one"""
    r = rigs(4096)
    with _env(r.g, {"ABC_HIP_CHUNK": "2", "ABC_HIP_LANES": lanes}):
        for count in (5, 11):
            r.check("count %d" % count, (0, 1, 2), (0, 3, 6), count)


@pytest.mark.parametrize("n", [4096, 8192])
def test_the_devices_own_sequence_gives_the_same_words(rigs, n):
    """abc_hip_rotate per baby step, abc_hip_ntt_limbs on the rotated ciphertexts, abc_hip_bfv_multiply_plain_sum on NTT-form terms
    per giant step, abc_hip_rotate_add onto the running sum"""
    r = rigs(n)
    g, L, count = r.g, r.L, 3
    baby, giant = (0, 1, 2, -3), (4, 0, 8)
    x = np.ascontiguousarray(r.x[:count])
    rows = len(baby) * len(giant)
    d_x, d_d = g.upload(x), g.upload(r.diags[:rows])
    d_rot = [g.alloc(x.nbytes) for _ in baby]
    d_inner, d_acc, d_out = g.alloc(x.nbytes), g.alloc(x.nbytes), g.alloc(x.nbytes)
    try:
        for b, d in zip(baby, d_rot):
            if b:
                g.op("rotate", d_x.ptr, d.ptr, L, b, C.c_size_t(count))
            else:
                g.op("memcpy_d2d", d.ptr, d_x.ptr, C.c_size_t(x.nbytes))
            g.op("ntt_limbs", d.ptr, L, C.c_size_t(count * 2), 0)
        for j, s in enumerate(giant):
            plains = [C.c_void_p(d_d.ptr.value + 8 * (j * len(baby) + i) * L * n) for i in range(len(baby))]
            g.op("bfv_multiply_plain_sum", g.term_pointers([d.ptr for d in d_rot]), spec.NTT, g.term_pointers(plains), C.c_size_t(0), len(baby),
                 None, d_inner.ptr, 2, C.c_size_t(count))
            if j == 0:
                g.op("rotate", d_inner.ptr, d_acc.ptr, L, s, C.c_size_t(count))
            elif s == 0:
                g.op("add", d_acc.ptr, d_inner.ptr, d_acc.ptr, 2, L, C.c_size_t(count))
            else:
                g.op("rotate_add", d_inner.ptr, d_acc.ptr, d_acc.ptr, L, s, C.c_size_t(count))
        g.op("bfv_diag_matvec_bsgs", d_x.ptr, d_d.ptr, C.c_size_t(L * n), _ints(baby), len(baby), _ints(giant), len(giant), d_out.ptr,
             C.c_size_t(count))
        _same("one call against the sequence of calls", g.download(d_out, x.shape), g.download(d_acc, x.shape))
        _same("... and the spec", g.download(d_out, x.shape), r.want(baby, giant, count))
        _same("the input is left alone", g.download(d_x, x.shape), x)
    finally:
        for b in [d_x, d_d, d_inner, d_acc, d_out] + d_rot:
            b.free()


# ---- refused and empty calls: nothing is written ----
def test_refused_and_empty_calls(oracle_mod, capi):
    r = Rig(oracle_mod, capi, 4096, (1, 4))  # step 2 has neither a key nor a chain of keys
    g, n, L, count = r.g, r.n, r.L, 2
    try:
        x = np.ascontiguousarray(r.x[:count])
        sentinel = np.full(x.shape, SENTINEL, dtype=np.uint64)
        d_x, d_d, d_o = g.upload(x), g.upload(r.diags[:4]), g.upload(sentinel)
        held = g.held_buffers()

        def call(baby=(0, 1), giant=(0, 4), src=None, diags=None, stride=L * n, out=None, cnt=count, nb=None, ng=None, pb=True, pg=True):
            g.op("bfv_diag_matvec_bsgs", d_x.ptr if src is None else src, d_d.ptr if diags is None else diags, C.c_size_t(stride), _ints(baby) if pb else None,
                 len(baby) if nb is None else nb, _ints(giant) if pg else None, len(giant) if ng is None else ng, d_o.ptr if out is None else out, C.c_size_t(cnt))

        with pytest.raises(capi.AbcHipError, match="diag_stride must be at least"):
            call(stride=L * n - 1)
        with pytest.raises(capi.AbcHipError, match="negative count"):
            call(cnt=-1)
        null = C.c_void_p(0)
        for kw in (dict(src=null), dict(out=null), dict(diags=null)):
            with pytest.raises(capi.AbcHipError, match="null pointer"):
                call(**kw)
        for kw in (dict(pb=False), dict(pg=False), dict(nb=-1), dict(ng=-1)):
            with pytest.raises(capi.AbcHipError, match="bad step list"):
                call(**kw)
        for kw in (dict(baby=(0, 2)), dict(giant=(4, 2)), dict(giant=(0, 3))):  # 3 = 4 - 1: no key for -1
            with pytest.raises(capi.AbcHipError, match="Galois key not present"):
                call(**kw)
        with pytest.raises(capi.AbcHipError, match="step count too large"):
            call(baby=(0, n // 2))
        words = x.size
        with pytest.raises(capi.AbcHipError, match="must not overlap d_in"):
            call(out=C.c_void_p(d_x.ptr.value + 8 * (words - 1)))
        with pytest.raises(capi.AbcHipError, match="must not overlap d_in"):
            call(out=d_x.ptr)
        with pytest.raises(capi.AbcHipError, match="must not overlap"):
            call(out=C.c_void_p(d_d.ptr.value + 8 * (4 * L * n - 1)))
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
            assert not g.download(d_o, x.shape).any(), "no diagonals: zeros"
        call()
        _same("after the refusals", g.download(d_o, x.shape), r.want((0, 1), (0, 4), count))
        for b in (d_x, d_d, d_o):
            b.free()
    finally:
        r.close()

    n = 1024
    gc = capi.Context(capi.CKKS, n, capi.create_primes(n, [50, 40, 50]))
    try:
        f_x, f_d = gc.upload(np.zeros((1, 2, 2, n), dtype=np.uint64)), gc.upload(np.zeros((2, n), dtype=np.uint64))
        f_o = gc.upload(np.full((1, 2, 2, n), SENTINEL, dtype=np.uint64))
        with pytest.raises(capi.AbcHipError, match="BFV only"):
            gc.op("bfv_diag_matvec_bsgs", f_x.ptr, f_d.ptr, C.c_size_t(2 * n), _ints((0,)), 1, _ints((0,)), 1, f_o.ptr, C.c_size_t(1))
        with pytest.raises(capi.AbcHipError, match="need BFV"):
            gc.route("bfv_matvec_bsgs", 2)
        gc.sync()
        assert (gc.download(f_o, (1, 2, 2, n)) == SENTINEL).all()
    finally:
        gc.close()


# ---- recorded circuits ----
@pytest.mark.parametrize("n", [4096, 8192])
def test_recorded_call_follows_its_inputs(rigs, n):
    """the call in a recording (eagerly once first: the arenas get their size), replayed twice on rewritten inputs"""
    r = rigs(n)
    baby, giant = (0, 1, -3), (4, 0, 8)
    g, L, count = r.g, r.L, 2
    x = np.ascontiguousarray(r.x[:count])
    rows = len(baby) * len(giant)
    d_x, d_d, d_o = g.upload(x), g.upload(r.diags[:rows]), g.alloc(x.nbytes)

    def circuit():
        g.op("bfv_diag_matvec_bsgs", d_x.ptr, d_d.ptr, C.c_size_t(L * n), _ints(baby), len(baby), _ints(giant), len(giant), d_o.ptr,
             C.c_size_t(count))

    circuit()
    g.sync()
    held = g.held_buffers()
    g.graph_begin()
    circuit()
    exe = g.graph_end()
    try:
        want = r.want(baby, giant, count)
        for turn, order in enumerate(([0, 1], [1, 0], [1, 1])):
            x2 = np.ascontiguousarray(x[order])
            g.op("memcpy_h2d", d_x.ptr, x2.ctypes.data_as(C.c_void_p), C.c_size_t(x2.nbytes))
            g.op("memcpy_h2d", d_o.ptr, np.full(x.shape, SENTINEL, dtype=np.uint64).ctypes.data_as(C.c_void_p), C.c_size_t(x.nbytes))
            if turn:
                g.graph_launch(exe)
            else:
                circuit()
            _same("turn %d" % turn, g.download(d_o, x.shape), want[order])
    finally:
        g.graph_destroy(exe)
    assert g.held_buffers() == held
    for b in (d_x, d_d, d_o):
        b.free()


# ---- end to end ----
def test_a_16_by_16_matrix_times_a_vector(capi):
    """batch_encode, encrypt, bfv_bsgs_diagonals + bfv_diag_matvec_bsgs 4 x 4, decrypt, batch_decode: exactly numpy's matrix-vector
    product modulo t.  The vector is tiled over both rows of slots with period 16, so a rotation of the rows is a cyclic rotation of
    the vector; BFVDefault(8192), where tests/test_bfv_plain_sum_spec.py finds noise budget left on the oracle"""
    n, dim, baby, giant = 8192, 16, (0, 1, 2, 3), (0, 4, 8, 12)
    g = capi.Context.bfv_default(n)
    try:
        g.keygen(0xB5F5)  # the default key set: 3 and 12 are NAF chains
        rng = np.random.default_rng(1616)
        m, v = rng.integers(0, 64, (dim, dim)), rng.integers(0, 64, dim)
        tile = n // dim
        diag_values = np.stack([np.tile(m[np.arange(dim), (np.arange(dim) + gs + bs) % dim], tile) for gs in giant for bs in baby])
        ct = g.encrypt(g.batch_encode(np.tile(v, tile)), seed=5)
        rows = g.bfv_bsgs_diagonals(diag_values, baby, giant)
        out = g.bfv_diag_matvec_bsgs(ct, rows, baby, giant)
        got = g.batch_decode(g.decrypt(out)) % g.t
        assert np.array_equal(got, np.tile((m @ v) % g.t, tile))
        budget = g.noise_budget(out)
        print("16 x 16 matvec mod t, BSGS 4 x 4 on BFVDefault(%d): noise budget %d bits" % (n, budget))
        assert budget > 0
    finally:
        g.close()
