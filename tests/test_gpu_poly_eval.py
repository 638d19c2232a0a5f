"""abc_hip_ckks_poly_eval on the device, word for word against tests/poly_eval_spec.py (the fixed sequence of include/abc_hip.h on
the CPU oracle): every route its products can take, the levels each power is read at, groups, refusals, recordings, and one
activation from encode to decode.

The constant term enters the last sum at out_scale * q_{m-1} and const_words holds that below 2^62: the seven-limb chain has
30-bit rescaling primes and works at scale 2^30 throughout; on the 40-bit chains of the other routes the result is asked for at
2^20 (the words, not the precision, are what those cases compare)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly_eval_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
SEVEN = [50, 30, 30, 30, 30, 30, 30, 50]
BOUND = 1e-4  # tests/test_poly_eval_spec.py: the project's bound; the spec itself measures 2.2e-06 at degree 7 there


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s" % (what, len(bad), got.size, tuple(bad[0])))


@contextlib.contextmanager
def _env(g, settings):
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
    """one oracle and one device context with the same keys; x: random residues at the top level, [count][2][L][N]"""

    def __init__(self, om, capi, n, bits, seed, count):
        self.o = om.Oracle(om.CKKS, n, om.create_primes(n, bits))
        self.o.keygen(seed)
        self.g = capi.Context(capi.CKKS, n, self.o.primes)
        self.g.keygen(seed)  # the same sampling spec: identical keys
        self.n, self.L = n, self.o.L
        rng = np.random.default_rng(seed)
        self.x = np.stack([rng.integers(0, q, size=(count, 2, n), dtype=np.uint64) for q in self.o.primes[: self.L]], axis=2)
        self.x.setflags(write=False)
        self._want = {}

    def want(self, x_scale, coeffs, out_scale, count=None):
        key = (x_scale, tuple(coeffs), out_scale)
        have = self._want.setdefault(key, [])
        for i in range(len(have), count or len(self.x)):
            have.append(spec.poly_eval(self.o, self.x[i], x_scale, list(coeffs), out_scale))
        return np.stack(have[: count or len(self.x)])

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def seven(oracle_mod, capi):
    r = Rig(oracle_mod, capi, 1024, SEVEN, 0x5E7E, 5)
    yield r
    r.close()


COEFFS = [0.3, -0.8, 0.45, 0.7, -0.2, 0.15, -0.6, 0.9, -0.35]


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 7, 8])
def test_seven_limbs_every_degree(seven, degree):
    r, s = seven, 2.0 ** 30
    g = r.g
    route = g.route("poly_eval", r.L, 3)
    assert route == "lds_fp constsum=separate" and route == g.route("mul_relin", r.L, 3) + " constsum=separate"
    coeffs = COEFFS[: degree + 1]
    got = g.poly_eval(r.x[:3], s, coeffs, s)
    assert got.shape == (3, 2, r.L - g.poly_eval_depth(degree), r.n)
    _same("degree %d" % degree, got, r.want(s, coeffs, s, 3))
    with _env(g, {"ABC_HIP_NO_CONST_MAC_SUM": "1"}):
        _same("degree %d, the last step composed" % degree, g.poly_eval(r.x[:1], s, coeffs, s), r.want(s, coeffs, s, 1))


def test_zero_coefficients_skip_terms_and_powers(seven):
    r, s, g = seven, 2.0 ** 30, seven.g
    for coeffs in ([0.25, -0.5, 0.0, 0.75], [0.0, 0.0, 0.0, 0.0, 1.0], [0.5, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0, -0.125], [1.5, 0.0, 0.0], [0.0, 0.0]):
        _same("coefficients %s" % coeffs, g.poly_eval(r.x[:2], s, coeffs, s), r.want(s, coeffs, s, 2))


def test_the_devices_own_sequence_of_calls_gives_the_same_words(seven):
    """mul_relin / rescale / mod_switch per power, then one multiply_const_sum_rescale over the powers at their own levels"""
    r, s, g = seven, 2.0 ** 30, seven.g
    coeffs = COEFFS[:6]
    p = spec.plan(r.o.primes, r.L, s, coeffs, s)
    pw = {1: np.ascontiguousarray(r.x[:2])}
    for k in range(2, p["d"] + 1):
        b = pw[p["lo"][k]]
        while b.shape[2] > p["level"][k] + 1:
            b = g.mod_switch(b)
        pw[k] = g.rescale(g.mul_relin(pw[p["hi"][k]], b))
        assert pw[k].shape[2] == p["level"][k]
    weights = np.stack([g.const_words(coeffs[k], s * r.o.primes[p["m"] - 1] / p["scale"][k], p["m"]) for k in p["terms"]])
    _same("the words of the plan", weights, np.stack(p["weights"]))
    w0 = g.const_words(coeffs[0], s * r.o.primes[p["m"] - 1], p["m"])
    own = g.multiply_const_sum_rescale([pw[k] for k in p["terms"]], weights, const=w0, nl=p["m"])
    _same("composed on the device", own, g.poly_eval(r.x[:2], s, coeffs, s))
    _same("... and the spec", own, r.want(s, coeffs, s, 2))


@pytest.mark.parametrize("lanes,chunk", [(1, 2), (2, 1), (2, 2)], ids=["one-lane", "two-lanes", "two-lanes-one-group"])
def test_groups_with_a_ragged_last_one(seven, lanes, chunk):
    """ABC_HIP_CHUNK=c: groups of exactly c * lanes ciphertexts; five ciphertexts leave a ragged last group (or none: 2 x 2 < 5 too)"""
    r, s, g = seven, 2.0 ** 30, seven.g
    coeffs = COEFFS[:4]
    with _env(g, {"ABC_HIP_CHUNK": str(chunk), "ABC_HIP_LANES": str(lanes)}):
        _same("chunk %d lanes %d" % (chunk, lanes), g.poly_eval(r.x, s, coeffs, s), r.want(s, coeffs, s))


@pytest.mark.parametrize("n,bits,degree,count,env,route", [
    (1024, [60, 40, 40, 40, 60], 3, 2, {}, None),
    (16384, [50, 40, 40, 40, 50], 3, 2, {}, "split14"),
    (16384, [50, 40, 40, 40, 50], 3, 1, {"ABC_HIP_NO_SPLIT": "1"}, None),
    (32768, [50, 40, 40, 50], 2, 1, {}, None),
], ids=["mixed-2^10", "2^14", "2^14-no_split", "2^15"])
def test_other_chains_and_rings(oracle_mod, capi, n, bits, degree, count, env, route):
    r = Rig(oracle_mod, capi, n, bits, n + degree, count)
    try:
        with _env(r.g, env):
            got_route = r.g.route("poly_eval", r.L, count)
            assert got_route.endswith(" constsum=separate") and got_route == r.g.route("mul_relin", r.L, count) + " constsum=separate"
            if route:
                assert got_route.startswith(route), got_route
            else:
                assert not got_route.startswith("split14"), got_route
            x_scale, out_scale = 2.0 ** 40, 2.0 ** 20
            coeffs = COEFFS[: degree + 1]
            _same("%s degree %d" % (got_route, degree), r.g.poly_eval(r.x, x_scale, coeffs, out_scale), r.want(x_scale, coeffs, out_scale))
    finally:
        r.close()


def test_refused_calls_leave_the_output_untouched(seven, capi):
    r, s, g = seven, 2.0 ** 30, seven.g
    n, L, count = r.n, r.L, 2
    d_x = g.upload(r.x[:count])
    sentinel = np.full((count, 2, L - 1, n), SENTINEL, dtype=np.uint64)
    d_o = g.upload(sentinel)
    held = g.held_buffers()

    def call(coeffs=(0.5, 0.25, 0.125), x_scale=s, out_scale=s, nl=L, out=None, x=None, degree=None):
        co = (C.c_double * max(len(coeffs), 1))(*coeffs)
        g.op("ckks_poly_eval", x or d_x.ptr, C.c_double(x_scale), co, len(coeffs) - 1 if degree is None else degree, C.c_double(out_scale),
             out or d_o.ptr, nl, C.c_size_t(count))

    for degree in (0, -1, 32):
        with pytest.raises(capi.AbcHipError, match="degree must be in 1 .. 31"):
            call(coeffs=[0.5] * 33, degree=degree)
    with pytest.raises(capi.AbcHipError, match="chain is too short"):
        call(nl=2)  # degree 2: E = 1, nl >= 3
    with pytest.raises(capi.AbcHipError, match="chain is too short"):
        call(coeffs=[0.1] * 10, nl=5)  # degree 9: E = 4, nl >= 6
    for level in (0, L + 1):
        with pytest.raises(capi.AbcHipError, match="limb count out of range"):
            call(nl=level)
    for bad in (0.0, -s, float("inf"), float("nan")):
        with pytest.raises(capi.AbcHipError, match="scales must be finite and positive"):
            call(x_scale=bad)
        with pytest.raises(capi.AbcHipError, match="scales must be finite and positive"):
            call(out_scale=bad)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(capi.AbcHipError, match="a coefficient is not finite"):
            call(coeffs=(0.5, bad, 0.25))
    with pytest.raises(capi.AbcHipError, match="2\\^62"):
        call(out_scale=2.0 ** 40)  # the constant term at 2^40 * q_{m-1}
    with pytest.raises(capi.AbcHipError, match="2\\^62"):
        call(coeffs=(0.0, 2.0 ** 40, 0.25))
    at = lambda buf, k: C.c_void_p(buf.ptr.value + 8 * k)  # noqa: E731
    with pytest.raises(capi.AbcHipError, match="must not overlap d_x"):
        call(out=at(d_x, count * 2 * L * n - 1))
    with pytest.raises(capi.AbcHipError, match="must not overlap d_x"):
        call(x=at(d_o, 1))
    g.sync()
    _same("refused calls wrote nothing", g.download(d_o, sentinel.shape), sentinel)
    _same("... nor to x", g.download(d_x, r.x[:count].shape), r.x[:count])
    assert g.held_buffers() == held
    # no relinearisation key; a BFV context
    bare = capi.Context(capi.CKKS, n, r.o.primes)
    gb = capi.Context.bfv_default(4096)
    try:
        b_x, b_o = bare.upload(r.x[:1]), bare.upload(sentinel[:1])
        co = (C.c_double * 3)(0.5, 0.25, 0.125)
        with pytest.raises(capi.AbcHipError, match="no relinearisation key"):
            bare.op("ckks_poly_eval", b_x.ptr, C.c_double(s), co, 2, C.c_double(s), b_o.ptr, L, C.c_size_t(1))
        bare.sync()
        _same("no key: nothing written", bare.download(b_o, sentinel[:1].shape), sentinel[:1])
        f_x = gb.upload(np.zeros((1, 2, gb.L, gb.n), dtype=np.uint64))
        with pytest.raises(capi.AbcHipError, match="is a CKKS operation"):
            gb.op("ckks_poly_eval", f_x.ptr, C.c_double(s), co, 2, C.c_double(s), f_x.ptr, gb.L, C.c_size_t(1))
    finally:
        bare.close()
        gb.close()
    call()
    _same("after the refusals", g.download(d_o, (count, 2, L - 2, n)), r.want(s, (0.5, 0.25, 0.125), s, count))
    d_x.free(); d_o.free()


def test_count_zero(seven):
    r, s, g = seven, 2.0 ** 30, seven.g
    sentinel = np.full((1, 2, r.L - 2, r.n), SENTINEL, dtype=np.uint64)
    d_x, d_o = g.upload(r.x[:1]), g.upload(sentinel)
    co = (C.c_double * 3)(0.5, 0.25, 0.125)
    g.op("ckks_poly_eval", d_x.ptr, C.c_double(s), co, 2, C.c_double(s), d_o.ptr, r.L, C.c_size_t(0))
    g.sync()
    _same("count = 0 writes nothing", g.download(d_o, sentinel.shape), sentinel)
    d_x.free(); d_o.free()


def test_recorded_call_follows_its_input(seven):
    """eagerly once (the arenas get their size), recorded, replayed twice on a rewritten x; the weights are part of the record"""
    r, s, g = seven, 2.0 ** 30, seven.g
    coeffs, count = COEFFS[:6], 2
    want = r.want(s, coeffs, s)
    d_x = g.upload(r.x[:count])
    d_o = g.alloc(want[:count].nbytes)
    co = (C.c_double * len(coeffs))(*coeffs)
    held = g.held_buffers()

    def circuit():
        g.op("ckks_poly_eval", d_x.ptr, C.c_double(s), co, len(coeffs) - 1, C.c_double(s), d_o.ptr, r.L, C.c_size_t(count))

    circuit()
    g.sync()
    g.graph_begin()
    circuit()
    exe = g.graph_end()
    try:
        for turn, pick in enumerate(([0, 1], [2, 3], [4, 1])):
            x2 = np.ascontiguousarray(r.x[pick])
            g.op("memcpy_h2d", d_x.ptr, x2.ctypes.data_as(C.c_void_p), C.c_size_t(x2.nbytes))
            fill = np.full(want[:count].shape, SENTINEL, dtype=np.uint64)
            g.op("memcpy_h2d", d_o.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes))
            if turn:
                g.graph_launch(exe)
            else:
                circuit()
            _same("turn %d" % turn, g.download(d_o, fill.shape), want[pick])
    finally:
        g.graph_destroy(exe)
    assert g.held_buffers() == held
    d_x.free(); d_o.free()


def test_a_degree_3_sigmoid_from_encode_to_decode(seven):
    """sigmoid(x) ~ 0.5 + 0.197 x - 0.004 x^3 on [-4, 4] (the usual least-squares cubic): encode, encrypt, poly_eval, decrypt, decode"""
    r, s, g, o = seven, 2.0 ** 30, seven.g, seven.o
    rng = np.random.default_rng(3)
    x = rng.uniform(-4, 4, (2, r.n // 2))
    coeffs = [0.5, 0.197, 0.0, -0.004]
    ct = np.stack([o.encrypt(o.ckks_encode(v, s), 40 + i) for i, v in enumerate(x)])
    out = g.poly_eval(ct, s, coeffs, s)
    got = np.stack([o.ckks_decode(o.decrypt(c), s) for c in out])
    clear = np.polynomial.polynomial.polyval(x, coeffs)
    err = np.abs(got - clear).max()
    print("degree-3 sigmoid, slots in [-4, 4]: max |error| %.3g against numpy's polynomial, %.3g against the sigmoid itself" % (err, np.abs(got.real - 1 / (1 + np.exp(-x))).max()))
    assert err < BOUND
    _same("and the spec's words", out, np.stack([spec.poly_eval(o, c, s, coeffs, s) for c in ct]))
