"""CKKS slot encoder / decoder on the device (abc_hip_ckks_encode / abc_hip_ckks_decode) against the CPU oracle's
orc_ckks_encode / orc_ckks_decode (the yardstick: same slot order, N-point transform in long double for the lift).

Encoding is floating point, so it is not a bit-parity target: coefficients may differ by one unit of rounding, decoded
values by the transform's rounding.  Batch invariance, by contrast, is bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAINS = {"50-40": [50, 40, 40, 40, 50], "60-40": [60, 40, 40, 40, 60]}
DEEP = [50] + [40] * 14 + [50]
SCALE = 2.0 ** 40


@pytest.fixture(scope="module")
def contexts(oracle_mod, capi):
    cache = {}

    def get(n, bits):
        key = (n, tuple(bits))
        if key not in cache:
            primes = oracle_mod.create_primes(n, bits)
            assert capi.create_primes(n, bits) == primes
            o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)  # the codec needs no keys
            g = capi.Context(capi.CKKS, n, primes)
            cache[key] = (o, g)
        return cache[key]
    yield get
    for o, g in cache.values():
        g.close()


def _grid():
    for logn in (10, 11, 12, 13, 14, 15, 16):
        for name, bits in CHAINS.items():
            yield pytest.param(1 << logn, bits, id="N%d-%s" % (1 << logn, name))
    yield pytest.param(1 << 16, [60, 50, 50, 50, 50, 50, 50, 50, 60], id="N65536-8limbs")
    yield pytest.param(1 << 14, DEEP, id="N16384-15limbs")


def _levels(o):
    """the deep chain: both sides of the decoder's 8-word / 16-word lift (SrcLift<8> up to eight limbs, SrcLift<16> above)"""
    return [1, 8, 9, 12, 15] if o.L == 15 else sorted({1, o.L})


def _values(rng, n, count, cplx):
    v = rng.uniform(-1, 1, count)
    return v + 1j * rng.uniform(-1, 1, count) if cplx else v


def _coeffs(o, plain):
    """NTT form -> centred integer coefficients (every limb must encode the same small integer)"""
    nl = plain.shape[0]
    cols = []
    for j in range(nl):
        q = o.primes[j]
        c = o.intt(j, plain[j]).astype(object)
        cols.append(np.where(c > q // 2, c - q, c))
    return cols


def _assert_close_coeffs(o, got, want, what):
    g, w = _coeffs(o, got), _coeffs(o, want)
    for j in range(len(g)):
        assert np.array_equal(g[j], g[0]), "%s: limb %d encodes another integer than limb 0" % (what, j)
        d = np.abs((g[j] - w[j]).astype(np.float64)).max()
        assert d <= 1, "%s: limb %d coefficients differ by %g" % (what, j, d)


@pytest.mark.parametrize("n,bits", list(_grid()))
def test_encode_matches_oracle(contexts, n, bits):
    o, g = contexts(n, bits)
    rng = np.random.default_rng(n + len(bits))
    for nl in _levels(o):
        for cplx in (False, True):
            for count in (n // 2, n // 2 - 37):
                v = _values(rng, n, count, cplx)
                what = "N=%d nl=%d complex=%s values=%d" % (n, nl, cplx, count)
                got = g.ckks_encode(v, SCALE, nl)
                assert got.shape == (nl, n)
                _assert_close_coeffs(o, got, o.ckks_encode(v, SCALE, nl), what)
                dec = o.ckks_decode(got, SCALE)
                want = np.zeros(n // 2, complex)
                want[:count] = v
                err = np.abs(dec - want) / np.maximum(1.0, np.abs(want))
                assert err.max() <= 1e-7, "%s: oracle decodes the device plaintext %g off" % (what, err.max())


@pytest.mark.parametrize("n,bits", list(_grid()))
def test_decode_matches_oracle(contexts, n, bits):
    o, g = contexts(n, bits)
    rng = np.random.default_rng(2 * n + len(bits))
    for nl in _levels(o):
        enc = o.ckks_encode(_values(rng, n, n // 2, True), SCALE, nl)
        # uniformly random residues: the full-width centred lift, both halves of (-Q/2, Q/2]
        rnd = np.stack([rng.integers(0, o.primes[j], n, dtype=np.uint64) for j in range(nl)])
        for what, plain in (("oracle encoding", enc), ("random residues", rnd)):
            want = o.ckks_decode(plain, SCALE)
            got = g.ckks_decode(plain, SCALE)
            tol = 1e-9 * max(1.0, np.abs(want).max())
            assert np.abs(got - want).max() <= tol, "N=%d nl=%d %s: max error %g > %g" % (
                n, nl, what, np.abs(got - want).max(), tol)


@pytest.mark.parametrize("n,bits", list(_grid()))
def test_round_trip(contexts, n, bits):
    o, g = contexts(n, bits)
    rng = np.random.default_rng(3 * n)
    for nl in (_levels(o) if o.L == 15 else range(1, o.L + 1)):
        v = _values(rng, n, n // 2, True)
        got = g.ckks_decode(g.ckks_encode(v, SCALE, nl), SCALE)
        err = np.abs(got - v) / np.maximum(1.0, np.abs(v))
        assert err.max() <= 1e-7, "N=%d nl=%d: round trip %g off" % (n, nl, err.max())


@pytest.mark.parametrize("nl", [1, 8, 9, 12, 15])
def test_decode_lift_exact_on_a_constant(contexts, nl):
    """The lift alone, without the oracle's long double: the constant polynomial V = Q // 3 (Q: the product of the first nl primes)
    and its negative Q - V.  In NTT form every word of limb j is V mod q_j, and every slot of a constant is the constant, so each
    must decode to +-float(V) / scale.  Bound 1e-12 relative: at most 16 roundings in the word Horner plus an 8192-point
    transform of a constant come to a few 1e-15."""
    n = 1 << 14
    o, g = contexts(n, DEEP)
    Q = 1
    for q in o.primes[:nl]:
        Q *= q
    V = Q // 3
    for sign, value in ((1.0, V), (-1.0, Q - V)):
        plain = np.stack([np.full(n, value % q, dtype=np.uint64) for q in o.primes[:nl]])
        got = g.ckks_decode(plain, SCALE)
        want = sign * float(V) / SCALE
        assert np.abs(got.real - want).max() <= 1e-12 * abs(want), "nl=%d sign %+d: real part %g off (relative)" % (
            nl, sign, np.abs(got.real - want).max() / abs(want))
        assert np.abs(got.imag).max() <= 1e-12 * abs(want), "nl=%d sign %+d: imaginary part %g (relative)" % (
            nl, sign, np.abs(got.imag).max() / abs(want))


def test_pipeline_without_host_codec(contexts):
    """device encode -> encrypt -> mul_relin -> rescale -> decrypt -> device decode (test_gpu_parity's CKKS check)"""
    n = 16384
    o, g = contexts(n, CHAINS["50-40"])
    rng = np.random.default_rng(7)
    g.keygen(0xC0DEC)
    x, y = rng.uniform(-1, 1, n // 2), rng.uniform(-1, 1, n // 2)
    cx, cy = g.encrypt(g.ckks_encode(x, SCALE), seed=11), g.encrypt(g.ckks_encode(y, SCALE), seed=12)
    plain = g.decrypt(g.rescale(g.mul_relin(cx, cy)))
    assert plain.shape == (o.L - 1, n)
    dec = g.ckks_decode(plain, SCALE * SCALE / o.primes[o.L - 1])
    assert np.abs(dec.real - x * y).max() < 1e-4
    assert np.abs(dec.imag).max() < 1e-4


@pytest.mark.parametrize("n", [1 << 13, 1 << 16])
def test_batch_invariance(contexts, n):
    o, g = contexts(n, CHAINS["60-40"])
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1, 1, (3, 1000)) + 1j * rng.uniform(-1, 1, (3, 1000))
    batch = g.ckks_encode(rows, SCALE)
    assert batch.shape == (3, o.L, n)
    for b in range(3):
        assert np.array_equal(batch[b], g.ckks_encode(rows[b], SCALE)), "encode row %d" % b
    dec = g.ckks_decode(batch, SCALE)
    assert dec.shape == (3, n // 2)
    for b in range(3):
        assert np.array_equal(dec[b], g.ckks_decode(batch[b], SCALE)), "decode row %d" % b


def test_error_paths(contexts, capi):
    n = 4096
    o, g = contexts(n, CHAINS["50-40"])
    v = np.linspace(-1, 1, 64)
    bfv = capi.Context.bfv_default(4096)
    with pytest.raises(capi.AbcHipError, match="CKKS"):
        bfv.ckks_encode(v, SCALE, 1)
    with pytest.raises(capi.AbcHipError, match="CKKS"):
        bfv.ckks_decode(np.zeros((1, n), np.uint64), SCALE)
    bfv.close()
    for nl in (0, o.L + 1):
        with pytest.raises(capi.AbcHipError, match="limb count"):
            g.ckks_encode(v, SCALE, nl)
    with pytest.raises(capi.AbcHipError, match="limb count"):
        g.ckks_decode(np.zeros((o.L + 1, n), np.uint64), SCALE)
    with pytest.raises(capi.AbcHipError, match="values_per_row"):
        g.ckks_encode(np.zeros(n // 2 + 1), SCALE)
    big = np.full(n // 2, 2.0)  # constant polynomial 2: coefficient 0 is 2 * scale
    with pytest.raises(AssertionError):
        o.ckks_encode(big, 9e18)  # the oracle refuses (-2) ...
    with pytest.raises(capi.AbcHipError, match="2\\^62"):
        g.ckks_encode(big, 9e18)  # ... and so does the device, whose bound 2^62 lies inside the oracle's
    # the context is still usable
    _assert_close_coeffs(o, g.ckks_encode(v, SCALE), o.ckks_encode(v, SCALE), "after errors")
    assert np.abs(g.ckks_decode(g.ckks_encode(v, SCALE), SCALE)[:64] - v).max() < 1e-7
