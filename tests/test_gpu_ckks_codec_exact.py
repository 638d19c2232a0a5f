"""abc_hip_ckks_encode / abc_hip_ckks_decode against an exact reference (tests/ckks_codec_spec.py: long double transform, Python
integers), where tests/test_gpu_ckks_codec.py compares with the oracle's fp64 encoder to one unit.

Margins and tolerances are 8 x the fp64 error the spec measures between its own two precisions (spec.FP64_ERR, checked on the CPU by
tests/test_ckks_codec_spec.py): three bits for the device's other summation order and FMA contraction.  Nothing here is taken from
what the device returns.  Rounding rule: nearest, ties away from zero (include/abc_hip.h).

Sections: A encode word for word, B ties, C large magnitudes and the 2^62 boundary, D non-finite input, E argument forms,
F second passes of the chunk loops, G decode against the exact lift, H round trip.
"""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_codec_spec as spec  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
CHAINS = {"50-40": [50, 40, 40, 50], "60-40": [60, 40, 40, 60], "50-30": [50, 30, 30, 30, 50], "60-30": [60, 30, 30, 30, 60],
          "60x16": [60] * 16}


@pytest.fixture(scope="module")
def contexts(oracle_mod, capi):
    cache = {}

    def get(n, name):
        key = (n, name)
        if key not in cache:
            primes = oracle_mod.create_primes(n, CHAINS[name])
            assert capi.create_primes(n, CHAINS[name]) == primes
            cache[key] = (oracle_mod.Oracle(oracle_mod.CKKS, n, primes), capi.Context(capi.CKKS, n, primes))  # the codec needs no keys
        return cache[key]
    yield get
    for o, g in cache.values():
        g.close()


# ---- raw calls: device pointers in, status out ----
def _at(buf, nbytes=0):
    return C.c_void_p(buf.ptr.value + nbytes)


def _encode_status(capi, g, re, im, vpr, scale, nl, out, count):
    return capi.lib().abc_hip_ckks_encode(g.h, re, im, C.c_size_t(vpr), C.c_double(scale), C.c_int(nl), out, C.c_size_t(count))


def _download(capi, g, ptr, shape, dtype=np.uint64):
    out = np.empty(shape, dtype)
    assert capi.lib().abc_hip_memcpy_d2h(g.h, out.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(out.nbytes)) == 0
    return out


def _words(o, coeffs, nl):
    """integer coefficients (|c| < 2^63) -> NTT-form words of limbs 0 .. nl-1"""
    c = np.array([int(x) for x in coeffs], dtype=np.int64)
    return np.stack([o.ntt(j, np.mod(c, np.int64(o.primes[j])).astype(np.uint64)) for j in range(nl)])


def _coeff_form(o, plain):
    return [o.intt(j, plain[j]) for j in range(plain.shape[0])]


def _lift(o, plain):
    """NTT-form words [nl][N] -> (centred Python integers of the full CRT lift over all nl limbs, Q)"""
    return spec.crt_centred(_coeff_form(o, plain), o.primes)


def _centred_diff(a, b, Q):
    d = (a - b) % Q
    return np.array([int(x) - Q if x > Q // 2 else int(x) for x in d], dtype=object)


def _round_away(value, scale):
    x = Fraction(value) * Fraction(scale)  # both doubles: exact
    r = int(abs(x) + Fraction(1, 2))  # floor(|x| + 1/2)
    return -r if x < 0 else r


# ---- A. encode, word for word ----
@pytest.mark.parametrize("top", [False, True], ids=["nl1", "nlL"])
@pytest.mark.parametrize("name", ["50-40", "60-40", "50-30"])
@pytest.mark.parametrize("logn", spec.RINGS)
def test_encode_exact(contexts, logn, name, top):
    """Scale 2^20: the reference has no coefficient within the margin of a tie (asserted on the CPU for these seeds), so every word
    of every limb is the reference's.  Scale 2^40: every coefficient farther than the margin from a tie is equal, the rest within one
    unit, and they are under 0.5 % of the row.  Integers compared after a CRT lift of all limbs (modulo Q where one limb is
    narrower than the coefficient)."""
    n = 1 << logn
    o, g = contexts(n, name)
    nl = o.L if top else 1
    for cplx in (False, True):
        for short in (False, True):
            what = "N=2^%d %s nl=%d complex=%s short=%s" % (logn, name, nl, cplx, short)
            v, want, dist = spec.encode_case_reference(logn, cplx, short, 20)
            assert dist.min() > spec.encode_margin(logn, 20)
            got = g.ckks_encode(v, 2.0 ** 20, nl)
            bad = int((got != _words(o, want, nl)).sum())
            assert bad == 0, "%s scale 2^20: %d of %d words differ from the exact encoding" % (what, bad, got.size)
            v, want, dist = spec.encode_case_reference(logn, cplx, short, 40)
            lifted, Q = _lift(o, g.ckks_encode(v, 2.0 ** 40, nl))
            d = _centred_diff(lifted, want, Q)
            near = dist <= spec.encode_margin(logn, 40)
            share = float(near.mean())
            print("%s scale 2^40: %.4f %% of the coefficients within the margin of a tie, %d of them one unit off" % (
                what, 100 * share, int(np.count_nonzero(d[near]))))
            assert share < 5e-3, "%s: %.3f %% of the row left out" % (what, 100 * share)
            assert not np.any(d[~near]), "%s scale 2^40: %d decidable coefficients differ" % (what, int(np.count_nonzero(d[~near])))
            assert all(abs(x) <= 1 for x in d[near]), "%s scale 2^40: a coefficient near a tie is more than one unit off" % what


# ---- B. ties ----
TIES = [(0.5, 1.0), (-0.5, 1.0), (1.5, 1.0), (2.5, 1.0), (-2.5, 1.0), (2.0 ** 40 + 0.5, 1.0), (0.5 * 2.0 ** -40, 2.0 ** 40)]


@pytest.mark.parametrize("half", [False, True], ids=["coef0", "coefN/2"])
@pytest.mark.parametrize("value,scale", TIES, ids=["0.5", "-0.5", "1.5", "2.5", "-2.5", "2^40+0.5", "2^-41@2^40"])
@pytest.mark.parametrize("logn", [10, 15])
def test_encode_ties_round_away_from_zero(contexts, logn, value, scale, half):
    """A constant slot vector c makes every butterfly sum exact, so coefficient 0 is exactly c * scale: a tie the device must take
    away from zero, as abc_hip_ckks_const_words does.  The slots +-i c (sign + where 3^i = 1 mod 4, i.e. i even) are those of
    c X^(N/2): the same tie through the other store of the last pass.  N = 2^10 is the one-pass store, 2^15 the four-step one."""
    n = 1 << logn
    o, g = contexts(n, "60-40")
    nl = o.L
    r = _round_away(value, scale)
    assert abs(r) == abs(int(value * scale)) + 1  # a tie indeed: away from zero is one past the truncation
    slots = np.full(n // 2, value, dtype=complex)
    if half:
        slots = slots * 1j * np.where(np.arange(n // 2) % 2 == 0, 1.0, -1.0)
    got = g.ckks_encode(slots, scale, nl)
    poly = np.zeros(n, dtype=object)
    poly[n // 2 if half else 0] = r
    want = _words(o, poly, nl)
    cw = g.const_words(value, scale, nl)
    assert [int(x) for x in cw] == [r % q for q in o.primes[:nl]]
    at = _coeff_form(o, got)
    assert np.array_equal(got, want), "c=%r scale=%g: coefficient %d is %s, want %s; other words %s" % (
        value, scale, n // 2 if half else 0, [int(a[n // 2 if half else 0]) for a in at], [r % q for q in o.primes[:nl]],
        "zero" if sum(int(np.count_nonzero(a)) for a in at) <= nl else "not all zero")
    if not half:
        for j in range(nl):
            assert np.all(got[j] == cw[j])  # NTT form of a constant: every word is the constant's word
    else:
        assert [int(a[n // 2]) for a in at] == [int(x) for x in cw]


# ---- C. large magnitudes and the 2^62 boundary ----
BIG = float(2 ** 62 - 512)  # the largest double below 2^62


@pytest.mark.parametrize("name", ["60-40", "50-30", "60-30"])
@pytest.mark.parametrize("logn", [12, 15])
def test_encode_accepts_up_to_the_bound_and_reduces_exactly(contexts, capi, logn, name):
    """+-(2^62 - 512) as a constant: accepted, every limb the exact residue of a magnitude far above its 60-, 40- or 30-bit prime
    (reduce64); +-2^62: status 2 with the 2^62 text, and the context stays usable."""
    n = 1 << logn
    o, g = contexts(n, name)
    nl = o.L
    for value in (BIG, -BIG):
        got = g.ckks_encode(np.full(n // 2, value), 1.0, nl)
        for j in range(nl):
            want = int(value) % o.primes[j]
            assert np.all(got[j] == np.uint64(want)), "constant %r limb %d (q = %d): words are not %d" % (value, j, o.primes[j], want)
        assert [int(x) for x in g.const_words(value, 1.0, nl)] == [int(value) % q for q in o.primes[:nl]]
    re = g.upload(np.full(n // 2, 2.0 ** 62))
    out = g.alloc(nl * n * 8)
    neg = g.upload(np.full(n // 2, -(2.0 ** 62)))
    for buf in (re, neg):
        assert _encode_status(capi, g, buf.ptr, None, n // 2, 1.0, nl, out.ptr, 1) == 2
        assert "2^62" in capi.lib().abc_hip_last_error().decode()
    for b in (re, neg, out):
        b.free()
    assert np.all(g.ckks_encode(np.full(n // 2, BIG), 1.0, 1)[0] == np.uint64(int(BIG) % o.primes[0]))


@pytest.mark.parametrize("name", ["60-30", "60-40"])
@pytest.mark.parametrize("logn", [10, 12])
def test_encode_large_coefficients(contexts, logn, name):
    """Random slots in the unit square at scale 2^58: coefficients around 2^52 .. 2^55, far above the 30- and 40-bit primes.  The
    integer lifted from all limbs is within the margin (+ the half unit of rounding) of the unrounded long-double coefficient, and
    every limb is the residue of the one integer limb 0 (60 bits) holds."""
    n = 1 << logn
    o, g = contexts(n, name)
    nl = o.L
    v = spec.fp64_inputs(99 + logn, n)
    c = spec.encode_unrounded(v, 2.0 ** 58, n)
    assert 2.0 ** 52 < float(np.abs(c).max()) < 2.0 ** 56
    got = g.ckks_encode(v, 2.0 ** 58, nl)
    lifted, Q = _lift(o, got)
    err = float(np.abs(spec.to_longdouble(lifted) - c).max())
    bound = spec.encode_margin(logn, 58) + 0.5
    print("N=2^%d %s scale 2^58: largest coefficient 2^%.1f, %.3g units from the reference (bound %.3g)" % (
        logn, name, np.log2(float(np.abs(c).max())), err, bound))
    assert err <= bound
    coef = _coeff_form(o, got)
    q0 = o.primes[0]
    one = [int(x) - q0 if int(x) > q0 // 2 else int(x) for x in coef[0]]
    for j in range(1, nl):
        assert [int(x) for x in coef[j]] == [x % o.primes[j] for x in one], "limb %d is not the residue of limb 0's integer" % j


# ---- D. non-finite input ----
@pytest.mark.parametrize("part", ["re", "im"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("logn", [11, 15])
def test_non_finite_value_fails_the_call_and_the_flag_resets(contexts, capi, logn, bad, part):
    n = 1 << logn
    o, g = contexts(n, "50-40")
    nl, vpr = o.L, 5
    rows = np.linspace(-1, 1, 3 * vpr).reshape(3, vpr)
    rows_bad = rows.copy()
    rows_bad[2, 3] = bad
    re, im = g.upload(rows_bad if part == "re" else rows), g.upload(rows_bad if part == "im" else rows)
    out = g.alloc(3 * nl * n * 8)
    assert _encode_status(capi, g, re.ptr, im.ptr, vpr, 2.0 ** 20, nl, out.ptr, 3) == 2
    msg = capi.lib().abc_hip_last_error().decode()
    assert "2^62" in msg and "not finite" in msg
    for b in (re, im, out):
        b.free()
    v, want, _ = spec.encode_case_reference(logn, True, False, 20)
    assert np.array_equal(g.ckks_encode(v, 2.0 ** 20, nl), _words(o, want, nl)), "the call after a refused one is not exact"


# ---- E. forms ----
def test_encode_forms(contexts):
    """values_per_row 0 with d_re NULL; values_per_row 1; d_im NULL against an all-zero d_im -- through Context.op, explicit pointers"""
    logn = 11
    n = 1 << logn
    o, g = contexts(n, "50-40")
    nl, scale = o.L, 2.0 ** 20
    out = g.upload(np.full((2, nl, n), 0xDEADBEEF, dtype=np.uint64))
    g.op("ckks_encode", None, None, C.c_size_t(0), C.c_double(scale), nl, out.ptr, C.c_size_t(2))
    assert not g.download(out, (2, nl, n)).any(), "no values: the plaintext is not zero"
    for value in (0.7310585786300049, -0.2689414213699951 + 0.6224593312018546j):
        ints, _, dist = spec.encode_exact([value], scale, n, [])
        assert dist.min() > spec.encode_margin(logn, 20)
        re, im = g.upload(np.array([value.real])), g.upload(np.array([value.imag]))
        g.op("ckks_encode", re.ptr, im.ptr, C.c_size_t(1), C.c_double(scale), nl, out.ptr, C.c_size_t(1))
        assert np.array_equal(g.download(out, (nl, n)), _words(o, ints, nl)), "one value per row"
        re.free(), im.free()
    rows = np.linspace(-1, 1, 2 * 100).reshape(2, 100)
    re, zero = g.upload(rows), g.upload(np.zeros_like(rows))
    out2 = g.alloc(2 * nl * n * 8)
    g.op("ckks_encode", re.ptr, None, C.c_size_t(100), C.c_double(scale), nl, out.ptr, C.c_size_t(2))
    g.op("ckks_encode", re.ptr, zero.ptr, C.c_size_t(100), C.c_double(scale), nl, out2.ptr, C.c_size_t(2))
    a = g.download(out, (2, nl, n))
    assert np.array_equal(a, g.download(out2, (2, nl, n)))
    ints, _, dist = spec.encode_exact(rows[1], scale, n, [])
    assert dist.min() > spec.encode_margin(logn, 20)
    assert np.array_equal(a[1], _words(o, ints, nl))
    for b in (re, zero, out, out2):
        b.free()


@pytest.mark.parametrize("logn", [11, 15])
def test_decode_without_imaginary_output(contexts, logn):
    """d_im NULL: the same real parts, and nothing written past them (a guard region behind d_re keeps its pattern)"""
    n = 1 << logn
    o, g = contexts(n, "50-40")
    nl, m, guard = o.L, n // 2, 4096
    plain = g.ckks_encode(spec.encode_case_values(logn, True, False).reshape(1, -1).repeat(2, 0) * np.array([[1.0], [0.5]]), 2.0 ** 40, nl)
    pb = g.upload(plain)
    re, im = g.alloc(2 * m * 8), g.alloc(2 * m * 8)
    g.op("ckks_decode", pb.ptr, nl, C.c_double(2.0 ** 40), re.ptr, im.ptr, C.c_size_t(2))
    both = g.download(re, (2 * m,), np.float64)
    pattern = np.full(2 * m + guard, 0x7FF8DEADBEEF0000, dtype=np.uint64)
    lone = g.upload(pattern)
    g.op("ckks_decode", pb.ptr, nl, C.c_double(2.0 ** 40), lone.ptr, None, C.c_size_t(2))
    back = g.download(lone, (2 * m + guard,))
    assert np.array_equal(back[:2 * m].view(np.float64), both)
    assert np.all(back[2 * m:] == pattern[2 * m:]), "words behind d_re were written"
    for b in (pb, re, im, lone):
        b.free()


# ---- F. second passes of the chunk loops ----
def _second_pass(capi, o, g, n, enc_rows, enc_chunk, dec_rows, dec_chunk):
    m, scale = n // 2, 2.0 ** 40
    rng = np.random.default_rng(n + enc_rows)
    vals = rng.uniform(-1, 1, (enc_rows, 2)) + 1j * rng.uniform(-1, 1, (enc_rows, 2))  # every row its own values
    re, im = g.upload(np.ascontiguousarray(vals.real)), g.upload(np.ascontiguousarray(vals.imag))
    plain = g.alloc(enc_rows * n * 8)
    one = g.alloc(n * 8)
    g.op("ckks_encode", re.ptr, im.ptr, C.c_size_t(2), C.c_double(scale), 1, plain.ptr, C.c_size_t(enc_rows))
    for b in (0, enc_chunk - 1, enc_chunk, enc_rows - 1):
        g.op("ckks_encode", _at(re, b * 16), _at(im, b * 16), C.c_size_t(2), C.c_double(scale), 1, one.ptr, C.c_size_t(1))
        assert np.array_equal(_download(capi, g, _at(plain, b * n * 8), (n,)), g.download(one, (n,))), "encode row %d of %d" % (b, enc_rows)
    ints, _, dist = spec.encode_exact(vals[enc_chunk], scale, n, [])  # and the first row of pass two is the right plaintext at all
    d = _centred_diff(_lift(o, _download(capi, g, _at(plain, enc_chunk * n * 8), (1, n)))[0], ints, o.primes[0])
    assert not np.any(d[dist > spec.encode_margin(n.bit_length() - 1, 40)])
    for b in (re, im):
        b.free()
    dre, dim = g.alloc(dec_rows * m * 8), g.alloc(dec_rows * m * 8)
    ore, oim = g.alloc(m * 8), g.alloc(m * 8)
    g.op("ckks_decode", plain.ptr, 1, C.c_double(scale), dre.ptr, dim.ptr, C.c_size_t(dec_rows))
    for b in (0, dec_chunk - 1, dec_chunk, dec_rows - 1):
        g.op("ckks_decode", _at(plain, b * n * 8), 1, C.c_double(scale), ore.ptr, oim.ptr, C.c_size_t(1))
        for batch, single, part in ((dre, ore, "re"), (dim, oim, "im")):
            assert np.array_equal(_download(capi, g, _at(batch, b * m * 8), (m,)), g.download(single, (m,))), "decode row %d of %d, %s" % (
                b, dec_rows, part)
        z = _download(capi, g, _at(dre, b * m * 8), (2,), np.float64) + 1j * _download(capi, g, _at(dim, b * m * 8), (2,), np.float64)
        assert np.abs(z - vals[b]).max() < 1e-6, "decode row %d does not hold row %d's values" % (b, b)
    for b in (plain, one, dre, dim, ore, oim):
        b.free()
    g.trim()


def test_second_pass_four_step(contexts, capi):
    """N = 2^15, nl = 1.  Encode: 1025 rows, one past kScratchCap (256 MiB) / 256 KiB of four-step intermediate = 1024 rows a pass.
    Decode: 513 rows, one past kScratchCap / (256 KiB coefficients + 256 KiB intermediate) = 512.  First row, last of pass one,
    first of pass two and last row equal the one-row call bit for bit; decode reads the encode's output."""
    o, g = contexts(1 << 15, "50-40")
    _second_pass(capi, o, g, 1 << 15, 1025, 1024, 513, 512)


def test_second_pass_grid_limit(contexts, capi):
    """N = 2^10, nl = 1.  Encode: 65537 rows, past kMaxGridY = 65535 rows a pass (512 MiB of output).  Decode: 32769 rows, one past
    kScratchCap (256 MiB) / 8 KiB of coefficients = 32768."""
    o, g = contexts(1 << 10, "50-40")
    _second_pass(capi, o, g, 1 << 10, 65537, 65535, 32769, 32768)


# ---- G. decode against the exact lift ----
LIFTS = [("60x16", 4), ("60x16", 5), ("60x16", 8), ("60x16", 9), ("60x16", 15), ("60-30", 4)]
SCALE = 2.0 ** 40


def _lift_values(Q):
    w = (Q.bit_length() + 63) // 64  # words of Q; its top word is non-zero, so 2^(64 (w - 1)) < Q
    top = 1 << (64 * (w - 1))
    vals = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2, 2 ** 64 - 1, 2 ** 64, Q - 2 ** 64, top, Q - top]
    assert all(0 <= v < Q for v in vals)
    return list(dict.fromkeys(vals))


@pytest.mark.parametrize("half", [False, True], ids=["coef0", "coefN/2"])
@pytest.mark.parametrize("name,nl", LIFTS)
def test_decode_lift_at_its_decision_points(contexts, name, nl, half):
    """V as a constant polynomial (every slot V' / scale) and as V X^(N/2) (slot i: +-i V' / scale, + for even i), V' the
    representative of V in (-Q/2, Q/2]: both sides of the sign decision at Q/2, borrow chains through every word (Q - 1, Q - 2^64),
    a top word that decides (four, eight and fifteen 60-bit primes fill the top word of the 4-, 8- and 16-word lift; nl = 5 and 9
    are the first levels of the next one) and, on 60-30, 60-bit Garner digits times 30-bit moduli.  1e-12 relative, as
    test_gpu_ckks_codec.py's constant test argues."""
    n = 1 << 14
    o, g = contexts(n, name)
    Q = 1
    for q in o.primes[:nl]:
        Q *= q
    sign = np.where(np.arange(n // 2) % 2 == 0, 1.0, -1.0)
    for V in _lift_values(Q):
        poly = np.zeros(n, dtype=np.uint64)
        plain = []
        for j in range(nl):
            poly[n // 2 if half else 0] = V % o.primes[j]
            plain.append(o.ntt(j, poly))
        got = g.ckks_decode(np.stack(plain), SCALE)
        want = float(V - Q if V > Q // 2 else V) / SCALE
        main, other = (got.imag * sign, got.real) if half else (got.real, got.imag)
        what = "%s nl=%d V=%#x" % (name, nl, V)
        assert np.abs(main - want).max() <= 1e-12 * abs(want), "%s: %g off (relative)" % (what, np.abs(main - want).max() / abs(want))
        assert np.abs(other).max() <= 1e-12 * abs(want), "%s: the other part is %g (relative)" % (what, np.abs(other).max() / abs(want))


@pytest.mark.parametrize("name,nl", LIFTS)
def test_decode_random_residues_exact(contexts, name, nl):
    n = 1 << 14
    o, g = contexts(n, name)
    rng = np.random.default_rng(nl)
    rnd = np.stack([rng.integers(0, o.primes[j], n, dtype=np.uint64) for j in range(nl)])
    want = spec.decode_exact(_coeff_form(o, rnd), SCALE, n, o.primes)
    got = g.ckks_decode(rnd, SCALE)
    err = float(np.abs(got.astype(np.clongdouble) - want).max() / np.abs(want).max())
    print("%s nl=%d: random residues decode %.3g off, relative to the largest slot (tolerance %.3g)" % (name, nl, err, spec.decode_tol(14)))
    assert err <= spec.decode_tol(14)


# ---- H. round trip ----
@pytest.mark.parametrize("logn", spec.RINGS)
def test_round_trip_within_both_tolerances(contexts, logn):
    """decode(encode(v)) - v is at most the sum over the N coefficients of what each may be off -- half a unit of rounding plus the
    encode margin -- divided by the scale, plus the decode tolerance"""
    n = 1 << logn
    o, g = contexts(n, "50-40")
    v = spec.encode_case_values(logn, True, False)
    got = g.ckks_decode(g.ckks_encode(v, SCALE, o.L), SCALE)
    bound = n * (0.5 + spec.encode_margin(logn, 40)) / SCALE + spec.decode_tol(logn) * np.abs(v).max()
    err = float(np.abs(got - v).max())
    print("N=2^%d: round trip %.3g (bound %.3g)" % (logn, err, bound))
    assert err <= bound
