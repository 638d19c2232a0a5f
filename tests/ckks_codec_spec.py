"""The CKKS slot codec restated exactly enough to be a yardstick for abc_hip_ckks_encode / abc_hip_ckks_decode.

The device's transform is fp64 with long-double tables; the CPU oracle's orc_ckks_encode is fp64 with fp64 twiddles, so it cannot
decide a rounding the device got right.  This module is independent of both and of abc_amd/ckks_encoder.py: an N-point numpy
transform in long double (64-bit mantissa, numpy transforms clongdouble natively) with the twist exp(-i pi k / N) built in long
double, Python integers for everything that is an integer.  tests/test_ckks_codec_spec.py checks it against a 50-digit mpmath
evaluation of the definition and measures what fp64 loses against it; that measured loss (FP64_ERR), not anything the device
returns, is where the GPU tests' margins come from.

The definition (include/abc_hip.h, abc_hip_ckks_encode): slot i is m(zeta^(3^i)), zeta = exp(i pi / N), m real, so
m(zeta^(-3^i)) is its conjugate; slots beyond the given values are zero.  With g = 3^i mod 2N the point zeta^g sits at position
j = (g - 1) / 2 of the odd powers zeta^(2j+1), and
    m_k = (1/N) sum_j w_j zeta^(-(2j+1) k) = zeta^(-k) / N * sum_j w_j exp(-2 pi i j k / N)       (inverse embedding)
    w_j = sum_k (m_k zeta^k) exp(+2 pi i j k / N)                                                 (forward)
Rounding: to the nearest integer, ties away from zero.
"""
import numpy as np

LD = np.longdouble
_PI = LD("3.14159265358979323846264338327950288419716939937510")


def _real_type(dtype):
    return LD if np.dtype(dtype) == np.dtype(np.clongdouble) else np.float64


def slot_positions(n):
    """position j of slot i's evaluation point zeta^(2j+1) = zeta^(3^i), and of its conjugate's"""
    g, pos, conj = 1, [], []
    for _ in range(n // 2):
        pos.append((g - 1) >> 1)
        conj.append((2 * n - g - 1) >> 1)
        g = g * 3 % (2 * n)
    return np.array(pos), np.array(conj)


def _twist(n, dtype, sign):
    """exp(sign * i pi k / N), k < N, in the precision of dtype (the angle k / N is exact in either)"""
    rt = _real_type(dtype)
    a = np.arange(n).astype(rt) * (rt(_PI) / rt(n))
    return (np.cos(a) + sign * 1j * np.sin(a)).astype(dtype)


def encode_unrounded(values, scale, n, dtype=np.clongdouble):
    """the N real coefficients of the encoding of `values` (<= N/2 real or complex slots) at `scale`, before rounding; with
    dtype=np.complex128 the same arithmetic in fp64"""
    rt = _real_type(dtype)
    v = np.asarray(values).astype(dtype).reshape(-1)
    assert len(v) <= n // 2
    pos, conj = slot_positions(n)
    w = np.zeros(n, dtype)
    w[pos[:len(v)]] = v
    w[conj[:len(v)]] = np.conj(v)
    u = np.fft.fft(w)
    assert u.dtype == np.dtype(dtype)
    return (u * _twist(n, dtype, -1)).real * (rt(scale) / rt(n))


def round_away(x):
    """nearest integer, ties away from zero, of a long-double array, as Python integers; |x - round| exactly"""
    x = np.asarray(x, LD)
    t = np.trunc(x)
    r = t + np.sign(x) * (np.abs(x - t) >= LD(0.5))  # x - t is exact
    return np.array([int(y) for y in r], dtype=object)


def encode_exact(values, scale, n, primes):
    """(coefficients as Python integers [N], residues uint64 [len(primes)][N] in coefficient form, distance of every unrounded
    coefficient to the nearest half-integer as float64 [N])"""
    c = encode_unrounded(values, scale, n)
    r = round_away(c)
    frac = np.abs(c - np.trunc(c))
    res = np.array([[int(x) % int(q) for x in r] for q in primes], dtype=np.uint64).reshape(len(primes), n)
    return r, res, np.abs(frac - LD(0.5)).astype(np.float64)


def crt_centred(residues, primes):
    """Python-integer CRT of residues [nl][N] (any integer dtype) into the representatives in (-Q/2, Q/2]; returns (object [N], Q)"""
    qs = [int(q) for q in primes[:len(residues)]]
    Q = 1
    for q in qs:
        Q *= q
    acc = np.zeros(len(residues[0]), dtype=object)
    for j, q in enumerate(qs):
        Qj = Q // q
        acc = acc + np.array([int(x) for x in residues[j]], dtype=object) * (Qj * pow(Qj % q, -1, q))
    acc = acc % Q
    return np.array([x - Q if x > Q // 2 else x for x in acc], dtype=object), Q


def to_longdouble(ints):
    """Python integers -> long double, correctly rounded to 64 bits for any size (two exact pieces, one rounding in the sum)"""
    out = np.empty(len(ints), LD)
    for i, x in enumerate(ints):
        x = int(x)
        s, a = (-1, -x) if x < 0 else (1, x)
        sh = max(0, a.bit_length() - 64)
        top = a >> sh  # < 2^64: exact in long double
        if sh and (a >> (sh - 1)) & 1:  # round to nearest on the dropped bits (ties up: half an ulp of 64 bits, below any tolerance here)
            top += 1
        out[i] = s * np.ldexp(LD(top >> 32) * LD(4294967296.0) + LD(top & 0xFFFFFFFF), sh)
    return out


def slots_of_polynomial(m, n, dtype=np.clongdouble):
    """the N/2 slots of the integer polynomial m (Python integers or anything to_longdouble takes), unscaled"""
    rt = _real_type(dtype)
    c = to_longdouble(m).astype(rt).astype(dtype)
    assert len(c) == n
    w = np.fft.ifft(c * _twist(n, dtype, +1)) * rt(n)
    assert w.dtype == np.dtype(dtype)
    pos, _ = slot_positions(n)
    return w[pos]


def decode_exact(residues_coeff_form, scale, n, primes, dtype=np.clongdouble):
    """residues [nl][N] in coefficient form -> the N/2 slot values / scale (clongdouble)"""
    ints, _ = crt_centred(residues_coeff_form, primes)
    return slots_of_polynomial(ints, n, dtype) / _real_type(dtype)(scale)


# ---- what fp64 loses against long double, measured between the two precisions of THIS module (test_ckks_codec_spec.py
# recomputes every entry and holds it within [recomputed, 4 x recomputed]).  The GPU tests take 8 x the entry as their margin
# (encode: distance to a tie below which a coefficient may land on either side, in units) and tolerance (decode: relative to
# max |want|): three bits for the device's other summation order and FMA contraction.
# key (log2 N, log2 scale) -> (encode error in units of one coefficient, decode error relative to the largest slot)
# Inputs: encode -- fp64_inputs(seed, n): complex slots uniform in the unit square; decode -- random residues on the whole of
# (-Q/2, Q/2], where the relative error does not depend on Q.
FP64_ERR = {
    (10, 20): (4.9e-11, 5.7e-16), (10, 40): (5.1e-05, 5.7e-16), (10, 58): (1.4e+01, 5.7e-16),
    (11, 20): (3.0e-11, 6.0e-16), (11, 40): (3.1e-05, 6.0e-16), (11, 58): (8.1e+00, 6.0e-16),
    (12, 20): (2.9e-11, 7.4e-16), (12, 40): (3.0e-05, 7.4e-16), (12, 58): (7.9e+00, 7.4e-16),
    (14, 20): (1.7e-11, 7.8e-16), (14, 40): (1.7e-05, 7.8e-16), (14, 58): (4.5e+00, 7.8e-16),
    (15, 20): (1.3e-11, 7.3e-16), (15, 40): (1.4e-05, 7.3e-16), (15, 58): (3.6e+00, 7.3e-16),
    (16, 20): (1.1e-11, 8.6e-16), (16, 40): (1.1e-05, 8.6e-16), (16, 58): (2.9e+00, 8.6e-16),
}
MEASURE_SEEDS = (0, 1, 2)  # the recorded figures: twice the largest of these three draws, rounded up to two digits


def encode_margin(logn, log_scale):
    return 8 * FP64_ERR[(logn, log_scale)][0]


def decode_tol(logn, log_scale=40):
    return 8 * FP64_ERR[(logn, log_scale)][1]


def fp64_inputs(seed, n, count=None, cplx=True):
    rng = np.random.default_rng(seed)
    count = n // 2 if count is None else count
    v = rng.uniform(-1, 1, count)
    return v + 1j * rng.uniform(-1, 1, count) if cplx else v


def measure_encode_err(logn, log_scale, seed=None):
    if seed is None:
        return max(measure_encode_err(logn, log_scale, s) for s in MEASURE_SEEDS)
    n = 1 << logn
    v = fp64_inputs(seed, n)
    hi = encode_unrounded(v, 2.0 ** log_scale, n)
    lo = encode_unrounded(v, 2.0 ** log_scale, n, np.complex128)
    return float(np.abs(hi - lo.astype(LD)).max())


def measure_decode_err(logn, seed=None):
    """fp64 against long double on integer coefficients uniform in 200 bits, relative to the largest slot (scale-free)"""
    if seed is None:
        return max(measure_decode_err(logn, s) for s in MEASURE_SEEDS)
    n = 1 << logn
    rng = np.random.default_rng(seed)
    m = [int(rng.integers(0, 1 << 62)) * (1 << 138) + int(rng.integers(0, 1 << 62)) - (1 << 199) for _ in range(n)]
    hi = slots_of_polynomial(m, n)
    lo = slots_of_polynomial(m, n, np.complex128)
    return float(np.abs(hi - lo.astype(np.clongdouble)).max() / np.abs(hi).max())


# ---- the inputs of the GPU file's word-for-word encode cases, fixed here so that the CPU tests can hold the reference alone to
# what those cases assume about it (test_ckks_codec_spec.py: no coefficient within the margin of a tie at scale 2^20, at most
# 0.1 % of them at scale 2^40)
RINGS = (10, 11, 12, 14, 15, 16)
SHORT = 37  # the short row has N/2 - 37 values


# seeds drawn on the CPU against the reference alone: the first of 7000 + ..., 8000 + ... that meets both conditions above
_REDRAWN = {(10, False, False): 8100, (10, False, True): 8101}  # N = 2^10, real slots: two of 1024 coefficients are 0.2 %


def encode_case_values(logn, cplx, short):
    n = 1 << logn
    seed = _REDRAWN.get((logn, bool(cplx), bool(short)), 7000 + 10 * logn + 2 * int(cplx) + int(short))
    return fp64_inputs(seed, n, n // 2 - (SHORT if short else 0), cplx)


_case_cache = {}


def encode_case_reference(logn, cplx, short, log_scale):
    """(values, integer coefficients, distance of each to a tie) of one case; computed once per process"""
    key = (logn, cplx, short, log_scale)
    if key not in _case_cache:
        v = encode_case_values(logn, cplx, short)
        r, _, dist = encode_exact(v, 2.0 ** log_scale, 1 << logn, [])
        r.setflags(write=False)
        dist.setflags(write=False)
        _case_cache[key] = (v, r, dist)
    return _case_cache[key]
