"""tests/ckks_codec_spec.py earns its place as the codec's yardstick: it inverts itself on integer polynomials, agrees with a
50-digit evaluation of the definition, brackets the CPU oracle's fp64 encoder within one unit, and the fp64 errors it records
(FP64_ERR, the source of every margin in tests/test_gpu_ckks_codec_exact.py) are the ones it measures.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckks_codec_spec as spec  # noqa: E402

LD = np.longdouble


@pytest.mark.parametrize("logn", spec.RINGS)
def test_round_trip_on_integer_polynomials(logn):
    """|m_k| < 2^24: with a 64-bit mantissa, 2^-30 of a unit leaves 2^34 for the magnitude and the growth sqrt(N) log N <= 2^12 of an
    N <= 2^16 point transform, there and back."""
    n = 1 << logn
    rng = np.random.default_rng(logn)
    m = [int(x) for x in rng.integers(-(1 << 24), 1 << 24, n)]
    back = spec.encode_unrounded(spec.slots_of_polynomial(m, n), 1.0, n)
    err = float(np.abs(back - spec.to_longdouble(m)).max())
    print("N=2^%d: round trip %.3g of a unit" % (logn, err))
    assert err <= 2.0 ** -30


def test_to_longdouble_is_exact_where_it_can_be():
    for x in (0, 1, -1, 2 ** 63 - 1, 2 ** 64 - 1, -(2 ** 64 - 1), 2 ** 64, 2 ** 200, -(2 ** 900) - 2 ** 840):
        assert int(spec.to_longdouble([x])[0]) == x
    assert int(spec.to_longdouble([2 ** 65 + 1])[0]) == 2 ** 65  # 66 bits: rounds to the nearest multiple of 4
    assert int(spec.to_longdouble([2 ** 65 + 3])[0]) == 2 ** 65 + 4


def test_round_away():
    x = np.array([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.0 ** 40 + 0.5, 0.0, -3.0], LD)
    assert list(spec.round_away(x)) == [1, -1, 2, 3, -3, 0, 0, 2 ** 40 + 1, 0, -3]


def _mpf(mp, x):
    """a long double as the same number in mpmath"""
    m, e = np.frexp(LD(x))
    return mp.mpf(int(m * LD(2.0 ** 64))) * mp.mpf(2) ** (int(e) - 64)


def test_against_mpmath():
    """the definition itself at 50 digits: m_k = (1/N) sum over all N evaluation points (slot and conjugate) of the value times the
    point to the power -k; and the slots of a polynomial by Horner-free direct summation"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    n, scale = 256, 2.0 ** 40
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, n // 2 - 3) + 1j * rng.uniform(-1, 1, n // 2 - 3)
    got = spec.encode_unrounded(v, scale, n)
    pts, vals, g = [], [], 1
    for i in range(n // 2):
        z = mp.mpc(v[i].real, v[i].imag) if i < len(v) else mp.mpc(0)
        pts += [g, 2 * n - g]
        vals += [z, mp.conj(z)]
        g = g * 3 % (2 * n)
    root = [mp.expjpi(mp.mpf(e) / n) for e in range(2 * n)]  # zeta^e
    worst = 0.0
    for k in range(n):
        c = sum(val * root[(-p * k) % (2 * n)] for p, val in zip(pts, vals)) / n * mp.mpf(scale)
        assert abs(c.imag) < mp.mpf(10) ** -30
        ref = c.real
        # relative to the coefficient, or to scale / N (1/16 of a typical one) where it happens to be smaller than that
        worst = max(worst, float(abs(_mpf(mp, got[k]) - ref) / max(abs(ref), mp.mpf(scale) / n)))
    print("encode against mpmath: %.3g relative" % worst)
    assert worst <= 1e-15
    # decode direction on a random integer polynomial
    m = [int(x) for x in rng.integers(-(1 << 50), 1 << 50, n)]
    slots = spec.slots_of_polynomial(m, n)
    g, worst, refs = 1, 0.0, []
    for i in range(n // 2):
        refs.append(sum(m[k] * root[(g * k) % (2 * n)] for k in range(n)))
        g = g * 3 % (2 * n)
    big = max(abs(r) for r in refs)
    for i, r in enumerate(refs):
        d = mp.mpc(_mpf(mp, slots[i].real), _mpf(mp, slots[i].imag)) - r
        worst = max(worst, float(abs(d) / big))
    print("slots against mpmath: %.3g relative to the largest" % worst)
    assert worst <= 1e-15


@pytest.mark.parametrize("logn", (10, 12, 14))
def test_oracle_encoder_is_within_one_unit(oracle_mod, logn):
    n = 1 << logn
    primes = oracle_mod.create_primes(n, [50, 40, 40, 50])
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    for log_scale in (20, 40):
        v, want, dist = spec.encode_case_reference(logn, True, False, log_scale)
        enc = o.ckks_encode(v, 2.0 ** log_scale, 3)
        got, Q = spec.crt_centred([o.intt(j, enc[j]) for j in range(3)], primes)
        diff = np.array([abs(int(a) - int(b)) for a, b in zip(got, want)])
        print("N=2^%d scale 2^%d: the oracle differs in %d of %d coefficients (%.4f %%)" % (
            logn, log_scale, int((diff != 0).sum()), n, 100.0 * (diff != 0).mean()))
        assert diff.max() <= 1
        # and only where the reference itself is near a tie
        assert dist[diff != 0].max(initial=0.0) <= spec.encode_margin(logn, log_scale)


@pytest.mark.parametrize("logn", spec.RINGS)
def test_recorded_fp64_errors(logn):
    """FP64_ERR is measured between the two precisions of the spec and never from the device: recorded >= recomputed, <= 4 x"""
    dec = spec.measure_decode_err(logn)
    for log_scale in (20, 40, 58):
        enc = spec.measure_encode_err(logn, log_scale)
        rec_enc, rec_dec = spec.FP64_ERR[(logn, log_scale)]
        print("N=2^%d scale 2^%d: encode %.3g units (recorded %.3g), decode %.3g relative (recorded %.3g)" % (
            logn, log_scale, enc, rec_enc, dec, rec_dec))
        assert enc <= rec_enc <= 4 * enc
        assert dec <= rec_dec <= 4 * dec


@pytest.mark.parametrize("logn", spec.RINGS)
def test_gpu_encode_cases_are_decidable(logn):
    """what test_gpu_ckks_codec_exact.py's word-for-word cases assume of the reference alone: at scale 2^20 no coefficient within
    the margin of a tie, at scale 2^40 at most 0.1 % of them"""
    n = 1 << logn
    for cplx in (False, True):
        for short in (False, True):
            _, _, dist = spec.encode_case_reference(logn, cplx, short, 20)
            assert dist.min() > spec.encode_margin(logn, 20), "seed of N=2^%d complex=%s short=%s needs another draw" % (logn, cplx, short)
            _, _, dist = spec.encode_case_reference(logn, cplx, short, 40)
            share = float((dist <= spec.encode_margin(logn, 40)).mean())
            print("N=2^%d complex=%s short=%s scale 2^40: %.4f %% within the margin of a tie" % (logn, cplx, short, 100 * share))
            assert share <= 1e-3
