"""Scalar constants as per-limb words, and the scalar-weighted sum that reads each term at its own level, as
tests/const_sum_spec.py states them, on the CPU (N = 1024, {50,40,40,40,50}, scale 2^40).

In NTT form the constant c is the plaintext whose every word of limb j is const_words(c)[j]: for a dyadic c * scale that is the
oracle's encoding of N/2 copies of c in every word; for another constant the encoder's fp64 transform may round coefficient 0 one
unit away, and no other coefficient is anything but zero."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import const_sum_spec as spec  # noqa: E402

N, BITS, SCALE = 1024, [50, 40, 40, 40, 50], 2.0 ** 40
NAMES = ("abc_hip_ckks_const_words", "abc_hip_multiply_const_sum", "abc_hip_multiply_const_sum_rescale")


@pytest.fixture(scope="module")
def rig(oracle_mod):
    om = oracle_mod
    o = om.Oracle(om.CKKS, N, om.create_primes(N, BITS))
    o.keygen(0xC057)
    rng = np.random.default_rng(17)
    xs = rng.uniform(-1, 1, (3, N // 2))
    cts = [o.encrypt(o.ckks_encode(v, SCALE), 200 + k) for k, v in enumerate(xs)]
    return dict(o=o, xs=xs, cts=cts)


def _coefficients(o, plain):
    """[nl][N] NTT form -> coefficient form"""
    return np.stack([o.intt(j, plain[j]) for j in range(plain.shape[0])])


@pytest.mark.parametrize("value", [0.5, -1.25, 3.0, 0.0])
def test_dyadic_constants_are_the_encoded_constant_vector_in_every_word(rig, value):
    o = rig["o"]
    for nl in (o.L, 2, 1):
        words = spec.const_words(o.primes, value, SCALE, nl)
        enc = o.ckks_encode(np.full(N // 2, value), SCALE, nl)
        assert np.array_equal(enc, spec.const_plain(words, N)), (value, nl)
        r = int(value * SCALE)
        assert [int(w) for w in words] == [r % q for q in o.primes[:nl]]


def test_equal_dyadic_values_sum_exactly(rig):
    o = rig["o"]
    a, b, c = (spec.const_words(o.primes, v, SCALE, o.L) for v in (0.5, -1.25, -0.75))
    assert [(int(x) + int(y)) % q for x, y, q in zip(a, b, o.primes)] == [int(z) for z in c]
    neg = spec.const_words(o.primes, 1.25, SCALE, o.L)
    assert all((int(x) + int(y)) % q == 0 for x, y, q in zip(b, neg, o.primes))  # subtraction is const_words(-c)


@pytest.mark.parametrize("value", [0.1, -1.0 / 3, 0.7853981633974483, 1e-7])
def test_a_non_dyadic_constant_is_within_one_unit_in_coefficient_0_and_equal_elsewhere(rig, value):
    o = rig["o"]
    words = spec.const_words(o.primes, value, SCALE, o.L)
    coef = _coefficients(o, o.ckks_encode(np.full(N // 2, value), SCALE))
    assert not coef[:, 1:].any()
    signed = []
    for j, q in enumerate(o.primes[: o.L]):
        diff = (int(coef[j, 0]) - int(words[j])) % q
        assert diff in (0, 1, q - 1), (value, j, diff)
        signed.append(-1 if diff == q - 1 else diff)
    assert len(set(signed)) == 1  # one and the same integer in every limb


def test_rounding_sign_and_limits():
    primes = [1125899906826241, 1099511590913]
    assert [int(w) for w in spec.const_words(primes, 2.5, 1.0, 2)] == [3, 3]  # ties away from zero
    assert [int(w) for w in spec.const_words(primes, -2.5, 1.0, 2)] == [q - 3 for q in primes]
    assert [int(w) for w in spec.const_words(primes, -0.4, 1.0, 2)] == [0, 0]  # -0 stays 0, not q
    big = spec.const_words(primes, 1.0, 2.0 ** 61, 2)
    assert [int(w) for w in big] == [2 ** 61 % q for q in primes]
    for bad in (2.0 ** 62, -2.0 ** 62, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            spec.const_words(primes, 1.0, bad, 2)


def test_the_sum_is_multiply_plain_add_and_add_plain_word_for_word_with_raised_terms(rig):
    o, cts = rig["o"], rig["cts"]
    nl = o.L - 2
    terms = [cts[0], o.mod_switch(cts[1]), o.mod_switch(o.mod_switch(cts[2]))]  # two, one and no level above nl
    assert [t.shape[1] for t in terms] == [nl + 2, nl + 1, nl]
    wscale = 2.0 ** 20  # the sum lands at 2^60: a constant there is within const_words' 2^62
    weights = [spec.const_words(o.primes, v, wscale, nl) for v in (0.5, -0.3, 2.0)]
    const = spec.const_words(o.primes, -1.7, SCALE * wscale, nl)
    addend = o.multiply_plain(terms[2], spec.const_plain(weights[0], N))
    want = None
    for t, w in zip(terms, weights):  # written out: orc_ckks_multiply_plain per term, orc_add, orc_ckks_add_plain
        low = t
        while low.shape[1] > nl:
            low = o.mod_switch(low)
        prod = o.multiply_plain(low, spec.const_plain(w, N))
        want = prod if want is None else o.add(want, prod)
    with_const = o.add_plain(want, spec.const_plain(const, N))
    assert np.array_equal(spec.multiply_const_sum(o, terms, weights), want)
    assert np.array_equal(spec.multiply_const_sum_words(o.primes, terms, weights), want)
    assert np.array_equal(spec.multiply_const_sum(o, terms, weights, const=const), with_const)
    assert np.array_equal(spec.multiply_const_sum_words(o.primes, terms, weights, const=const), with_const)
    assert np.array_equal(with_const[1], want[1]) and not np.array_equal(with_const[0], want[0])  # component 0 only
    assert np.array_equal(spec.multiply_const_sum_words(o.primes, terms, weights, const=const, addend=addend), o.add(addend, with_const))
    assert np.array_equal(spec.multiply_const_sum(o, terms, weights, const=const, addend=addend), o.add(addend, with_const))
    # and the values: 0.5 x0 - 0.3 x1 + 2 x2 - 1.7 at scale * wscale
    clear = 0.5 * rig["xs"][0] - 0.3 * rig["xs"][1] + 2.0 * rig["xs"][2] - 1.7
    got = o.ckks_decode(o.decrypt(with_const), SCALE * wscale)
    assert np.abs(got - clear).max() < 1e-4


def test_spec_edges(rig):
    o, ct = rig["o"], rig["cts"][0]
    const = spec.const_words(o.primes, 0.25, SCALE, 3)
    only = spec.multiply_const_sum(o, [], [], const=const, size=2, nl=3)
    assert only.shape == (2, 3, N) and not only[1].any() and np.array_equal(only[0], spec.const_plain(const, N))
    assert np.array_equal(spec.multiply_const_sum(o, [], [], addend=ct), ct)
    w = [spec.const_words(o.primes, 0.5, SCALE, o.L)]
    assert np.array_equal(spec.multiply_const_sum_rescale(o, [ct], w), o.rescale(o.multiply_plain(ct, spec.const_plain(w[0], N))))
    two = spec.multiply_const_sum_rescale(o, [ct, rig["cts"][1]], w * 2)
    assert (two != spec.per_term_rescaled_sum(o, [ct, rig["cts"][1]], w * 2)).mean() > 0.1  # one rounding instead of two: other words


def test_library_exports_the_entry_points(capi):
    lib = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "abc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
        assert re.search(r"\bint %s\(abc_hip_ctx \*ctx" % name, header), name
        assert name in capi.SYMBOLS
    for method in ("const_words", "multiply_const_sum", "multiply_const_sum_rescale", "multiply_const", "add_const"):
        assert callable(getattr(capi.Context, method))
    m = re.search(r"#define ABC_HIP_ROUTE_CONST_SUM_RESCALE (\d+)", header)
    assert m and int(m.group(1)) == 18 == capi.Context.ROUTE_OPS["const_sum_rescale"]
    assert "kRouteConstSumRescale = 18, kRoutePolyEval = 19" in open(os.path.join(root, "abc_amd", "csrc", "abc_route.hpp")).read()
