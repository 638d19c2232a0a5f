"""abc_hip_ckks_poly_eval's fixed sequence as tests/poly_eval_spec.py restates it on the CPU oracle: N = 1024, a seven-limb chain
{50,30,30,30,30,30,30 | 50}, slots in [-1, 1], x and the result at scale 2^30.  Thirty-bit rescaling primes because the constant term
enters the last sum at out_scale * q_{m-1}, and const_words holds |c_0| out_scale q_{m-1} below 2^62: 2^60 |c_0| here.

The yardstick of the error is the sequence a caller composes today (poly_eval_composed: encoded constant vectors, one rescale per
product, mod_switch, add): the spec's max |error| against numpy's polynomial may be at most twice that sequence's, and stays
below the project's 1e-4.

Measured with this file's seeds (max |error| of the decoded slots, spec / composed):
  degree 1: 9.43e-07 / 9.44e-07    degree 2: 1.85e-06 / 2.11e-06    degree 3: 1.75e-06 / 2.00e-06
  degree 5: 1.50e-06 / 2.38e-06    degree 7: 2.22e-06 / 2.37e-06
and every word of the two results differs from degree 2 on (at degree 1 there is one term and one rescale either way: component 1
is the same, component 0 takes its constant before the rescale instead of behind it)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import const_sum_spec as cs  # noqa: E402
import poly_eval_spec as spec  # noqa: E402

N, BITS, SCALE = 1024, [50, 30, 30, 30, 30, 30, 30, 50], 2.0 ** 30
BOUND = 1e-4  # the project's bound at this scale (tests/test_plain_sum_spec.py)
DEGREES = [1, 2, 3, 5, 7]


@pytest.fixture(scope="module")
def rig(oracle_mod):
    om = oracle_mod
    o = om.Oracle(om.CKKS, N, om.create_primes(N, BITS))
    o.keygen(0x901E)
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, N // 2)
    coeffs = rng.uniform(-1, 1, 8)
    ct = o.encrypt(o.ckks_encode(x, SCALE), 5)
    return dict(o=o, x=x, ct=ct, coeffs=coeffs)


def _error(o, ct, clear):
    return np.abs(o.ckks_decode(o.decrypt(ct), SCALE) - clear).max()


def test_depth_and_plan(rig):
    assert [spec.depth(d) for d in (1, 2, 3, 4, 5, 7, 8, 9, 31)] == [1, 2, 3, 3, 4, 4, 4, 5, 6]
    o = rig["o"]
    p = spec.plan(o.primes, 7, SCALE, [1.0] * 8, SCALE)
    assert p["level"][1:] == [7, 6, 5, 5, 4, 4, 4] and p["m"] == 4
    assert [(p["hi"][k], p["lo"][k]) for k in range(2, 8)] == [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3)]
    assert p["scale"][2] == SCALE * SCALE / o.primes[6] and p["scale"][3] == p["scale"][2] * SCALE / o.primes[5]
    # a zero middle coefficient: x^5 and x^6 are neither terms nor factors, x^3 is a factor of x^7 still
    z = spec.plan(o.primes, 7, SCALE, [1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0], SCALE)
    assert z["terms"] == [1, 4, 7] and z["need"][1:] == [True, True, True, True, False, False, True]


@pytest.mark.parametrize("degree", DEGREES)
def test_the_spec_decodes_to_numpys_polynomial_no_worse_than_the_composed_sequence(rig, degree):
    o, ct = rig["o"], rig["ct"]
    coeffs = list(rig["coeffs"][: degree + 1])
    clear = np.polynomial.polynomial.polyval(rig["x"], coeffs)
    got = spec.poly_eval(o, ct, SCALE, coeffs, SCALE)
    composed = spec.poly_eval_composed(o, ct, SCALE, coeffs, SCALE)
    assert got.shape == composed.shape == (2, o.L - spec.depth(degree), N)
    e_spec, e_comp = _error(o, got, clear), _error(o, composed, clear)
    frac = (got != composed).mean()
    print("degree %d: max |error| spec %.3g, composed %.3g; words that differ: %.2f %%" % (degree, e_spec, e_comp, 100 * frac))
    assert e_spec <= 2 * e_comp
    assert e_spec < BOUND and e_comp < BOUND
    if degree >= 2:  # a rescale per term is another ciphertext in every word: forwarding to K multiply_plain_rescale calls cannot pass
        assert (got != composed).all()


def test_a_zero_coefficient_and_a_skipped_power_change_no_word(rig):
    o, ct = rig["o"], rig["ct"]
    coeffs = [0.25, -0.5, 0.0, 0.75, 0.0, 0.0]  # degree 5 on paper: x^5 and x^4 are never formed
    p = spec.plan(o.primes, o.L, SCALE, coeffs, SCALE)
    assert p["terms"] == [1, 3] and not p["need"][4] and not p["need"][5]
    got = spec.poly_eval(o, ct, SCALE, coeffs, SCALE)
    # every power formed and every term kept, zero weights included: the same words
    full = dict(p, need=[False] + [True] * 5, terms=[1, 2, 3, 4, 5],
                weights=[cs.const_words(o.primes, coeffs[k], SCALE * o.primes[p["m"] - 1] / p["scale"][k], p["m"]) for k in range(1, 6)])
    pw = spec.powers(o, ct, full)
    want = cs.multiply_const_sum_rescale(o, [pw[k] for k in full["terms"]], full["weights"], const=p["w0"], nl=p["m"])
    assert np.array_equal(got, want)
    clear = np.polynomial.polynomial.polyval(rig["x"], coeffs)
    assert _error(o, got, clear) < BOUND


def test_library_exports_the_entry_points(capi):
    lib = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "abc_hip.h")).read()
    assert hasattr(lib, "abc_hip_ckks_poly_eval") and hasattr(lib, "abc_hip_ckks_poly_eval_depth")
    assert re.search(r"\bint abc_hip_ckks_poly_eval\(abc_hip_ctx \*ctx", header) and re.search(r"\bint abc_hip_ckks_poly_eval_depth\(int degree\)", header)
    assert "abc_hip_ckks_poly_eval" in capi.SYMBOLS and "abc_hip_ckks_poly_eval_depth" in capi.SYMBOLS
    assert callable(capi.Context.poly_eval) and callable(capi.Context.poly_eval_depth)
    assert [capi.Context.poly_eval_depth(d) for d in (1, 2, 3, 4, 5, 8, 9, 31)] == [spec.depth(d) for d in (1, 2, 3, 4, 5, 8, 9, 31)]
    with pytest.raises(capi.AbcHipError, match="degree"):
        capi.Context.poly_eval_depth(0)
    m = re.search(r"#define ABC_HIP_ROUTE_POLY_EVAL (\d+)", header)
    assert m and int(m.group(1)) == 19 == capi.Context.ROUTE_OPS["poly_eval"]
