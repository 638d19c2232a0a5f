"""The spec of the sum-of-products calls (tests/mul_sum_spec.py) against the eager form, on the CPU oracle alone: a sum that is
relinearised once differs from the sum of K relinearised products in nearly every word, so a GPU implementation that relinearises
per term cannot pass the parity tests of tests/test_gpu_mul_sum.py.  Also: the Python binding names both entry points and the route."""
import numpy as np
import pytest

import mul_sum_spec as spec

N, K = 1024, 3


def _random_cts(rng, primes, nl, how_many):
    return [np.stack([rng.integers(0, q, size=(2, N), dtype=np.uint64) for q in primes[:nl]], axis=1) for _ in range(how_many)]


@pytest.mark.parametrize("bits", [[50, 40, 40, 50], [60, 40, 40, 60]], ids=["fp", "wide"])
def test_one_relinearisation_is_not_k_relinearisations(oracle_mod, bits):
    om = oracle_mod
    o = om.Oracle(om.CKKS, N, om.create_primes(N, bits))
    o.keygen(21)
    nl = o.L
    rng = np.random.default_rng(sum(bits))
    as_, bs = _random_cts(rng, o.primes, nl, K), _random_cts(rng, o.primes, nl, K)
    lazy = spec.mul_sum_relin(o, as_, bs)
    eager = spec.per_term_relin(o, as_, bs)
    assert lazy.shape == eager.shape == (2, nl, N)
    for comp in range(2):
        for j in range(nl):
            differ = float(np.mean(lazy[comp, j] != eager[comp, j]))
            print("chain %s component %d limb %d: %.2f %% of the words differ" % (bits, comp, j, 100 * differ))
            assert differ >= 0.99
    # and the two agree on what they are made of: the size-3 sum is the sum of the size-3 products, in any order
    s3 = spec.multiply_sum(o, as_, bs)
    assert np.array_equal(s3, spec.multiply_sum(o, as_[::-1], bs[::-1]))
    assert np.array_equal(spec.mul_sum_relin(o, as_[:1], bs[:1]), o.mul_relin(as_[0], bs[0]))
    assert not spec.multiply_sum(o, [], [], nl).any() and not spec.mul_sum_relin(o, [], [], nl).any()


def test_binding_names_the_calls(capi):
    assert "abc_hip_multiply_sum" in capi.SYMBOLS and "abc_hip_mul_sum_relin" in capi.SYMBOLS
    assert capi.Context.ROUTE_OPS["mul_sum_relin"] == 12
    assert callable(capi.Context.multiply_sum) and callable(capi.Context.mul_sum_relin)
