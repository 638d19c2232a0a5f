"""What abc_hip_multiply_sum and abc_hip_mul_sum_relin compute, composed from the CPU oracle's own operations on one ciphertext
([size][nl][N] arrays): the oracle's multiply per term, its add on the size-3 products, and -- for the second call -- ONE relinearize
of the sum.  The sum of K relinearised products is a different ciphertext (K key switches, K roundings): per_term_relin below, which
tests/test_mul_sum_spec.py shows to differ from the spec in nearly every word."""
import numpy as np


def multiply_sum(o, as_, bs, nl=None):
    """size-3 sum of the products as_[k] (x) bs[k]; an empty sum is zero at level nl"""
    assert len(as_) == len(bs)
    if not as_:
        return np.zeros((3, nl, o.n), dtype=np.uint64)
    acc = o.multiply(as_[0], bs[0])
    for a, b in zip(as_[1:], bs[1:]):
        acc = o.add(acc, o.multiply(a, b))
    return acc


def mul_sum_relin(o, as_, bs, nl=None):
    """relinearize(multiply_sum): one key switch for the whole sum"""
    if not as_:
        return np.zeros((2, nl, o.n), dtype=np.uint64)
    return o.relinearize(multiply_sum(o, as_, bs))


def per_term_relin(o, as_, bs):
    """the eager form: every product relinearised, then added.  Decrypts to the same values; not the same words"""
    acc = o.mul_relin(as_[0], bs[0])
    for a, b in zip(as_[1:], bs[1:]):
        acc = o.add(acc, o.mul_relin(a, b))
    return acc
