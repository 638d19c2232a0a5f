"""What abc_hip_ckks_const_words, abc_hip_multiply_const_sum and abc_hip_multiply_const_sum_rescale compute.

const_words is exact integer arithmetic on the rounded product.  The sums come twice: `multiply_const_sum`, composed from the CPU
oracle's own operations on one ciphertext ([size][level][N] arrays) in the order the header gives -- mod_switch down to nl,
multiply_plain with the constant plaintext, add, add_plain for the constant -- which is the reference of the device tests; and
`multiply_const_sum_words`, the same words from Python integers alone, which tests/test_const_sum_spec.py holds against it."""
import math
from fractions import Fraction

import numpy as np


def const_words(primes, value, scale, nl):
    """r = value * scale (the double product) rounded to the nearest integer, ties away from zero; r mod q_j in [0, q_j), uint64 [nl]"""
    r = float(value) * float(scale)
    if not math.isfinite(r):
        raise ValueError("value * scale is not finite")
    f = Fraction(r)
    mag = (abs(f) + Fraction(1, 2)).__floor__()
    if mag >= 2 ** 62:
        raise ValueError("|value * scale| must stay below 2^62")
    ri = -mag if f < 0 else mag
    return np.array([ri % int(q) for q in primes[:nl]], dtype=np.uint64)  # Python's % is already in [0, q)


def const_plain(words, n):
    """the constant in NTT form: every word of limb j is words[j]; [nl][N]"""
    return np.ascontiguousarray(np.repeat(np.asarray(words, dtype=np.uint64)[:, None], n, axis=1))


def lower(o, ct, nl):
    """mod_switch repeated down to nl limbs"""
    while ct.shape[1] > nl:
        ct = o.mod_switch(ct)
    return ct


def multiply_const_sum(o, cts, weights, const=None, addend=None, size=2, nl=None):
    """(addend or 0) + const (component 0) + sum over k of weights[k] * cts[k]; cts[k] [size][its level >= nl][N]; weights [K][nl],
    const [nl]: words.  nl: the addend's level, else the lowest among the terms, unless given"""
    if nl is None:
        nl = addend.shape[1] if addend is not None else min(c.shape[1] for c in cts)
    acc = None if addend is None else np.ascontiguousarray(addend)
    for ct, w in zip(cts, weights):
        term = o.multiply_plain(lower(o, np.ascontiguousarray(ct), nl), const_plain(w, o.n))
        acc = term if acc is None else o.add(acc, term)
    if acc is None:
        acc = np.zeros((size, nl, o.n), dtype=np.uint64)
    if const is not None:
        acc = o.add_plain(acc, const_plain(const, o.n))
    return acc


def multiply_const_sum_rescale(o, cts, weights, const=None, addend=None, size=2, nl=None):
    """ONE rescale, behind the sum; [size][nl - 1][N]"""
    return o.rescale(multiply_const_sum(o, cts, weights, const=const, addend=addend, size=size, nl=nl))


def per_term_rescaled_sum(o, cts, weights):
    """sum over k of rescale(weights[k] * cts[k]), every term at one level: what K multiply_plain_rescale calls and K - 1 adds give"""
    acc = None
    for ct, w in zip(cts, weights):
        term = o.rescale(o.multiply_plain(np.ascontiguousarray(ct), const_plain(w, o.n)))
        acc = term if acc is None else o.add(acc, term)
    return acc


def multiply_const_sum_words(primes, cts, weights, const=None, addend=None, size=2, nl=None):
    """multiply_const_sum from Python integers: no oracle"""
    if nl is None:
        nl = addend.shape[1] if addend is not None else min(c.shape[1] for c in cts)
    n = (cts[0] if len(cts) else addend).shape[2] if (len(cts) or addend is not None) else None
    q = np.array([int(p) for p in primes[:nl]], dtype=object)[None, :, None]
    acc = np.zeros((size, nl, n), dtype=object) if addend is None else np.asarray(addend).astype(object)
    for ct, w in zip(cts, weights):
        wk = np.array([int(v) for v in w], dtype=object)[None, :, None]
        acc = (acc + np.asarray(ct)[:, :nl].astype(object) * wk) % q
    if const is not None:
        acc[0] = (acc[0] + np.array([int(v) for v in const], dtype=object)[:, None]) % q[0]
    return acc.astype(np.uint64)
