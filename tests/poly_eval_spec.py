"""What abc_hip_ckks_poly_eval computes: the fixed sequence of include/abc_hip.h restated on the CPU oracle, one ciphertext
([2][level][N] arrays) at a time.

  x^1 = x: level(1) = nl, scale(1) = x_scale.  For k = 2 .. d: e = ceil(log2 k), h = 2^(e-1), l = k - h,
  x^k = rescale(mul_relin(x^h, mod_switch(x^l down to nl - e + 1 limbs))), level(k) = nl - e, scale(k) = scale(h) scale(l) / q_{nl-e}.
  E = ceil(log2 d), m = nl - E;  W_k = const_words(c_k, out_scale q_{m-1} / scale(k), m), W_0 = const_words(c_0, out_scale q_{m-1}, m);
  the output is ONE multiply_const_sum_rescale at level m over the powers, each read at its own level.

`plan` is the host half (levels, scales, weights: doubles, in the order the library evaluates them); `poly_eval` the whole;
`poly_eval_composed` is what a caller writes without it: encoded constant vectors, a rescale per product, mod_switch, add."""
import numpy as np

import const_sum_spec as cs


def ceil_log2(k):
    e = 0
    while (1 << e) < k:
        e += 1
    return e


def depth(degree):
    return ceil_log2(degree) + 1


def plan(primes, nl, x_scale, coeffs, out_scale):
    """levels, scales, which powers are formed, the terms of the last sum and their words"""
    d = len(coeffs) - 1
    assert 1 <= d <= 31 and nl >= ceil_log2(d) + 2
    level, scale, hi, lo = [nl] * (d + 1), [float(x_scale)] * (d + 1), [0] * (d + 1), [0] * (d + 1)
    for k in range(2, d + 1):
        e = ceil_log2(k)
        hi[k], lo[k], level[k] = 1 << (e - 1), k - (1 << (e - 1)), nl - e
        scale[k] = scale[hi[k]] * scale[lo[k]] / float(primes[nl - e])
    need = [False] + [float(coeffs[k]) != 0.0 for k in range(1, d + 1)]
    for k in range(d, 1, -1):
        if need[k]:
            need[hi[k]] = need[lo[k]] = True
    m = nl - ceil_log2(d)
    top = float(out_scale) * float(primes[m - 1])
    terms = [k for k in range(1, d + 1) if float(coeffs[k]) != 0.0]
    weights = [cs.const_words(primes, coeffs[k], top / scale[k], m) for k in terms]
    w0 = cs.const_words(primes, coeffs[0], top, m)
    return dict(d=d, m=m, level=level, scale=scale, hi=hi, lo=lo, need=need, terms=terms, weights=weights, w0=w0)


def powers(o, x, p):
    """{k: x^k at level(k)} for the powers the plan forms"""
    pw = {1: np.ascontiguousarray(x)}
    for k in range(2, p["d"] + 1):
        if not p["need"][k]:
            continue
        lk = p["level"][k] + 1
        pw[k] = o.rescale(o.mul_relin(pw[p["hi"][k]], cs.lower(o, pw[p["lo"][k]], lk)))
    return pw


def poly_eval(o, x, x_scale, coeffs, out_scale):
    """[2][nl - depth][N] at out_scale"""
    p = plan(o.primes, x.shape[1], x_scale, coeffs, out_scale)
    pw = powers(o, x, p)
    return cs.multiply_const_sum_rescale(o, [pw[k] for k in p["terms"]], p["weights"], const=p["w0"], nl=p["m"])


def poly_eval_composed(o, x, x_scale, coeffs, out_scale):
    """the same polynomial as a caller composes it today: the powers as above; per term an ENCODED vector of N/2 copies of c_k at the
    scale that brings the product to out_scale after ITS OWN rescale at the power's level, mod_switch down to the common level, add;
    the constant encoded at out_scale and added last.  [2][nl - depth][N] at out_scale"""
    p = plan(o.primes, x.shape[1], x_scale, coeffs, out_scale)
    pw = powers(o, x, p)
    slots, last = o.n // 2, p["m"] - 1
    acc = None
    for k in p["terms"]:
        lk = p["level"][k]
        plain = o.ckks_encode(np.full(slots, float(coeffs[k])), float(out_scale) * float(o.primes[lk - 1]) / p["scale"][k], lk)
        term = cs.lower(o, o.rescale(o.multiply_plain(pw[k], plain)), last)
        acc = term if acc is None else o.add(acc, term)
    c0 = o.ckks_encode(np.full(slots, float(coeffs[0])), float(out_scale), last)
    if acc is None:
        acc = np.zeros((2, last, o.n), dtype=np.uint64)
    return o.add_plain(acc, c0)
