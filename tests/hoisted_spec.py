"""Hoisted rotations ("Hoisted rotations") composed from oracle calls -- TEST INFRASTRUCTURE ONLY.

    hoisted(ct, g) = ( s_g(ks0 + c0), s_g(ks1) ),   (ks0, ks1) = KeySwitch(c1, key'_g)

key'_g is the Galois key of g with every [N] row permuted by g^-1 mod 2N in NTT form; the key switch is the oracle's own, on
the UNPERMUTED c1; s_g acts in the ciphertext's form (NTT-index permutation for CKKS, signed coefficient permutation for BFV).
Not the oracle's apply_galois, which decomposes s_g(c1): the two decrypt alike and differ in every word.
"""
import numpy as np


def permuted_key(o, elt):
    """key'_g: uint64 [L][2][K][N]"""
    key = o.galois_key(elt)
    ginv = pow(int(elt), -1, 2 * o.n)
    out = np.empty_like(key)
    for d in range(key.shape[0]):
        for c in range(2):
            out[d, c] = o.galois_permute(key[d, c], ginv, True)  # K rows, row j modulo key prime j: an index permutation
    return out


def hoisted_reference(o, ct, elt, key=None):
    """ct uint64 [2][nl][N] -> [2][nl][N]; key: permuted_key(o, elt) if the caller has it already"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    ks = o.keyswitch(ct[1], permuted_key(o, elt) if key is None else key)
    s0 = o.add(ks[0:1], ct[0:1])[0]
    ntt_form = o.scheme == 2  # CKKS
    return np.stack([o.galois_permute(s0, elt, ntt_form), o.galois_permute(ks[1], elt, ntt_form)])
