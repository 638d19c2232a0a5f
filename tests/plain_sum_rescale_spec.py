"""What abc_hip_multiply_plain_sum_rescale and abc_hip_diag_matvec_bsgs_rescale compute, composed from the CPU oracle's own operations
on one ciphertext ([size][nl][N] arrays): plain_sum_spec.multiply_plain_sum for the sum, Oracle.rescale behind it, Oracle.rotate and
Oracle.add for the giant steps, in the order the header gives."""
import numpy as np

import plain_sum_spec as base


def multiply_plain_sum_rescale(o, cts, plains, addend=None, size=2, nl=None):
    """rescale((addend or 0) + sum over k of plains[k] (.) cts[k]): ONE rescale, behind the sum; [size][nl - 1][N]"""
    return o.rescale(base.multiply_plain_sum(o, cts, plains, addend=addend, size=size, nl=nl))


def per_term_rescaled_sum(o, cts, plains):
    """sum over k of rescale(plains[k] (.) cts[k]): what K multiply_plain_rescale calls and K - 1 adds give -- the same values, K
    rescale roundings, other words"""
    acc = None
    for ct, p in zip(cts, plains):
        term = o.rescale(o.multiply_plain(ct, np.ascontiguousarray(np.asarray(p)[: np.shape(ct)[1]])))
        acc = term if acc is None else o.add(acc, term)
    return acc


def diag_matvec_bsgs_rescale(o, ct, bsgs_diags, baby, giant):
    """sum over j of rotate(rescale(sum over i of bsgs_diags[j * len(baby) + i] (.) rotate(ct, baby[i])), giant[j]): the baby rotations at
    nl, per giant step the rescaled inner sum, its rotation at nl - 1 (none for a step of 0) and the add onto the running sum"""
    nb = len(baby)
    if not nb or not len(giant):
        return np.zeros((ct.shape[0], ct.shape[1] - 1, ct.shape[2]), dtype=np.uint64)
    rot = [o.rotate(ct, b) if b else ct for b in baby]
    acc = None
    for j, g in enumerate(giant):
        inner = multiply_plain_sum_rescale(o, rot, [bsgs_diags[j * nb + i] for i in range(nb)])
        term = o.rotate(inner, g) if g else inner
        acc = term if acc is None else o.add(acc, term)
    return acc
