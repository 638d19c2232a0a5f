"""What abc_hip_multiply_plain_sum, abc_hip_rotate_plain and abc_hip_diag_matvec_bsgs compute, composed from the CPU oracle's own
operations on one ciphertext ([size][nl][N] arrays) and on plaintexts ([rows >= nl][N]): multiply_plain, add and rotate for the
ciphertext side, in the order the header gives, and galois_permute for the plaintext side."""
import numpy as np


def multiply_plain_sum(o, cts, plains, addend=None, size=2, nl=None):
    """(addend or 0) + sum over k of plains[k] (.) cts[k]; a plaintext's first nl limbs are read"""
    assert len(cts) == len(plains)
    acc = None if addend is None else np.ascontiguousarray(addend)
    for ct, p in zip(cts, plains):
        prod = o.multiply_plain(ct, np.ascontiguousarray(np.asarray(p)[: np.shape(ct)[1]]))
        acc = prod if acc is None else o.add(acc, prod)
    if acc is None:
        return np.zeros((size, nl, o.n), dtype=np.uint64)
    return acc


def rotate_plain(o, plain, steps):
    """the slot rotation of an NTT-form plaintext [rows][N]: the index permutation of the step's Galois element, limb by limb"""
    plain = np.ascontiguousarray(plain)
    if steps == 0:
        return plain.copy()
    return o.galois_permute(plain, o.elt_from_step(steps), True)


def bsgs_diagonals(o, diags, baby, giant):
    """row (j, i) = rotate_plain(diags[j * len(baby) + i], -giant[j]), diags[j * len(baby) + i] the diagonal of step giant[j] + baby[i]"""
    nb = len(baby)
    return np.stack([rotate_plain(o, diags[j * nb + i], -giant[j]) for j in range(len(giant)) for i in range(nb)]) if nb * len(giant) else \
        np.zeros((0,) + np.shape(diags)[1:], dtype=np.uint64)


def diag_matvec(o, ct, diags, steps):
    """abc_hip_diag_matvec composed: sum over r of diags[r] (.) rotate(ct, steps[r]), in order"""
    nl = ct.shape[1]
    acc = None
    for d, s in zip(diags, steps):
        term = o.multiply_plain(o.rotate(ct, s) if s else ct, np.ascontiguousarray(d[:nl]))
        acc = term if acc is None else o.add(acc, term)
    return np.zeros_like(ct) if acc is None else acc


def diag_matvec_bsgs(o, ct, bsgs_diags, baby, giant):
    """sum over j of rotate(sum over i of bsgs_diags[j * len(baby) + i] (.) rotate(ct, baby[i]), giant[j]): the baby rotations first, then
    per giant step the inner sum, its rotation (none for a step of 0) and the add onto the running sum"""
    nb = len(baby)
    if not nb or not len(giant):
        return np.zeros_like(ct)
    rot = [o.rotate(ct, b) if b else ct for b in baby]
    acc = None
    for j, g in enumerate(giant):
        inner = multiply_plain_sum(o, rot, [bsgs_diags[j * nb + i] for i in range(nb)])
        term = o.rotate(inner, g) if g else inner
        acc = term if acc is None else o.add(acc, term)
    return acc
