"""What abc_hip_bfv_plain_to_ntt, abc_hip_bfv_multiply_plain_sum and abc_hip_bfv_diag_matvec_bsgs compute, on the CPU oracle's
transforms and Python integers.  The sum is the exact NTT-domain model -- the big-integer sum of the limb-wise products, reduced
once, then ONE oracle.intt per limb -- so that arbitrary residues (q - 1 in every word) have a reference; tests/test_bfv_plain_sum_spec.py
shows that on real plaintexts it equals oracle.multiply_plain per term and oracle.add in every word."""
import numpy as np

COEFF, NTT = 0, 1  # ABC_HIP_CT_COEFF, ABC_HIP_CT_NTT


def lift(o, plain):
    """[N] mod t -> [L][N]: Evaluator::multiply_plain's lift, values of (t + 1) / 2 and above move up by q_i - t"""
    p = np.ascontiguousarray(plain, dtype=np.uint64)
    thr = np.uint64((o.t + 1) // 2)
    return np.stack([np.where(p >= thr, p + np.uint64(q - o.t), p) for q in o.primes[:o.L]])


def plain_to_ntt(o, plain):
    """[N] mod t -> [L][N] in NTT form: the lift, then the forward transform per data limb"""
    return np.stack([o.ntt(i, row) for i, row in enumerate(lift(o, plain))])


def ct_to_ntt(o, ct):
    """[size][L][N] coefficient form -> NTT form limb by limb (Evaluator::transform_to_ntt_inplace)"""
    ct = np.asarray(ct, dtype=np.uint64)
    return np.stack([np.stack([o.ntt(i, ct[s, i]) for i in range(ct.shape[1])]) for s in range(ct.shape[0])])


def multiply_plain_sum(o, cts, plains_ntt, addend=None, ct_form=COEFF, size=2):
    """(addend or 0) + sum over k of plains_ntt[k] * cts[k] for one ciphertext: cts[k] [size][L][N] in the form ct_form says,
    plains_ntt[k] [L][N] any residues below q_i, addend and result in coefficient form"""
    assert len(cts) == len(plains_ntt)
    if not cts:
        return np.zeros((size, o.L, o.n), dtype=np.uint64) if addend is None else np.array(addend, dtype=np.uint64)
    xs = [np.asarray(c, dtype=np.uint64) if ct_form == NTT else ct_to_ntt(o, c) for c in cts]
    out = np.empty_like(xs[0])
    for s in range(out.shape[0]):
        for i in range(o.L):
            q = o.primes[i]
            acc = np.zeros(o.n, dtype=object)
            for x, p in zip(xs, plains_ntt):
                acc = acc + x[s, i].astype(object) * np.asarray(p)[i].astype(object)
            r = o.intt(i, np.array([int(v) % q for v in acc], dtype=np.uint64))
            if addend is not None:
                r = (r + np.asarray(addend, dtype=np.uint64)[s, i]) % np.uint64(q)  # both below 2^60: no overflow
            out[s, i] = r
    return out


def composed_sum(o, cts, plains, addend=None):
    """the same from the oracle's own calls, for plaintexts [N] mod t: multiply_plain per term, add"""
    acc = None if addend is None else np.ascontiguousarray(addend)
    for ct, p in zip(cts, plains):
        prod = o.multiply_plain(np.ascontiguousarray(ct), np.ascontiguousarray(p, dtype=np.uint64))
        acc = prod if acc is None else o.add(acc, prod)
    return acc


def roll_rows(o, values, steps):
    """the slots of rotate(ct, steps): each half of the N values (a row of the 2 x N/2 batching matrix) rolled left by steps"""
    v = np.asarray(values).reshape(2, o.n // 2)
    return np.roll(v, -steps, axis=1).reshape(o.n)


def bsgs_diagonals(o, diag_values, baby, giant):
    """rows abc_hip_bfv_diag_matvec_bsgs takes, as plaintexts [N] mod t: row (j, i) encodes the cleartext diagonal of step
    giant[j] + baby[i] with each half-row rolled by -giant[j]"""
    nb = len(baby)
    return [o.encode(roll_rows(o, diag_values[j * nb + i], -giant[j])) for j in range(len(giant)) for i in range(nb)]


def diag_matvec_bsgs(o, ct, plains, baby, giant):
    """sum over j of rotate(sum over i of plains[j * nb + i] * rotate(ct, baby[i]), giant[j]), plains [N] mod t, composed from
    oracle.rotate, multiply_plain and add in the order the header gives"""
    nb = len(baby)
    if not nb or not len(giant):
        return np.zeros_like(ct)
    rot = [o.rotate(ct, b) if b else ct for b in baby]
    acc = None
    for j, g in enumerate(giant):
        inner = composed_sum(o, rot, plains[j * nb:(j + 1) * nb])
        term = o.rotate(inner, g) if g else inner
        acc = term if acc is None else o.add(acc, term)
    return acc
