"""The baby-step giant-step matvec and the plaintext rotation as tests/plain_sum_spec.py composes them from the CPU oracle, on the CPU:
N = 1024, {50,40,40,50}, scale 2^40, 16 random diagonals in [-1, 1], baby 0..3, giant 0, 4, 8, 12, keys for the steps 1..15.

Measured with this file's seeds (max |error| against the cleartext matvec, at the scale of the product): 6.9e-08 for the composed
diag_matvec, 3.6e-08 for BSGS (the issue's own run, other seeds: 2.8e-08 and 4.3e-08); 100 % of the two results' words differ; BSGS
on diagonals that were NOT pre-rotated misses the cleartext result by 5.18 (there: 4.98); rotate_plain's spec equals ckks_encode of
the rolled vector in every word."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plain_sum_spec as spec  # noqa: E402

N, BITS, SCALE = 1024, [50, 40, 40, 50], 2.0 ** 40
BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]
BOUND = 1e-4  # the project's bound for a rotation at this scale (tests/test_hoisted_spec.py)
NAMES = ("abc_hip_multiply_plain_sum", "abc_hip_rotate_plain", "abc_hip_diag_matvec_bsgs")


@pytest.fixture(scope="module")
def rig(oracle_mod):
    om = oracle_mod
    o = om.Oracle(om.CKKS, N, om.create_primes(N, BITS))
    o.keygen(0xB565, elts=[o.elt_from_step(s) for s in range(1, 16)])
    rng = np.random.default_rng(16)
    x = rng.uniform(-1, 1, N // 2)
    diag_values = rng.uniform(-1, 1, (16, N // 2))
    steps = [g + b for g in GIANT for b in BABY]
    assert steps == list(range(16))
    ct = o.encrypt(o.ckks_encode(x, SCALE), 7)
    diags = np.stack([o.ckks_encode(d, SCALE) for d in diag_values])
    clear = sum(d * np.roll(x, -s) for d, s in zip(diag_values, steps))
    composed = spec.diag_matvec(o, ct, diags, steps)
    bsgs = spec.diag_matvec_bsgs(o, ct, spec.bsgs_diagonals(o, diags, BABY, GIANT), BABY, GIANT)
    return dict(o=o, x=x, diag_values=diag_values, ct=ct, diags=diags, clear=clear, composed=composed, bsgs=bsgs)


def _error(o, ct, clear):
    return np.abs(o.ckks_decode(o.decrypt(ct), SCALE * SCALE) - clear).max()


def test_bsgs_decodes_to_the_cleartext_matvec_within_the_bound_of_the_composed_one(rig):
    e_composed, e_bsgs = _error(rig["o"], rig["composed"], rig["clear"]), _error(rig["o"], rig["bsgs"], rig["clear"])
    print("max |error|: composed diag_matvec %.3g, BSGS %.3g" % (e_composed, e_bsgs))
    assert e_composed < BOUND and e_bsgs < BOUND


def test_bsgs_is_another_ciphertext_than_the_composed_matvec(rig):
    frac = (rig["bsgs"] != rig["composed"]).mean()
    print("words that differ: %.2f %%" % (100 * frac))
    assert frac > 0.99  # an implementation that forwards to diag_matvec cannot pass the word-for-word GPU tests


def test_diagonals_that_were_not_pre_rotated_give_another_matrix(rig):
    o = rig["o"]
    wrong = spec.diag_matvec_bsgs(o, rig["ct"], rig["diags"], BABY, GIANT)
    miss = _error(o, wrong, rig["clear"])
    print("without the pre-rotation: max |error| %.3g" % miss)
    assert miss > 1


def test_rotate_plain_is_the_encoding_of_the_rolled_vector(rig):
    o = rig["o"]
    for s in (1, 5, 12, -4, -12, 0):
        got = spec.rotate_plain(o, rig["diags"][3], s)
        want = o.ckks_encode(np.roll(rig["diag_values"][3], -s), SCALE)
        assert np.array_equal(got, want), s


def test_multiply_plain_sum_spec_edges(rig):
    o, ct = rig["o"], rig["ct"]
    assert not spec.multiply_plain_sum(o, [], [], nl=3).any()
    assert np.array_equal(spec.multiply_plain_sum(o, [], [], addend=ct), ct)
    one = spec.multiply_plain_sum(o, [ct], [rig["diags"][0]])
    assert np.array_equal(one, o.multiply_plain(ct, rig["diags"][0]))
    assert np.array_equal(spec.multiply_plain_sum(o, [ct], [rig["diags"][0]], addend=ct), o.add(ct, one))


def test_library_exports_the_three_entry_points(capi):
    lib = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "abc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
        assert re.search(r"\bint %s\(abc_hip_ctx \*ctx" % name, header), name
        assert name in capi.SYMBOLS
    for method in ("multiply_plain_sum", "rotate_plain", "bsgs_diagonals", "diag_matvec_bsgs"):
        assert callable(getattr(capi.Context, method))
    m = re.search(r"#define ABC_HIP_ROUTE_DIAG_MATVEC_BSGS (\d+)", header)
    assert m and int(m.group(1)) == 13 == capi.Context.ROUTE_OPS["diag_matvec_bsgs"]
