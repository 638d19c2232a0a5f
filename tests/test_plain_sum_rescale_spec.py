"""The K-term plaintext sum with ONE rescale behind it, and the baby-step giant-step matvec that rescales every inner sum before its
giant rotation, as tests/plain_sum_rescale_spec.py composes them from the CPU oracle, on the CPU: the rig of test_plain_sum_spec.py
(N = 1024, {50,40,40,50}, scale 2^40, 16 random diagonals in [-1, 1], baby 0..3, giant 0, 4, 8, 12, keys for the steps 1..15).

Measured with this file's seeds (max |error| of the decoded slots against the cleartext result):
  weighted sum, K = 2: 1.12e-09 with one rescale behind the sum, 1.29e-09 with a rescale per term; K = 8: 1.66e-09 and 3.04e-09 (the
  issue's own run, other inputs: 9.2e-10 / 1.4e-09 and 2.0e-09 / 2.3e-09); 100 % of the words of the two results differ, in every
  (component, limb), at either K;
  matvec: 7.48e-08 with the rescale before the giant rotations, 3.54e-08 with it behind diag_matvec_bsgs (the issue's run: 3.0e-08 /
  3.3e-08); 100 % of the words differ."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plain_sum_rescale_spec as spec  # noqa: E402
import plain_sum_spec as base  # noqa: E402

N, BITS, SCALE = 1024, [50, 40, 40, 50], 2.0 ** 40
BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]
BOUND = 1e-4  # the project's bound at this scale (tests/test_plain_sum_spec.py)
NAMES = ("abc_hip_multiply_plain_sum_rescale", "abc_hip_diag_matvec_bsgs_rescale")


@pytest.fixture(scope="module")
def rig(oracle_mod):
    om = oracle_mod
    o = om.Oracle(om.CKKS, N, om.create_primes(N, BITS))
    o.keygen(0xB565, elts=[o.elt_from_step(s) for s in range(1, 16)])
    rng = np.random.default_rng(16)
    x = rng.uniform(-1, 1, N // 2)
    diag_values = rng.uniform(-1, 1, (16, N // 2))
    steps = [g + b for g in GIANT for b in BABY]
    ct = o.encrypt(o.ckks_encode(x, SCALE), 7)
    diags = np.stack([o.ckks_encode(d, SCALE) for d in diag_values])
    clear = sum(d * np.roll(x, -s) for d, s in zip(diag_values, steps))
    # the weighted sum: eight inputs of their own, weights = the first eight diagonals
    xs = rng.uniform(-1, 1, (8, N // 2))
    cts = [o.encrypt(o.ckks_encode(v, SCALE), 100 + k) for k, v in enumerate(xs)]
    rot = base.bsgs_diagonals(o, diags, BABY, GIANT)
    lazy = spec.diag_matvec_bsgs_rescale(o, ct, rot, BABY, GIANT)
    after = o.rescale(base.diag_matvec_bsgs(o, ct, rot, BABY, GIANT))
    return dict(o=o, ct=ct, diags=diags, diag_values=diag_values, clear=clear, xs=xs, cts=cts, lazy=lazy, after=after,
                out_scale=SCALE * SCALE / o.primes[o.L - 1])


def _error(rig, ct, clear):
    o = rig["o"]
    return np.abs(o.ckks_decode(o.decrypt(ct), rig["out_scale"]) - clear).max()


@pytest.mark.parametrize("K", [2, 8])
def test_lazy_sum_decodes_to_the_weighted_sum_and_is_another_ciphertext_than_the_per_term_one(rig, K):
    o = rig["o"]
    cts, plains = rig["cts"][:K], list(rig["diags"][:K])
    clear = sum(rig["diag_values"][k] * rig["xs"][k] for k in range(K))
    lazy = spec.multiply_plain_sum_rescale(o, cts, plains)
    per_term = spec.per_term_rescaled_sum(o, cts, plains)
    assert lazy.shape == per_term.shape == (2, o.L - 1, N)
    e_lazy, e_term = _error(rig, lazy, clear), _error(rig, per_term, clear)
    differ = (lazy != per_term).reshape(2, o.L - 1, N).mean(axis=2)
    print("K = %d: max |error| lazy %.3g, per term %.3g; words that differ per (component, limb): %s" % (K, e_lazy, e_term, differ.tolist()))
    assert e_lazy < BOUND and e_term < BOUND
    assert (differ > 0.99).all()  # an implementation that rescales per term cannot pass the word-for-word GPU tests


def test_bsgs_rescale_decodes_to_the_cleartext_matvec_and_is_another_ciphertext_than_rescale_after(rig):
    e_lazy, e_after = _error(rig, rig["lazy"], rig["clear"]), _error(rig, rig["after"], rig["clear"])
    frac = (rig["lazy"] != rig["after"]).mean()
    print("max |error|: rescale before the giant steps %.3g, rescale after %.3g; words that differ: %.2f %%" % (e_lazy, e_after, 100 * frac))
    assert rig["lazy"].shape == rig["after"].shape == (2, rig["o"].L - 1, N)
    assert e_lazy < BOUND and e_after < BOUND
    assert frac > 0.99


def test_spec_edges(rig):
    o, ct, p = rig["o"], rig["ct"], rig["diags"][0]
    zero = spec.multiply_plain_sum_rescale(o, [], [], nl=3)
    assert zero.shape == (2, 2, N) and not zero.any()  # K = 0: rescale(0) = 0
    assert np.array_equal(spec.multiply_plain_sum_rescale(o, [], [], addend=ct), o.rescale(ct))  # the addend alone
    one = spec.multiply_plain_sum_rescale(o, [ct], [p])
    assert np.array_equal(one, o.rescale(o.multiply_plain(ct, p)))  # K = 1: multiply_plain + rescale
    assert np.array_equal(spec.multiply_plain_sum_rescale(o, [ct], [p], addend=ct), o.rescale(o.add(ct, o.multiply_plain(ct, p))))
    assert not spec.diag_matvec_bsgs_rescale(o, ct, rig["diags"][:0], [], GIANT).any()
    assert spec.diag_matvec_bsgs_rescale(o, ct, rig["diags"][:0], BABY, []).shape == (2, 2, N)


def test_library_exports_the_two_entry_points(capi):
    lib = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "abc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
        assert re.search(r"\bint %s\(abc_hip_ctx \*ctx" % name, header), name
        assert name in capi.SYMBOLS
    for method in ("multiply_plain_sum_rescale", "diag_matvec_bsgs_rescale"):
        assert callable(getattr(capi.Context, method))
    for macro, number, key in (("PLAIN_SUM_RESCALE", 16, "plain_sum_rescale"), ("DIAG_MATVEC_BSGS_RESCALE", 17, "diag_matvec_bsgs_rescale")):
        m = re.search(r"#define ABC_HIP_ROUTE_%s (\d+)" % macro, header)
        assert m and int(m.group(1)) == number == capi.Context.ROUTE_OPS[key]
