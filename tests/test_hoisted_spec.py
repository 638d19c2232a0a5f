"""The hoisted form of a rotation (tests/hoisted_spec.py) on the CPU oracle alone: it decrypts as the regular rotation does, with
the same noise, and is a different ciphertext -- so nobody "simplifies" the reference of the device tests to o.apply_galois."""
import os
import re

import numpy as np

from hoisted_spec import hoisted_reference, permuted_key


def test_bfv_hoisted_rotation_decrypts_like_the_regular_one(oracle_mod):
    n = 4096
    o = oracle_mod.Oracle.bfv_default(n)
    elts = [o.elt_from_step(s) for s in (1, -2, 0)]  # step 0: the column swap, element 2N - 1
    assert elts[2] == 2 * n - 1
    o.keygen(0xABC00001, elts=elts)
    rng = np.random.default_rng(1)
    vals = rng.integers(-1000, 1000, size=n)
    ct = o.encrypt(o.encode(vals), 7)
    for elt in elts:
        want, got = o.apply_galois(ct, elt), hoisted_reference(o, ct, elt)
        assert np.array_equal(o.decode(o.decrypt(got)), o.decode(o.decrypt(want))), elt
        assert abs(o.noise_budget(got) - o.noise_budget(want)) <= 1, elt
        assert not np.array_equal(got, want), elt
    row = n // 2
    d = o.decode(o.decrypt(hoisted_reference(o, ct, elts[0]))).reshape(2, row)
    assert np.array_equal(d, np.roll(vals.reshape(2, row), -1, axis=1))


def test_ckks_hoisted_rotation_within_the_regular_bound_and_a_different_ciphertext(oracle_mod):
    n = 1024
    primes = oracle_mod.create_primes(n, [50, 40, 40, 50])
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, primes)
    steps = (1, 4)
    elts = [o.elt_from_step(s) for s in steps] + [2 * n - 1]  # and the conjugation
    o.keygen(0xABC00002, elts=elts)
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, n // 2) + 1j * rng.uniform(-1, 1, n // 2)
    scale = 2.0 ** 40
    ct = o.encrypt(o.ckks_encode(x, scale), 3)
    for level in (3, 2, 1):
        assert ct.shape[1] == level
        for elt, want_x in zip(elts, [np.roll(x, -1), np.roll(x, -4), np.conj(x)]):
            got = hoisted_reference(o, ct, elt)
            err = np.abs(o.ckks_decode(o.decrypt(got), scale) - want_x).max()
            assert err < 1e-4, (level, elt, err)  # the bound of the regular rotation at this scale (test_gpu_properties.py)
            reg = o.apply_galois(ct, elt)
            assert np.abs(o.ckks_decode(o.decrypt(reg), scale) - want_x).max() < 1e-4
            assert (got != reg).mean() > 0.99, (level, elt)
        if level > 1:
            ct = o.mod_switch(ct)


def test_permuted_key_is_an_index_permutation_of_every_row(oracle_mod):
    n = 1024
    o = oracle_mod.Oracle(oracle_mod.CKKS, n, oracle_mod.create_primes(n, [50, 40, 50]))
    elt = o.elt_from_step(3)
    o.keygen(5, elts=[elt])
    key, perm = o.galois_key(elt), permuted_key(o, elt)
    assert perm.shape == key.shape and not np.array_equal(perm, key)
    assert np.array_equal(np.sort(perm, axis=-1), np.sort(key, axis=-1))
    back = np.stack([np.stack([o.galois_permute(perm[d, c], elt, True) for c in range(2)]) for d in range(key.shape[0])])
    assert np.array_equal(back, key)  # s_g undoes s_{g^-1}


def test_library_exports_the_hoisted_entry_points(capi):
    lib = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "abc_hip.h")).read()
    for name in ("abc_hip_apply_galois_hoisted", "abc_hip_rotate_hoisted"):
        assert hasattr(lib, name), "missing export: " + name
        assert re.search(r"\bint %s\(abc_hip_ctx \*" % name, header), name
        assert name in capi.SYMBOLS
    for method in ("apply_galois_hoisted", "rotate_hoisted"):
        assert callable(getattr(capi.Context, method))
