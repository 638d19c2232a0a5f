"""tests/bfv_plain_sum_spec.py against the CPU oracle's own BFV calls, on the CPU.

The NTT-domain sum (one inverse transform) equals oracle.multiply_plain per term + oracle.add in every word: the inverse transform
is linear and every step is exact modulo q_i.  The baby-step giant-step matvec decodes to the cleartext matrix-vector product
modulo t exactly; with diagonals that were not rolled it does not; its noise budget is positive on the ring the GPU end-to-end test
uses (BFVDefault(8192))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bfv_plain_sum_spec as spec  # noqa: E402

K = 5
NAMES = ("abc_hip_bfv_plain_to_ntt", "abc_hip_bfv_multiply_plain_sum", "abc_hip_bfv_diag_matvec_bsgs")


def _oracle(om, kind):
    if kind == "default4096":
        return om.Oracle.bfv_default(4096)
    bits = {"40-40-50": [40, 40, 50], "60-40-60": [60, 40, 60]}[kind]
    return om.Oracle(om.BFV, 1024, om.create_primes(1024, bits), om.plain_modulus_batching(1024, 20))


def _plains(o, rng):
    """five plaintexts: t - 1 everywhere, the two values around the lift threshold (and 0) by coefficient, random ones"""
    t, thr = o.t, (o.t + 1) // 2
    edge = np.array([0, t - 1, thr - 1, thr], dtype=np.uint64)
    return [np.full(o.n, t - 1, dtype=np.uint64), edge[np.arange(o.n) % 4], edge[(np.arange(o.n) // 3) % 4][::-1].copy(),
            rng.integers(0, t, o.n, dtype=np.uint64), rng.integers(0, t, o.n, dtype=np.uint64)]


@pytest.mark.parametrize("kind", ["40-40-50", "60-40-60", "default4096"])
@pytest.mark.parametrize("size", [2, 3])
def test_ntt_domain_sum_equals_multiply_plain_per_term_and_add(oracle_mod, kind, size):
    o = _oracle(oracle_mod, kind)
    rng = np.random.default_rng(o.n + size)
    cts = [np.stack([rng.integers(0, q, size=(size, o.n), dtype=np.uint64) for q in o.primes[:o.L]], axis=1) for _ in range(K + 1)]
    plains = _plains(o, rng)
    p_ntt = [spec.plain_to_ntt(o, p) for p in plains]
    want = spec.composed_sum(o, cts[:K], plains)
    assert np.array_equal(spec.multiply_plain_sum(o, cts[:K], p_ntt), want)
    assert np.array_equal(spec.multiply_plain_sum(o, cts[:K], p_ntt, addend=cts[K]), o.add(cts[K], want))
    # one term: the words of multiply_plain
    assert np.array_equal(spec.multiply_plain_sum(o, cts[:1], p_ntt[:1]), o.multiply_plain(cts[0], plains[0]))
    # terms handed over in NTT form: oracle.ntt limb by limb
    x_ntt = [spec.ct_to_ntt(o, c) for c in cts[:K]]
    assert np.array_equal(x_ntt[0][1, 0], o.ntt(0, cts[0][1, 0]))
    assert np.array_equal(spec.multiply_plain_sum(o, x_ntt, p_ntt, ct_form=spec.NTT), want)
    # the empty sum
    assert not spec.multiply_plain_sum(o, [], [], size=size).any()
    assert np.array_equal(spec.multiply_plain_sum(o, [], [], addend=cts[0]), cts[0])


def test_lift_moves_the_upper_half_by_q_minus_t(oracle_mod):
    o = _oracle(oracle_mod, "40-40-50")
    thr = (o.t + 1) // 2
    p = np.zeros(o.n, dtype=np.uint64)
    p[:4] = [0, thr - 1, thr, o.t - 1]
    got = spec.lift(o, p)
    for i, q in enumerate(o.primes[:o.L]):
        assert [int(v) for v in got[i, :4]] == [0, thr - 1, q - o.t + thr, q - 1]


N_E2E, DIM, BABY, GIANT = 8192, 16, [0, 1, 2, 3], [0, 4, 8, 12]


@pytest.fixture(scope="module")
def matvec(oracle_mod):
    om = oracle_mod
    o = om.Oracle.bfv_default(N_E2E)
    o.keygen(0xB5F5, elts=[o.elt_from_step(s) for s in sorted(set(BABY + GIANT) - {0})])
    rng = np.random.default_rng(DIM)
    m = rng.integers(0, 64, (DIM, DIM))
    x = rng.integers(0, 64, DIM)
    tile = o.n // 2 // DIM
    xs = np.tile(x, 2 * tile)
    steps = [g + b for g in GIANT for b in BABY]
    diag_values = [np.tile(m[np.arange(DIM), (np.arange(DIM) + s) % DIM], 2 * tile) for s in steps]
    ct = o.encrypt(o.encode(xs), 3)
    return dict(o=o, m=m, x=x, ct=ct, diag_values=diag_values, want=(m @ x) % o.t)


def test_bsgs_decodes_to_the_cleartext_matvec_exactly_with_budget_left(matvec):
    o = matvec["o"]
    out = spec.diag_matvec_bsgs(o, matvec["ct"], spec.bsgs_diagonals(o, matvec["diag_values"], BABY, GIANT), BABY, GIANT)
    got = o.decode(o.decrypt(out))
    assert np.array_equal(got[:DIM] % o.t, matvec["want"])
    assert np.array_equal(got[o.n // 2:o.n // 2 + DIM] % o.t, matvec["want"])
    budget = o.noise_budget(out)
    print("noise budget of the BSGS matvec on BFVDefault(%d): %d bits (fresh: %d)" % (o.n, budget, o.noise_budget(matvec["ct"])))
    assert budget > 0


def test_diagonals_that_were_not_rolled_give_another_matrix(matvec):
    o = matvec["o"]
    plain_rows = [o.encode(d) for d in matvec["diag_values"]]
    out = spec.diag_matvec_bsgs(o, matvec["ct"], plain_rows, BABY, GIANT)
    assert not np.array_equal(o.decode(o.decrypt(out))[:DIM] % o.t, matvec["want"])


def test_library_exports_the_entry_points(capi):
    import re
    lib = capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "abc_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), "missing export: " + name
        assert re.search(r"\bint %s\(abc_hip_ctx \*" % name, header), name
        assert name in capi.SYMBOLS
    for method in ("bfv_plain_to_ntt", "bfv_multiply_plain_sum", "bfv_bsgs_diagonals", "bfv_diag_matvec_bsgs"):
        assert callable(getattr(capi.Context, method))
    assert capi.Context.ROUTE_OPS["bfv_plain_sum"] == 14 and capi.Context.ROUTE_OPS["bfv_matvec_bsgs"] == 15
