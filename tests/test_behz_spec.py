"""tests/behz_spec.py against the CPU oracle: the big-integer model of DESIGN.md section 4c equals the oracle's BEHZ multiply on
every word, the crafted coefficients reach the decision points they claim, and a model with the tie of r centred the other way
differs from the oracle at exactly the coefficients crafted for r = 2^31 -- so the inputs of tests/test_gpu_behz_decisions.py
discriminate.  Decryption: the oracle's gamma-corrected rounding against exact rounding away from the rounding boundaries."""
import ctypes as C

import numpy as np
import pytest

import behz_spec as bs

CHAINS = {  # name: (N, key-prime widths; None: BFVDefault), sparse terms of b in the crafted row
    "N1024-40-45-50": (1024, [40, 45, 50], 5),
    "BFVDefault4096": (4096, None, 0),
    "N4096-58-52-60": (4096, [58, 52, 60], 0),  # the oracle's auxiliary base: 61-bit primes
}


def _oracle(om, name):
    n, bits, _ = CHAINS[name]
    if bits is None:
        return om.Oracle.bfv_default(n)
    return om.Oracle(om.BFV, n, om.create_primes(n, bits), om.plain_modulus_batching(n, 20))


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """per chain: the oracle, the model, the crafted batch and the oracle's products (computed once, read-only)"""
    cache = {}

    def get(name):
        if name not in cache:
            o = _oracle(oracle_mod, name)
            spec = bs.Behz(o.primes[:-1], o.t)
            rng = np.random.default_rng(len(name))
            a, terms, marks = bs.crafted_batch(spec, o.n, rng, sparse_terms=CHAINS[name][2])
            b = np.stack([spec.dense(tm, o.n) for tm in terms])
            want = np.stack([o.multiply(a[row], b[row]) for row in range(3)])
            want.setflags(write=False)
            cache[name] = (o, spec, a, b, terms, marks, want)
        return cache[name]
    return get


def _diff(got, want):
    """{(component, position)} where any limb differs, and whether every limb differs there"""
    ne = np.asarray(got) != np.asarray(want)
    where = {(int(c), int(x)) for c, x in np.argwhere(ne.any(axis=1))}
    return where, all(ne[c, :, x].all() for c, x in where)


@pytest.mark.parametrize("name", list(CHAINS))
def test_model_equals_the_oracle_on_every_word(name, cases):
    o, spec, a, b, terms, marks, want = cases(name)
    if CHAINS[name][2]:
        assert len(terms[2][0]) == 5 and len(terms[2][1]) == 5  # a sparse second operand, not a monomial pair
    for row in range(3):
        assert np.array_equal(spec.multiply(a[row], terms[row]), want[row]), (name, row)
    # the product is symmetric in its operands: the crafted residues as b0 / b1
    assert np.array_equal(o.multiply(b[0], a[0]), want[0])
    assert np.array_equal(o.multiply(b[2], a[2]), want[2])


@pytest.mark.parametrize("name", list(CHAINS))
def test_zero_polynomials(name, cases):
    o, spec, a, b, terms, marks, want = cases(name)
    zero = np.zeros_like(a[1, 0])
    for which, parts in (("a0", (0,)), ("a1", (1,)), ("both", (0, 1))):
        az = a[1].copy()
        for p in parts:
            az[p] = zero
        got = o.multiply(az, b[1])
        assert np.array_equal(spec.multiply(az, terms[1]), got), (name, which)
        for comp in {"a0": (0,), "a1": (2,), "both": (0, 1, 2)}[which]:
            assert not got[comp].any(), (name, which, comp)  # E = 0


@pytest.mark.parametrize("name", list(CHAINS))
def test_builders_reach_what_they_claim(name, cases):
    o, spec, a, b, terms, marks, want = cases(name)
    L, q = spec.L, spec.q
    ext = spec.extend_summands()
    by_name = {c.name: c for c in ext}
    assert by_name["y: q-1 in every limb"].y == [p - 1 for p in q] and by_name["y: q-1 in every limb"].alpha == L - 1
    assert by_name["y: 0 in every limb"].y == [0] * L and by_name["y: 0 in every limb"].alpha == 0
    assert by_name["y: 0 in every limb"].res == [0] * L
    for e, label in enumerate(bs.EXTREME_NAMES):
        assert by_name["y: %s in every limb" % label].y == [bs.extremes(p)[e] for p in q]
    for c in ext:
        assert all(v in bs.extremes(p) for v, p in zip(c.y, q)) and all(0 <= v < p for v, p in zip(c.res, q))
        assert spec.extend(c.res)[1:] == (c.y, c.alpha, c.r)
    assert len({tuple(c.y) for c in ext}) >= 8  # mixed choices too, not one pattern ten times
    # the ties: every target, y_0 at both ends of its range
    ties = spec.r_ties()
    assert len(ties) == len(bs.R_TARGETS) * 3 * 2
    for i, c in enumerate(ties):
        target = bs.R_TARGETS[i // 6]
        assert c.r == target == spec.extend(c.res).r, c.name
        assert all(v in bs.extremes(p) for v, p in zip(c.y[1:], q[1:]))
        assert (c.y[0] < bs.M_TILDE) if i % 2 == 0 else (q[0] - bs.M_TILDE <= c.y[0] < q[0]), c.name
    assert {c.r for c in ties} == set(bs.R_TARGETS)
    assert max(c.alpha for c in ext + ties) == L - 1 and min(c.alpha for c in ext + ties) == 0
    # the floor summands: any integer with these residues has the claimed z and beta
    flo = spec.floor_summands()
    for c in flo:
        f = spec.floor(spec.crt(c.res) + 3 * spec.Q)
        assert f.z == c.z and f.beta == c.beta and all(v in bs.extremes(p) for v, p in zip(c.z, q)), c.name
    assert {c.beta for c in flo} >= {0, L - 1}
    assert [c.beta for c in flo if c.name == "z: q-1 in every limb"] == [L - 1]
    # ... and in the product itself: row 0 has b0 = 1, so component 0 at a crafted position floors with exactly these summands
    trace = {}
    at = sorted({x for row, poly, x, c in marks if row == 0 and poly == 0})
    spec.multiply_at(a[0], terms[0], at, trace=trace)
    seen = set()
    for row, poly, x, c in marks:
        if row == 0 and poly == 0:
            assert isinstance(c, bs.CraftedFloor) and trace[0, x].z == c.z and trace[0, x].beta == c.beta, (c.name, x)
            seen.add(c.name)
        else:
            assert isinstance(c, bs.Crafted) and [int(v) for v in a[row, poly, :, x]] == c.res
            seen.add(c.name)
    assert seen == {c.name for c in ext + ties + flo}  # every crafted coefficient is placed somewhere
    placed = {x for row, poly, x, c in marks}
    assert set(bs.kernel_positions(o.n)) <= placed


def test_kernel_positions_cover_blocks_and_position_groups():
    assert bs.kernel_positions(1024) == [0, 1023]
    assert bs.kernel_positions(4096) == [0, 1023, 1024, 2047, 2048, 3071, 3072, 4095]
    for logn in (13, 14, 15, 16):
        n, R = 1 << logn, logn - 10
        P = 512 >> R
        pos = set(bs.kernel_positions(n))
        assert {0, n - 1} <= pos and all({e - 1, e} <= pos for e in range(1024, n, 1024))
        groups = {(x >> 10, (x & 1023) // P, x % P) for x in pos}
        for kb in (0, (1 << R) - 1):
            for pg in (0, 1024 // P - 1):
                for p in (0, P - 1):
                    assert (kb, pg, p) in groups


@pytest.mark.parametrize("name", list(CHAINS))
def test_crafted_ties_discriminate(name, cases):
    """centring r = 2^31 the other way moves the product by t Y_b in every limb, at the coefficients the tie enters and nowhere else"""
    o, spec, a, b, terms, marks, want = cases(name)
    hits = bs.tie_outputs(o.n, terms, marks)
    assert not [h for h in hits if h[0] == 1] and {h[0] for h in hits} == {0, 2}
    for row in range(3):
        where, every_limb = _diff(spec.multiply(a[row], terms[row], tie_up=True), want[row])
        assert where == {(comp, x) for r_, comp, x in hits if r_ == row}, (name, row)
        assert every_limb
        assert (len(where) > 0) == (row != 1)


def test_decryption_oracle_against_exact_rounding(oracle_mod):
    n = 4096
    o = oracle_mod.Oracle.bfv_default(n)
    o.keygen(0xBE42)
    spec = bs.Behz(o.primes[:-1], o.t)
    gamma = int(oracle_mod.lib().orc_ctx_behz_prime(o.h, 1))
    assert gamma.bit_length() == 61 and gamma % (2 * n) == 1
    v, fam = spec.decrypt_phases(n, gamma, np.random.default_rng(42))
    assert {"special", "gamma", "boundary", "quarter", "random"} == set(fam)
    assert v[:5] == [0, 1, spec.Q - 1, spec.Q // 2, spec.Q // 2 + 1]
    ct = np.zeros((2, spec.L, n), dtype=np.uint64)
    ct[0] = spec.residues(v)
    got = o.decrypt(ct)
    pinned = [spec.decrypt_is_pinned(x) for x in v]
    for x, f, g, p in zip(v, fam, got, pinned):
        assert p or f in ("boundary", "gamma", "special"), f
        if p:
            assert int(g) == spec.decrypt(x), (f, x)
    assert all(p for p, f in zip(pinned, fam) if f in ("quarter", "random"))
    assert not any(p for p, f in zip(pinned, fam) if f == "boundary")
    assert pinned.count(False) < n // 4
    # size 3 with c1 = c2 = 0: the same phase
    ct3 = np.zeros((3, spec.L, n), dtype=np.uint64)
    ct3[0] = ct[0]
    assert np.array_equal(o.decrypt(ct3), got)
