"""Divide by a dropped prime with rounding -- the key switch's mod-down and CKKS rescale -- word for word against the CPU oracle, on
the shapes the other files leave out (abc_ntt.hpp, "divide by a dropped prime"; the kernels are k_fused_ks_special_intt /
k_fused_ks_moddown / k_fused_ks_moddown_bfv and their _fp twins, k_rescale_intt_fp / _mixed, k_rescale_ntt and the generic pair
k_divround_tmod / k_divround_finish):

  * N = 2^11 and 2^13: the block lengths whose pass schedules (4+3+2+2, 4+4+3+2) no other LDS-resident test runs;
  * batches of 5 ciphertexts: 10 (ciphertext, component) polynomials, 15 for a size-3 rescale -- one full group of eight workgroup
    slots per L2 slice followed by a ragged one (xcd_slot, abc_context.hpp; k_fused_ks_moddown_fp);
  * every integer form of the arithmetic policy (lazy, unguarded, guarded) next to fp64, and rescale's per-prime mix of the two;
  * the rounding boundary itself: a dropped limb built in coefficient form from 0, 1, (p-3)/2, (p-1)/2, (p+1)/2, p-2, p-1, so
    that + floor(p/2) wraps or does not, and the fix lands on both sides.

Inputs are residues, not encryptions: every limb drawn from {0, 1, q-1, q-2, floor(q/2), floor(q/2)+1}.  One row of each batch is
compared with the single-ciphertext result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# bit sizes, special prime last -> (key-switch route, {nl: rescale route})
CKKS_CHAINS = {
    # level 3 drops a 45-bit prime between a 40-bit and a 50-bit one, level 2 a 50-bit prime under a 40-bit one: the largest
    # unreduced operand the fp64 forward transform is asked to absorb
    "fp_40_50_45_49": ([40, 50, 45, 49, 50], "lds_fp", {4: "fp", 3: "fp", 2: "fp"}),
    "lazy_52_40_55": ([52, 40, 55, 54], "lds_int guard=0 lazy=1", {3: "mixed fpmask=0x2", 2: "mixed fpmask=0x2"}),
    "unguarded_57_40_56": ([57, 40, 56, 57], "lds_int guard=0 lazy=0", {3: "mixed fpmask=0x2", 2: "mixed fpmask=0x2"}),
    "guarded_60_40_58": ([60, 40, 58, 60], "lds_int guard=1 lazy=0", {3: "mixed fpmask=0x2", 2: "mixed fpmask=0x2"}),
}
BFV_CHAINS = {
    "fp_40_45": ([40, 45, 50], "lds_fp"),
    "guarded_58_52": ([58, 52, 60], "lds_int guard=1 lazy=0"),
}
RINGS = (2048, 8192)
BATCH = 5


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ; first at %s got %d want %d" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _edge(rng, primes, nl, size, n):
    """[size][nl][N], every limb from the ends and the middle of its range"""
    ct = np.empty((size, nl, n), dtype=np.uint64)
    for j, q in enumerate(primes[:nl]):
        ct[:, j, :] = rng.choice(np.array([0, 1, q - 1, q - 2, q // 2, q // 2 + 1], dtype=np.uint64), size=(size, n))
    return ct


def _boundary(rng, o, primes, nl, size, n):
    """_edge with the limb a rescale drops (nl - 1) built in COEFFICIENT form around the rounding boundary"""
    ct = _edge(rng, primes, nl, size, n)
    p = primes[nl - 1]
    vals = np.array([0, 1, (p - 3) // 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1], dtype=np.uint64)
    for s in range(size):
        coef = rng.choice(vals, size=n)
        coef[:len(vals)] = vals  # each of them at least once
        ct[s, nl - 1, :] = o.ntt(nl - 1, coef)
    return ct


def _pair(oracle_mod, capi, scheme, n, bits, seed, t=0):
    primes = oracle_mod.create_primes(n, bits)
    o = oracle_mod.Oracle(scheme, n, primes, t)
    elt = o.elt_from_step(1)
    o.keygen(seed, elts=[elt])
    g = capi.Context(scheme, n, primes, t)
    g.load_keys(sk=o.secret_key(), pk=o.public_key(), relin=o.relin_key(), galois={elt: o.galois_key(elt)})
    return o, g, primes


def _batch(single, other, row):
    """BATCH rows, `single` at `row` and `other` everywhere else"""
    return np.stack([single if i == row else other for i in range(BATCH)])


def oracle_ckks_level(o, rng, primes, nl, n):
    """inputs and the oracle's results at one level; runs without a GPU"""
    x, y, z = _edge(rng, primes, nl, 2, n), _edge(rng, primes, nl, 2, n), _edge(rng, primes, nl, 3, n)
    d = dict(x=x, y=y, z=z, mul=o.mul_relin(x, y), rot=o.rotate(x, 1), relin=o.relinearize(z))
    if nl >= 2:
        d["bx"], d["bz"] = _boundary(rng, o, primes, nl, 2, n), _boundary(rng, o, primes, nl, 3, n)
        for k in ("x", "z", "bx", "bz"):
            d["rescale_" + k] = o.rescale(d[k])
    return d


@pytest.mark.parametrize("n", RINGS)
@pytest.mark.parametrize("chain", list(CKKS_CHAINS))
def test_ckks_key_switch_and_rescale_at_every_level(chain, n, oracle_mod, capi):
    bits, ks_route, rescale_routes = CKKS_CHAINS[chain]
    o, g, primes = _pair(oracle_mod, capi, oracle_mod.CKKS, n, bits, 0xD1400 + n)
    rng = np.random.default_rng(n + len(chain))
    for nl in range(len(bits) - 1, 0, -1):
        tag = "%s N=%d nl=%d" % (chain, n, nl)
        for count in (1, BATCH):
            assert g.route("mul_relin", nl, count) == ks_route, (tag, count)
            assert g.route("relinearize", nl, count) == ks_route, (tag, count)
            assert g.route("rotate", nl, count) == "permute " + ks_route, (tag, count)
            if nl >= 2:
                assert g.route("rescale", nl, count) == rescale_routes[nl], (tag, count)
        d = oracle_ckks_level(o, rng, primes, nl, n)
        x, y, z = d["x"], d["y"], d["z"]
        _same(tag + " mul_relin", g.mul_relin(x, y), d["mul"])
        _same(tag + " mul_relin, row 3 of 5", g.mul_relin(_batch(x, y, 3), _batch(y, y, 3))[3], d["mul"])
        _same(tag + " rotate 1", g.rotate(x, 1), d["rot"])
        _same(tag + " rotate 1, row 4 of 5", g.rotate(_batch(x, y, 4), 1)[4], d["rot"])
        _same(tag + " relinearize", g.relinearize(z), d["relin"])
        _same(tag + " relinearize, row 0 of 5", g.relinearize(_batch(z, z[::-1].copy(), 0))[0], d["relin"])
        if nl < 2:
            continue
        for k, other in (("x", y), ("z", z[::-1].copy()), ("bx", x), ("bz", z)):
            _same(tag + " rescale " + k, g.rescale(d[k]), d["rescale_" + k])
            _same(tag + " rescale %s, row 2 of 5" % k, g.rescale(_batch(d[k], other, 2))[2], d["rescale_" + k])
    g.close()


def oracle_bfv(oracle_mod, o, rng, primes, n):
    a = o.encrypt(o.encode(oracle_mod.expand_vector([3, 1, 4, 1, 5, 9, 2, 6], n)), 1)
    b = o.encrypt(o.encode(oracle_mod.expand_vector([2, 7, 1, 8, 2, 8, 1, 8], n)), 2)
    ex = _edge(rng, primes, len(primes) - 1, 2, n)
    return dict(a=a, b=b, ex=ex, mul=o.mul_relin(a, b), mul_ex=o.mul_relin(ex, a), rot=o.rotate(ex, 1), rot_a=o.rotate(a, 1))


@pytest.mark.parametrize("chain", list(BFV_CHAINS))
def test_bfv_mod_down_in_coefficient_form(chain, oracle_mod, capi):
    n = 2048
    bits, ks_route = BFV_CHAINS[chain]
    o, g, primes = _pair(oracle_mod, capi, oracle_mod.BFV, n, bits, 0xD1500, oracle_mod.plain_modulus_batching(n, 20))
    L = len(bits) - 1
    for count in (1, BATCH):
        assert g.route("mul_relin", L, count) == "generic mul=behz ks=" + ks_route, (chain, count)
        assert g.route("rotate", L, count) == "permute " + ks_route, (chain, count)
    d = oracle_bfv(oracle_mod, o, np.random.default_rng(7), primes, n)
    a, b, ex = d["a"], d["b"], d["ex"]
    _same(chain + " mul_relin", g.mul_relin(a, b), d["mul"])
    _same(chain + " mul_relin, end-of-range residues", g.mul_relin(ex, a), d["mul_ex"])
    _same(chain + " mul_relin, row 1 of 5", g.mul_relin(_batch(ex, a, 1), _batch(a, b, 1))[1], d["mul_ex"])
    _same(chain + " rotate 1, end-of-range residues", g.rotate(ex, 1), d["rot"])
    _same(chain + " rotate 1, row 3 of 5", g.rotate(_batch(a, ex, 3), 1)[3], d["rot_a"])
    g.close()


def test_generic_pair_on_the_rounding_boundary(oracle_mod, capi, monkeypatch):
    """rescale through k_divround_tmod / k_divround_finish around the stand-alone transforms (ABC_HIP_NO_FUSED=1)"""
    monkeypatch.setenv("ABC_HIP_NO_FUSED", "1")
    n, (bits, _, _) = 2048, CKKS_CHAINS["lazy_52_40_55"]
    o, g, primes = _pair(oracle_mod, capi, oracle_mod.CKKS, n, bits, 0xD1600)
    rng = np.random.default_rng(11)
    for nl in (3, 2):
        assert g.route("rescale", nl, BATCH) == "generic"
        for size in (2, 3):
            ct, other = _boundary(rng, o, primes, nl, size, n), _edge(rng, primes, nl, size, n)
            want = o.rescale(ct)
            _same("generic rescale nl=%d size=%d" % (nl, size), g.rescale(ct), want)
            _same("generic rescale nl=%d size=%d, row 4 of 5" % (nl, size), g.rescale(_batch(ct, other, 4))[4], want)
    g.close()
