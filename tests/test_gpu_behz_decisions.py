"""BFV multiply and decryption at their integer decision points, on every implementation of them.

BEHZ uses a residue as an integer in a few places: the canonical summands of the two base conversions out of q, r = [-X q^-1] mod
2^32 and its centring at 2^31, the overflow counts of the conversions, the sign of the Shenoy-Kumaresan correction, the rounding of
decryption.  None of them sees a raw input residue -- each sees it times a constant, uniform again -- so random and end-of-range
inputs reach r = 2^31 once in 2^32 coefficients and "every summand at q_i - 1" never.  tests/behz_spec.py builds the coefficients
that do, and states the multiply as one big integer, independent of the oracle's RNS code;
tests/test_behz_spec.py shows on the CPU that the model equals the oracle and that these inputs tell a wrong tie apart.

Here a batch of three ciphertexts, the crafted rows at 0 and 2, goes through each implementation: the route string first, then
`multiply` word for word against the oracle, against the model at every coefficient a crafted one enters plus 256 sampled ones,
the same with the operands swapped (the crafted residues as b0 / b1), zero polynomials, and `mul_relin` against the oracle.
Every comparison is equality of uint64 words.
"""
import numpy as np
import pytest

import behz_spec as bs

pytestmark = pytest.mark.gpu

_B14 = "bsplit14 pass0=per_target"
CHAINS = {  # name: (N, key-prime widths; None: BFVDefault(N))
    "BFVDefault4096": (1 << 12, None),
    "BFVDefault8192": (1 << 13, None),
    "BFVDefault16384": (1 << 14, None),
    "N32768-49x8": (1 << 15, [49] * 8 + [50]),
    "N65536-49x8": (1 << 16, [49] * 8 + [50]),
    "N8192-50x10": (1 << 13, [50] * 11),   # ten data primes: the most the fp64 base conversions accept
    "N8192-50x11": (1 << 13, [50] * 12),
    "N4096-58-52-60": (1 << 12, [58, 52, 60]),
}
CASES = {  # id: (chain, switches, route of mul_relin, route of multiply) -- and, in the comment, the kernels that decide
    # k_behz_extend_fp<2, 2> / k_behz_floor_fp<2, 2>
    "N4096": ("BFVDefault4096", {}, "generic mul=behz ks=lds_fp", "behz"),
    # k_behz_extend<2, 2> / k_behz_floor<2, 2>, 50-bit auxiliary base
    "N4096-int-kernels": ("BFVDefault4096", {"ABC_HIP_BEHZ_INT_KERNELS": "1"}, "generic mul=behz ks=lds_fp", "behz"),
    # the same kernels on SEAL's 61-bit base: the flush path of dot_shoup_lazy
    "N4096-seal-base": ("BFVDefault4096", {"ABC_HIP_BEHZ_SEAL_BASE": "1"}, "generic mul=behz ks=lds_fp", "behz"),
    # k_bmul_front / k_bmul_back<13, 3, 4, 4>: multiply through bmul_big (want3 = 1), mul_relin through bmul_split (want3 = 0)
    "N8192": ("BFVDefault8192", {}, "bmul", "bmul_big"),
    # k_behz_extend_fp<4, 4> / k_behz_floor_fp<4, 4>
    "N8192-no-bmul": ("BFVDefault8192", {"ABC_HIP_NO_BMUL": "1"}, "generic mul=behz ks=bsplit_big", "behz"),
    # k_bmul_front / k_bmul_back<14, 4, 8, 8>: mul_relin takes the want3 = 0 form of the back kernel (component 2 stays in LDS for
    # the key switch), multiply the want3 = 1 form
    "N16384": ("BFVDefault16384", {}, "bmul", "bmul"),
    # k_behz_extend_fp<8, 8> / k_behz_floor_fp<8, 8>
    "N16384-no-bmul": ("BFVDefault16384", {"ABC_HIP_NO_BMUL": "1"}, "generic mul=behz ks=" + _B14, "behz"),
    # k_bmul_front / k_bmul_back<15, 5, 8, 8, 576> and <16, 6, 8, 8, 576>: nine wavefronts, the workgroup-id remap of R > 4
    "N32768": ("N32768-49x8", {}, "generic mul=bmul_big ks=bsplit_big", "bmul_big"),
    "N65536": ("N65536-49x8", {}, "generic mul=bmul_big ks=bsplit_big", "bmul_big"),
    # k_behz_extend_fp<0, 0> / k_behz_floor_fp<0, 0> at their largest L: 'q-1 in every limb' is the largest sum they add up
    "N8192-50x10": ("N8192-50x10", {}, "generic mul=behz ks=lds_fp", "behz"),
    # k_behz_extend<0, 0> / k_behz_floor<0, 0>, 50-bit auxiliary base
    "N8192-50x11": ("N8192-50x11", {}, "generic mul=behz ks=lds_fp", "behz"),
    # integer kernels on SEAL's base under a chain that has no other
    "N4096-58-52-60": ("N4096-58-52-60", {}, "generic mul=behz ks=lds_int guard=1 lazy=0", "behz"),
}
SAMPLED = 256


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, name
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s: got %d want %d" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


class _Chain:
    """one oracle with a relinearisation key, the crafted batch, and everything expected of it -- computed once, read-only"""

    def __init__(self, om, name):
        self.n, bits = CHAINS[name]
        if bits is None:
            self.o = om.Oracle.bfv_default(self.n)
        else:
            self.o = om.Oracle(om.BFV, self.n, om.create_primes(self.n, bits), om.plain_modulus_batching(self.n, 20))
        o, n = self.o, self.n
        o.keygen(0xBE42 + n, elts=[])
        self.spec = spec = bs.Behz(o.primes[:-1], o.t)
        rng = np.random.default_rng(n + len(o.primes))
        self.a, self.terms, self.marks = bs.crafted_batch(spec, n, rng)
        self.b = np.stack([spec.dense(tm, n) for tm in self.terms])
        self.want = np.stack([o.multiply(self.a[row], self.b[row]) for row in range(3)])
        self.want_relin = np.stack([o.relinearize(w) for w in self.want])
        # the model: every product coefficient that a crafted coefficient enters, and sampled ones
        self.model = {}
        for row in (0, 2):
            pos = set(int(x) for x in rng.choice(n, size=SAMPLED, replace=False))
            for r_, poly, x, c in self.marks:
                if r_ == row:
                    pos.add(x)
                    pos.update((x + k) % n for s in (0, 1) for k, _ in self.terms[row][s])
            pos = sorted(pos)
            self.model[row] = (pos, spec.multiply_at(self.a[row], self.terms[row], pos))
        # zero polynomials as a0, as a1, as both, against row 1's monomials
        self.az = np.stack([self.a[1]] * 3)
        self.az[0, 0] = 0
        self.az[1, 1] = 0
        self.az[2] = 0
        self.zpos = sorted(int(x) for x in rng.choice(n, size=SAMPLED, replace=False))
        self.zmodel = [spec.multiply_at(self.az[i], self.terms[1], self.zpos) for i in range(3)]
        self.zwant = np.stack([o.multiply(self.az[i], self.b[1]) for i in range(3)]) if n <= 1 << 14 else None
        for arr in (self.a, self.b, self.want, self.want_relin, self.az):
            arr.setflags(write=False)


@pytest.fixture(scope="module")
def chains(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()  # the cases of one chain are neighbours: one chain's arrays at a time
            cache[name] = _Chain(oracle_mod, name)
        return cache[name]
    yield get
    cache.clear()


def test_the_model_agrees_with_the_oracle_on_these_inputs(chains):
    """no GPU work: the expectation itself, on the smallest chain (tests/test_behz_spec.py does this on every word)"""
    ch = chains("BFVDefault4096")
    for row in (0, 2):
        pos, want = ch.model[row]
        _same("model row %d" % row, want, ch.want[row][:, :, pos])
    hits = bs.tie_outputs(ch.n, ch.terms, ch.marks)
    assert hits and all((x in ch.model[row][0]) for row, comp, x in hits)  # the coefficients that tell a wrong tie apart are checked


@pytest.mark.parametrize("case", list(CASES))
def test_multiply_at_the_decision_points(case, chains, capi, monkeypatch):
    name, env, route_mul_relin, route_multiply = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the context is created
    ch = chains(name)
    o, L = ch.o, ch.spec.L
    g = capi.Context(capi.BFV, o.n, o.primes, o.t)
    try:
        g.load_keys(relin=o.relin_key())
        for count in (1, 3):
            assert g.route("multiply", L, count) == route_multiply, (case, count)
            assert g.route("mul_relin", L, count) == route_mul_relin, (case, count)
        for swapped in (False, True):
            tag = case + (" swapped" if swapped else "")
            x, y = (ch.b, ch.a) if swapped else (ch.a, ch.b)
            got = g.multiply(x, y)
            for row in range(3):
                _same("%s multiply row %d against the oracle" % (tag, row), got[row], ch.want[row])
            for row in (0, 2):
                pos, want = ch.model[row]
                _same("%s multiply row %d against the model" % (tag, row), got[row][:, :, pos], want)
            got = g.mul_relin(x, y)
            for row in range(3):
                _same("%s mul_relin row %d" % (tag, row), got[row], ch.want_relin[row])
        got = g.multiply(ch.az, np.stack([ch.b[1]] * 3))
        for i, (which, zero) in enumerate((("a0 = 0", (0,)), ("a1 = 0", (2,)), ("a = 0", (0, 1, 2)))):
            _same("%s %s against the model" % (case, which), got[i][:, :, ch.zpos], ch.zmodel[i])
            for comp in zero:
                assert not got[i, comp].any(), (case, which, comp)
            if ch.zwant is not None:
                _same("%s %s against the oracle" % (case, which), got[i], ch.zwant[i])
    finally:
        g.close()


DECRYPT_CHAINS = {"BFVDefault4096": (1 << 12, None), "BFVDefault16384": (1 << 14, None), "N32768-55x8-56": (1 << 15, [55] * 8 + [56])}


@pytest.mark.parametrize("name", list(DECRYPT_CHAINS))
def test_decrypt_at_the_rounding_boundaries(name, oracle_mod, capi):
    """k_bfv_decrypt_round on phases real encryptions never have: at and next to a rounding boundary, 0 / 1 / Q-1 / Q/2, the summands
    of its base conversion at the ends of their range, a quarter step from a boundary.  The phase is c0 (c1 = 0, and c2 = 0)."""
    om = oracle_mod
    n, bits = DECRYPT_CHAINS[name]
    o = om.Oracle.bfv_default(n) if bits is None else om.Oracle(om.BFV, n, om.create_primes(n, bits), om.plain_modulus_batching(n, 20))
    o.keygen(0xDEC + n, elts=[])
    spec = bs.Behz(o.primes[:-1], o.t)
    gamma = int(om.lib().orc_ctx_behz_prime(o.h, 1))
    rng = np.random.default_rng(n)
    g = capi.Context(capi.BFV, n, o.primes, o.t)
    try:
        g.load_keys(sk=o.secret_key())
        for size in (2, 3):
            cts = np.zeros((2, size, spec.L, n), dtype=np.uint64)
            phases = [spec.decrypt_phases(n, gamma, rng) for _ in range(2)]
            for i, (v, fam) in enumerate(phases):
                cts[i, 0] = spec.residues(v)
            got = g.decrypt(cts)
            for i, (v, fam) in enumerate(phases):
                _same("%s size %d decrypt [%d] against the oracle" % (name, size, i), got[i], o.decrypt(cts[i]))
                pinned = [spec.decrypt_is_pinned(x) for x in v]
                assert pinned.count(False) < n // 4
                for x, f, m, p in zip(v, fam, got[i], pinned):
                    if p:
                        assert int(m) == spec.decrypt(x), (name, size, f, x)
    finally:
        g.close()
