"""Direct parity of the stand-alone transforms (abc_hip_ntt_forward / _inverse / _limbs, abc_kernels_ntt.hip) with the CPU oracle,
bit for bit, at every ring size N = 2^10 .. 2^16 and every prime width whose code path differs.

One CKKS context per ring on the chain [50, 49, 48, 44, 40, 36, 58, 50] bits (no keys): 50 and 49 bits take FpK::red, 50 bits also
FpTail's threshold; 48 / 44 are pack kind 2, 40 / 36 pack kind 1; 58 bits is an integer limb inside the same context.  (Every
ring accepts the whole chain, so it is not shortened anywhere.)  The rows of a call are zeros, an impulse 1 at index 0, an
impulse q - 1 at index N - 1, the input families of the CPU model (tests/test_fp64_exactness_single_twiddle.py, _inputs: all
q - 1, runs of q - 1 / (q + 1)/2 / 0 / (q - 1)/2, random, alternating, halves) and a second random row: nine rows.  The inverse is
checked on Oracle.ntt of these rows AND on the rows themselves (any vector of residues is a valid NTT-form input), against
Oracle.intt, not only as a round trip.

What these tests can catch: a wrong twiddle index in some block of some LB / S0, a wrong limb-to-prime mapping, a load or store
index slip, the few-limb / whole-block switch at N = 2^14, canonicalisation (fp_to_canon, fp_from_u64, the N^-1 scaling) at the
ends of the range, modulus kind 2 (the plaintext modulus).

What they cannot catch, measured so that nobody tries a third time: a dropped or misplaced re-centring in a ten-stage tail.
On the CPU (n = 1024, the largest 50-bit prime = 1 mod 2^17, ten forward stages with NO re-centring at all, centred inputs), the
peak magnitude after ten stages, of the 8 q that 2^53 allows, was
    all +q/2, alternating                                                        3.34 q
    random                                                                       2.93 q
    greedy backward construction (3000 tries per node), every butterfly of one
    path aligned and the quotient-estimate error exploited                       5.94 q
so no input that can be constructed changes an output word when a re-centring goes missing; guarding the schedule is the job of
the bound recurrence in the CPU model.  No kernel instrumentation, no magnitude read-back here.
"""
import numpy as np
import pytest

import test_fp64_exactness_single_twiddle as model

pytestmark = pytest.mark.gpu

BITS = [50, 49, 48, 44, 40, 36, 58, 50]
NFP = 6      # the first six primes are below 2^50: a prefix of at most NFP limbs is one fp64 launch
_DATA = {}   # logn -> oracle-side inputs and expected outputs, computed once and never modified


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d/%d words differ, first at %s: got %d want %d" % (
            name, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _rows(n, q, rng):
    fam = model._inputs(n, q, "canonical", rng, few=False)
    rows = np.zeros((9, n), dtype=np.uint64)
    rows[1, 0] = 1
    rows[2, n - 1] = q - 1
    for r, key in enumerate(("all top", "runs", "alternating", "halves", "random")):
        rows[3 + r] = np.array(fam[key], dtype=np.uint64)
    rows[8] = rng.integers(0, q, size=n, dtype=np.uint64)
    return rows


class Ring:
    def __init__(self, om, logn):
        self.logn, self.n = logn, 1 << logn
        self.primes = om.create_primes(self.n, BITS)
        assert [p.bit_length() for p in self.primes] == BITS
        o = om.Oracle(om.CKKS, self.n, self.primes)
        rng = np.random.default_rng(1000 + logn)
        self.raw = [_rows(self.n, q, rng) for q in self.primes]                        # [prime][row][N]
        self.fwd = [np.stack([o.ntt(j, r) for r in x]) for j, x in enumerate(self.raw)]
        # inverse inputs: the forward images, then the raw rows themselves
        self.inv_in = [np.concatenate([f, x]) for f, x in zip(self.fwd, self.raw)]
        self.inv = [np.stack([o.intt(j, r) for r in x]) for j, x in enumerate(self.inv_in)]
        for j in range(len(self.primes)):  # the oracle against itself, so that a mistake in it cannot hide in the round trip
            assert np.array_equal(self.inv[j][:9], self.raw[j])

    def poly(self, src, nl, rows):
        """[len(rows)][nl][N]: polynomial p carries row rows[p] of every prime's set"""
        return np.stack([np.stack([src[j][r] for j in range(nl)]) for r in rows])


def _data(om, logn):
    if logn not in _DATA:
        _DATA[logn] = Ring(om, logn)
    return _DATA[logn]


@pytest.fixture(scope="module", params=range(10, 17), ids=lambda l: "N=2^%d" % l)
def ring(request, oracle_mod, capi):
    d = _data(oracle_mod, request.param)
    assert capi.create_primes(d.n, BITS) == d.primes
    g = capi.Context(capi.CKKS, d.n, d.primes)
    yield d, g
    g.close()


def _check_every_prime(tag, d, g):
    for j in range(len(d.primes)):
        _same("%s N=2^%d fwd prime %d (%d bits)" % (tag, d.logn, j, BITS[j]), g.ntt(d.raw[j], 0, j), d.fwd[j])
        _same("%s N=2^%d inv prime %d (%d bits)" % (tag, d.logn, j, BITS[j]), g.ntt(d.inv_in[j], 0, j, inverse=True), d.inv[j])


def test_every_prime_forward_and_inverse(ring):
    """nine (forward) / eighteen (inverse) limbs of ONE prime per call: whole blocks for N <= 2^13, the few-limb form at N = 2^14,
    strided + 4096-point blocks above; the 58-bit prime takes the integer kernels of the same launch code"""
    _check_every_prime("ntt", *ring)


def test_limb_launches_with_a_different_prime_per_limb(ring):
    """ntt_limbs at nl = 1 .. L with three polynomials: prefixes of fp64 primes are one fp64 launch with another prime per limb
    (the limb-to-prime mapping of every fp64 kernel), prefixes with the 58-bit prime switch the whole launch to integers"""
    d, g = ring
    rows = [3, 4, 8]  # all q - 1, runs, random
    first_f, first_i = None, None
    for nl in range(1, g.L + 1):
        f = g.ntt_limbs(d.poly(d.raw, nl, rows), inverse=False)
        _same("ntt_limbs N=2^%d fwd nl=%d" % (d.logn, nl), f, d.poly(d.fwd, nl, rows))
        inv_rows = [9 + r for r in rows]  # independent data: the raw rows as NTT-form input
        i = g.ntt_limbs(d.poly(d.inv_in, nl, inv_rows), inverse=True)
        _same("ntt_limbs N=2^%d inv nl=%d" % (d.logn, nl), i, d.poly(d.inv, nl, inv_rows))
        if nl == 1:
            first_f, first_i = f[:, 0].copy(), i[:, 0].copy()
        assert np.array_equal(f[:, 0], first_f) and np.array_equal(i[:, 0], first_i), "limb 0 differs at nl=%d" % nl
    assert g.L == 7 and NFP < g.L  # nl = 7 includes the 58-bit prime


def _both_shapes14(tag, d, g):
    """the rows as 8 polynomials of six fp64 limbs (48 limbs in flight) and as 9 (54 limbs)"""
    out = {}
    for polys in (8, 9):
        rows = list(range(polys))
        f = g.ntt_limbs(d.poly(d.raw, NFP, rows))
        _same("%s fwd %d limbs" % (tag, polys * NFP), f, d.poly(d.fwd, NFP, rows))
        inv_rows = [9 + r for r in rows]
        i = g.ntt_limbs(d.poly(d.inv_in, NFP, inv_rows), inverse=True)
        _same("%s inv %d limbs" % (tag, polys * NFP), i, d.poly(d.inv, NFP, inv_rows))
        i2 = g.ntt_limbs(d.poly(d.inv_in, NFP, rows), inverse=True)
        _same("%s inv of the forward images, %d limbs" % (tag, polys * NFP), i2, d.poly(d.raw, NFP, rows))
        out[polys] = (f, i)
    assert np.array_equal(out[8][0], out[9][0][:8]) and np.array_equal(out[8][1], out[9][1][:8])
    return out[9]


def test_n14_strided_plus_blocks_and_whole_block_launches(oracle_mod, capi, monkeypatch):
    """N = 2^14: at most 48 limbs in flight take the strided radix-16 pass + 1024-point blocks, more take k_ntt_*_fp<14> as whole
    blocks.  ABC_HIP_FEW_LIMBS (read when the context is created) moves the switch: 0 = always whole blocks, a large value =
    always strided + blocks.  Every run equals the oracle, and so one another."""
    d = _data(oracle_mod, 14)
    res = []
    for few in (None, "0", "100000"):
        if few is None:
            monkeypatch.delenv("ABC_HIP_FEW_LIMBS", raising=False)
        else:
            monkeypatch.setenv("ABC_HIP_FEW_LIMBS", few)
        g = capi.Context(capi.CKKS, d.n, d.primes)
        tag = "N=2^14 FEW_LIMBS=%s" % few
        res.append(_both_shapes14(tag, d, g))
        _check_every_prime(tag, d, g)  # 9 / 18 limbs of one prime: few-limb form by default, whole blocks with 0
        g.close()
    for r in res[1:]:
        assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1])


@pytest.mark.parametrize("logn", [13, 14, 16])
def test_integer_kernels_give_the_same_words(logn, oracle_mod, capi, monkeypatch):
    """ABC_HIP_NO_FP64=1: the same rows through the integer kernels of every launch shape"""
    d = _data(oracle_mod, logn)
    monkeypatch.setenv("ABC_HIP_NO_FP64", "1")
    g = capi.Context(capi.CKKS, d.n, d.primes)
    _check_every_prime("NO_FP64", d, g)
    rows = [3, 4, 8]
    _same("NO_FP64 ntt_limbs fwd", g.ntt_limbs(d.poly(d.raw, NFP, rows)), d.poly(d.fwd, NFP, rows))
    inv_rows = [9 + r for r in rows]
    _same("NO_FP64 ntt_limbs inv", g.ntt_limbs(d.poly(d.inv_in, NFP, inv_rows), inverse=True), d.poly(d.inv, NFP, inv_rows))
    if logn == 14:
        _both_shapes14("NO_FP64 N=2^14", d, g)
    g.close()


# ---- modulus kind 2: the plaintext modulus (a prime of about 20 bits, on the fp64 path) --------------------------------------
def _negacyclic(x, q, inverse):
    """plain negacyclic transform of the rows of x modulo q in the oracle's convention: minimal primitive 2N-th root, forward =
    Cooley-Tukey natural in -> bit-reversed out, inverse = Gentleman-Sande + N^-1.  The same code on Python integers (object arrays:
    the key prime that pins it against the oracle) and, where every product fits, on 64-bit words (the plaintext modulus)."""
    dt = object if q >= 1 << 31 else np.uint64
    x = np.array(x, dtype=dt) % q
    rows, n = x.shape
    logn = n.bit_length() - 1
    psi = model._min_root(2 * n, q)
    tw, p = [0] * n, 1
    for i in range(n):
        tw[model._bitrev(i, logn)] = p
        p = p * psi % q
    if inverse:
        tw = [pow(w, q - 2, q) for w in tw]
    tw = np.array(tw, dtype=dt)
    inv_n = pow(n, q - 2, q)
    if dt is not object:
        q, inv_n = np.uint64(q), np.uint64(inv_n)
    for s in (range(logn - 1, -1, -1) if inverse else range(logn)):
        blocks, half = 1 << s, n >> (s + 1)
        v = x.reshape(rows, blocks, 2, half)
        w = tw[blocks:2 * blocks].reshape(1, blocks, 1)
        a, c = v[:, :, 0, :], v[:, :, 1, :]
        if inverse:
            v = np.stack([(a + c) % q, (a + q - c) * w % q], axis=2)
        else:
            t = c * w % q
            v = np.stack([(a + t) % q, (a + q - t) % q], axis=2)
        x = v.reshape(rows, n)
    if inverse:
        x = x * inv_n % q
    return x.astype(np.uint64)


@pytest.mark.parametrize("n", [4096, 16384])
def test_plain_modulus_transforms(n, oracle_mod, capi):
    o = oracle_mod.Oracle.bfv_default(n)
    g = capi.Context.bfv_default(n)
    assert g.t == o.t and g.t.bit_length() <= 21
    rng = np.random.default_rng(n)
    # pin the reference on a key prime, where the oracle has a transform
    q0 = o.primes[0]
    x0 = rng.integers(0, q0, size=(1, n), dtype=np.uint64)
    f0 = o.ntt(0, x0[0])
    assert np.array_equal(_negacyclic(x0, q0, False)[0], f0)
    assert np.array_equal(_negacyclic(x0, q0, True)[0], o.intt(0, x0[0]))
    t = g.t
    rows = _rows(n, t, rng)
    want_f = _negacyclic(rows, t, False)
    _same("kind 2 fwd N=%d" % n, g.ntt(rows, 2, 0), want_f)
    inv_in = np.concatenate([want_f, rows])
    want_i = _negacyclic(inv_in, t, True)
    assert np.array_equal(want_i[:9], rows)
    _same("kind 2 inv N=%d" % n, g.ntt(inv_in, 2, 0, inverse=True), want_i)
    g.close()


def test_bad_arguments_are_errors_and_leave_the_context_usable(ring, capi):
    import ctypes
    d, g = ring
    x = d.raw[0][:2]
    for kind, index in ((3, 0), (-1, 0), (0, g.K), (0, -1), (2, 0), (1, 0)):  # kinds 1 and 2 exist in a BFV context only
        for inverse in (False, True):
            with pytest.raises(capi.AbcHipError):
                g.ntt(x, kind, index, inverse=inverse)
    buf = g.upload(np.zeros((g.K, d.n), dtype=np.uint64))
    for nl in (0, -1, g.L + 1):  # the special prime is no data level
        for inverse in (0, 1):
            with pytest.raises(capi.AbcHipError):
                g.op("ntt_limbs", buf.ptr, nl, ctypes.c_size_t(1), inverse)
    buf.free()
    _same("after the errors, fwd", g.ntt(x, 0, 0), d.fwd[0][:2])
    _same("after the errors, inv", g.ntt(d.inv_in[1][9:11], 0, 1, inverse=True), d.inv[1][9:11])
