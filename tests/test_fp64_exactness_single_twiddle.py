"""CPU model of the fp64 butterflies with ONE double per twiddle (abc_amd/csrc/abc_ntt.hpp: fp_mul_tw, FpArith, FpTail).

The quotient of a twiddle product is estimated from the product itself, c = rint(fl(fl(y w) * fl(1/q))), so the table keeps
only w.  Three roundings instead of two: one stage grows a bound Y on |value| to Y (1 + 1.5 q 2^-53) + q/2 (it was
Y (1 + q 2^-53) + q/2 with a stored w/q).  The estimate only chooses WHICH representative comes out; everything else is exact
as long as magnitudes stay below 2^53.  This file replays, with Python integers for the exact parts and IEEE doubles for the
estimate, every stage schedule the kernels are compiled with:

  * whole forward and inverse block transforms of 10 .. 14 stages (ntt_fwd_block_a<LB> / ntt_inv_block_a<LB>, FpArith, Sched<LB>);
  * the stand-alone launches of abc_kernels_ntt.hip that are not one block: the few-limb N = 2^14 form (k_ntt_fwd_strided_fp<4>: four
    raw stages from a canonical input, then k_ntt_fwd_fp<10> with a re-centred load; inverse k_ntt_inv_fp<10>, then
    k_ntt_inv_strided_fp<4> with a re-centred load) and the N = 2^15 / 2^16 forms (three / four strided stages around 4096-point
    blocks), each to its very end: fp_to_canon in the forward store; fp_mul_lazy by N^-1 with its stored fl(w/q), then fp_to_canon,
    in the inverse one;
  * the N = 2^14 split forms: a radix-16 register pass from a canonical residue, from a residue of ANOTHER (50-bit) prime or
    from a sum of two residues (k_split3_pass_fp: t + fix), then the ten-stage tail from re-centred values -- FpTail's 3 + 4 + 3
    (k_split4_main_fp through ntt_fwd_tail1024_pairs; k_split_special_fp, k_bmul_mid, k_gsplit_special through TailSched<10>),
    the raw (never re-centred) form primes of at most 48 bits take when half-done limbs are not packed, and FpArith's 4 + 4 + 2
    (k_split3_main_fp);
  * the N = 2^15 forms: a radix-32 cross pass (CrossLds: 2 + 3 stages; a sum of two residues is re-centred first for 49/50-bit
    primes), then the same tails (k_gsplit_main: FpTail, k_gsplit_main_deep: FpArith 3 + 4 + 3); inverse: ten-stage block tails,
    then the cross pass with its re-centring after three stages;

on adversarial inputs (runs of q - 1, (q +- 1)/2 and 0, alternating signs) and random ones, for primes of 40, 48, 49 and 50
bits, and asserts for each: both FMA steps are exact, every intermediate stays below 2^53, the residues equal the oracle's
transform.  Concrete inputs do not reach the worst case of every rounding at once, so the proof obligation itself -- the bound
recurrence over each schedule -- is asserted next to the replay, and as a check on that bookkeeping the schedule FpTail had
before (4 + 4 stages before its one re-centring) is shown to pass 2^53 for a 50-bit prime under the new growth while it did
not under the old one.  The plans are written from the tables SCHED / TAIL_SCHED below, and test_plans_follow_the_header parses
the Sched<> / TailSched<> specialisations out of abc_ntt.hpp and compares: a header edit without a model edit fails there, so the
proof stays about the schedule that is compiled.  No GPU, no HIP library.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "abc_amd", "csrc", "abc_ntt.hpp")
NTT_KERNELS = os.path.join(ROOT, "abc_amd", "csrc", "abc_kernels_ntt.hip")

LIMIT = 1 << 53
BITS = [40, 48, 49, 50]
C = "c"  # a re-centring step of a plan


def _pow(a, e, q):
    return pow(int(a), int(e), int(q))


def _min_root(two_n, q):
    cof = (q - 1) // two_n
    g = next(c for c in (_pow(x, cof, q) for x in range(2, 1000)) if _pow(c, two_n // 2, q) == q - 1)
    sq, best, cur = g * g % q, g, g
    for _ in range(two_n // 2):
        best = min(best, cur)
        cur = cur * sq % q
    return best


def _bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def _tables(n, q):
    """device tables: forward and inverse twiddles in bit-reversed order, each ONE centred value"""
    logn = n.bit_length() - 1
    psi = _min_root(2 * n, q)
    tw, p = [0] * n, 1
    for i in range(n):
        tw[_bitrev(i, logn)] = p
        p = p * psi % q
    centred = lambda w: w - q if w > q // 2 else w
    return [centred(w) for w in tw], [centred(_pow(w, q - 2, q)) for w in tw]


class Model:
    """exact replay of fp_mul_tw / fp_centre with range bookkeeping"""

    def __init__(self, q):
        self.q, self.qinv = q, 1.0 / float(q)
        self.peak = 0

    def mul_tw(self, y, w):
        q = self.q
        prod = y * w
        h = float(prod)                 # fl(y w): correctly rounded int -> double
        hi = int(h)
        l = prod - hi                   # the FMA's low part, must be a double
        assert float(l) == l, "low product part is not a double"
        c = round(h * self.qinv)        # rint(fl(h * qinv)): round() on a float is round-half-even -- the only approximate quantity
        d = hi - c * q                  # fma(-c, q, h), exact iff representable
        assert abs(d) < LIMIT, "h - c q left the exact range"
        v = d + l
        assert abs(v) < LIMIT
        return v

    def mul_lazy(self, y, w, wq):
        """fp_mul_lazy: y * w for a constant that carries wq = fl(w / q); the quotient comes from fl(y * wq)"""
        q = self.q
        prod = y * w
        h = float(prod)
        hi = int(h)
        l = prod - hi
        assert float(l) == l, "low product part is not a double"
        c = round(float(y) * wq)        # |y| < 2^53 is an integer-valued double already
        d = hi - c * q
        assert abs(d) < LIMIT, "h - c q left the exact range"
        v = d + l
        assert abs(v) < LIMIT
        return v

    def centre(self, x):
        r = x - round(float(x) * self.qinv) * self.q
        assert abs(r) <= self.q // 2 + 1
        return r

    def see(self, xs):
        p = max(max(xs), -min(xs))
        if p > self.peak:
            self.peak = p
        assert p < LIMIT, "a value left the exact range"


def _to_canon(x, q):
    """fp_to_canon on integer-valued doubles, its bit manipulation replayed with numpy: centre, add q where the sign bit of the high
    dword is set (a mask, no comparison), add 2^52 and strip the exponent.  fma(-c, q, x) is exact whenever its result fits 53 bits
    (asserted), so integers give it; a result that cancels to zero is +0 in round-to-nearest (c and x are never both -0: -0 in gives
    c = -0, so the product -c q is +0), which is what the array built from integers holds."""
    x = np.asarray(x, dtype=np.float64)
    qd = np.float64(q)
    qinv = np.float64(1.0) / qd
    c = np.rint(x * qinv)
    r_int = [int(a) - int(b) * q for a, b in zip(x, c)]
    assert all(abs(v) < LIMIT for v in r_int)
    r = np.array(r_int, dtype=np.float64)
    neg = ((r.view(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.int32) >> 31).view(np.uint32).astype(np.uint64)
    qb = np.array([qd]).view(np.uint64)[0]
    add = (((qb >> np.uint64(32)) & neg) << np.uint64(32)) | ((qb & np.uint64(0xffffffff)) & neg)
    r = r + add.view(np.float64)
    return (r + np.float64(4503599627370496.0)).view(np.uint64) & np.uint64(0x000fffffffffffff)


def _from_u64(v):
    """fp_from_u64: the word below 2^52 dropped into the mantissa of 2^52, minus 2^52"""
    v = np.asarray(v, dtype=np.uint64)
    return (v | np.uint64(0x4330000000000000)).view(np.float64) - np.float64(4503599627370496.0)


def _run_forward(x, q, tw, plan, canon=False):
    """Cooley-Tukey, natural in -> bit-reversed out; plan = stage counts and re-centrings in the order the kernels apply them"""
    n = len(x)
    m = Model(q)
    x = list(x)
    m.see(x)
    stage = 0
    for step in plan:
        if step == C:
            x = [m.centre(v) for v in x]
            continue
        for _ in range(step):
            half, blocks = n >> (stage + 1), 1 << stage
            for b in range(blocks):
                w = tw[blocks + b]
                base = b * 2 * half
                for j in range(base, base + half):
                    a = x[j]
                    v = m.mul_tw(x[j + half], w)
                    x[j], x[j + half] = a + v, a - v
            m.see(x)
            stage += 1
    assert 1 << stage == n
    if canon:  # the stand-alone kernels' store functor
        return [int(v) for v in _to_canon([float(v) for v in x], q)], m.peak
    return [v % q for v in x], m.peak


def _run_inverse(x, q, itw, plan, finish=False):
    """Gentleman-Sande, bit-reversed in -> natural out (before N^-1): X = a + b, Y = (a - b) w"""
    n = len(x)
    m = Model(q)
    x = list(x)
    m.see(x)
    stage = n.bit_length() - 1
    for step in plan:
        if step == C:
            x = [m.centre(v) for v in x]
            continue
        for _ in range(step):
            stage -= 1
            half, blocks = n >> (stage + 1), 1 << stage
            for b in range(blocks):
                w = itw[blocks + b]
                base = b * 2 * half
                for j in range(base, base + half):
                    a, c = x[j], x[j + half]
                    d = a - c
                    assert abs(d) < LIMIT
                    x[j], x[j + half] = a + c, m.mul_tw(d, w)
            m.see(x)
    assert stage == 0
    inv_n = _pow(n, q - 2, q)
    if finish:  # the stand-alone kernels' end: fp_mul_lazy by the centred N^-1 and its fl(w / q) (make_mod), then fp_to_canon
        w = inv_n - q if inv_n > q // 2 else inv_n
        wq = float(w) / float(q)
        x = [m.mul_lazy(v, w, wq) for v in x]
        m.see(x)
        return [int(v) for v in _to_canon([float(v) for v in x], q)], m.peak
    return [v * inv_n % q for v in x], m.peak


def _qmax(bits):
    """the bounds below grow with q, so the largest prime of a width is its worst case: q = 1 (mod 2N), N >= 1024"""
    return float((1 << bits) - 2047)


def _forward_bound(plan, start, bits):
    """worst case of |value| over a forward plan: Y -> Y (1 + 1.5 q 2^-53) + q/2 per stage, a re-centring gives q/2 + 2
    (fp_centre: the quotient of |x| <= 8 q is off by at most 2^-49, so the remainder by q 2^-49 < 2)"""
    q = _qmax(bits)
    g, y, peak = 1.0 + 1.5 * q * 2.0 ** -53, start, start
    for step in plan:
        if step == C:
            y = q / 2 + 2.0
            continue
        for _ in range(step):
            y = y * g + q / 2
            peak = max(peak, y)
    return peak


def _inverse_bound(plan, start, bits):
    """the same for an inverse plan: |a + b| <= 2 Y, |(a - b) w| <= q/2 + 1.5 (2 Y) q 2^-53"""
    q = _qmax(bits)
    e, y, peak = 1.5 * q * 2.0 ** -53, start, start
    for step in plan:
        if step == C:
            y = q / 2 + 2.0
            continue
        for _ in range(step):
            y = max(2.0 * y, q / 2 + 2.0 * y * e)
            peak = max(peak, y)
    return peak


def _red(bits):
    return [C] if bits >= 49 else []   # FpK::red: FpArith re-centres before every pass but the first


def _c50(bits):
    return [C] if bits == 50 else []   # FpTail: one re-centring, 50-bit primes only


# The pass schedules the plans are written from: Sched<LB> / TailSched<LB> of abc_ntt.hpp (test_plans_follow_the_header compares)
SCHED = {10: (4, 4, 2, 0), 11: (4, 3, 2, 2), 12: (4, 4, 2, 2), 13: (4, 4, 3, 2), 14: (4, 4, 4, 2)}
TAIL_SCHED = {10: (3, 4, 3, 0)}
BIG_BLOCK_LB = 12                      # kBigBlockLB of abc_kernels_ntt.hip: the block under the strided pass for N > 2^14


def _tail(bits):                       # FpTail, 3 + 4 + 3 from centred values: its one re-centring comes before pass 2
    r0, r1, r2, _ = TAIL_SCHED[10]
    return [r0, r1] + _c50(bits) + [r2]


def _fwd_block(lb, bits):
    """ntt_fwd_block_a<LB, FpArith>: FpArith::fwd_begin<PASS> re-centres before every pass but the first, 49/50-bit primes only"""
    plan = []
    for i, r in enumerate(r for r in SCHED[lb] if r):
        plan += (_red(bits) if i else []) + [r]
    return plan


def _inv_block(lb, bits):
    """ntt_inv_block_a<LB, FpArith>: the passes of Sched<LB> backwards; FpArith::inv_begin<PASS> re-centres before every pass but the
    first, and before that one too for 49/50-bit primes"""
    plan = []
    for i, r in enumerate(r for r in reversed(SCHED[lb]) if r):
        plan += ([C] if i else _red(bits)) + [r]
    return plan


# forward plans: name -> (logn, plan(bits), kind of input, applicable(bits))
FORWARD = {
    # ntt_fwd_block_a<14, FpArith>: 4 + 4 + 4 + 2 from a canonical input
    "whole14": (14, lambda b: _fwd_block(14, b), "canonical", lambda b: True),
    # register pass (k_split2_tensor_pass0_fp: residue of another prime; k_split3_pass_fp: t + fix), re-centred load
    # (packed limbs, 49/50-bit primes, the special prime), FpTail
    "split14_tail": (14, lambda b: [4, C] + _tail(b), "foreign", lambda b: True),
    "split14_tail_sum": (14, lambda b: [4, C] + _tail(b), "sum", lambda b: True),
    # the same without any re-centring: raw half-done limbs of primes of at most 48 bits
    "split14_raw": (14, lambda b: [4, 3, 4, 3], "foreign", lambda b: b <= 48),
    # k_split3_main_fp: ntt_fwd_block_a<10, FpArith>, 4 + 4 + 2 behind the register pass
    "split14_fparith": (14, lambda b: [4, C] + _fwd_block(10, b), "sum", lambda b: True),
    # N = 2^15: CrossLds::forward (2 + 3 stages; a sum is re-centred first for 49/50-bit primes), then k_gsplit_main's FpTail
    "cross15_tail": (15, lambda b: [5, C] + _tail(b), "foreign", lambda b: True),
    "cross15_tail_sum": (15, lambda b: _red(b) + [5, C] + _tail(b), "sum", lambda b: True),
    # k_gsplit_main_deep: FpArith through ntt_fwd_tail1024_pairs, the load re-centred for 49/50-bit primes only
    "cross15_deep": (15, lambda b: _red(b) + [5] + _red(b) + [3] + _red(b) + [4] + _red(b) + [3], "sum", lambda b: True),
}
# k_ntt_fwd_fp<LB>, S0 = 0 (launch_ntt, N = 2^10 .. 2^13): one whole block from a canonical input (fp_from_u64)
for _lb in (10, 11, 12, 13):
    FORWARD["whole%d" % _lb] = (_lb, lambda b, lb=_lb: _fwd_block(lb, b), "canonical", lambda b: True)
# launch_ntt, N = 2^14 with few limbs in flight: k_ntt_fwd_strided_fp<4> (four stages, nothing re-centred, raw doubles out), then
# k_ntt_fwd_fp<10> with S0 = 4: the load re-centres (fp_centre, every width), then Sched<10> under FpArith
FORWARD["few14"] = (14, lambda b: [4, C] + _fwd_block(10, b), "canonical", lambda b: True)
# N = 2^15 / 2^16: k_ntt_fwd_strided_fp<logN - 12>, then k_ntt_fwd_fp<12> with S0 = logN - 12 in the same way
for _logn in (15, 16):
    FORWARD["big%d" % _logn] = (_logn, lambda b, s0=_logn - BIG_BLOCK_LB: [s0, C] + _fwd_block(BIG_BLOCK_LB, b), "canonical",
                                lambda b: True)
# the plans of the stand-alone kernels (abc_kernels_ntt.hip) are replayed to their last instruction: the forward store is
# fp_to_canon, the inverse one fp_mul_lazy by N^-1, then fp_to_canon
STANDALONE = {"whole10", "whole11", "whole12", "whole13", "whole14", "few14", "big15", "big16"}
FULL_INPUTS = {"whole10", "whole11", "whole12", "whole13", "whole14", "few14"}  # the others: the "few" set (pure Python at N >= 2^15)
# what a plan may start from (the bound) -- "foreign": a canonical residue of another prime, |y| < 2^50 whatever q
START = {"canonical": lambda bits: _qmax(bits), "sum": lambda bits: 2.0 * _qmax(bits), "foreign": lambda bits: 2.0 ** 50}

# inverse plans: ntt_inv_block_a re-centres before every pass but the first, and before that one too for 49/50-bit primes
INVERSE = {
    # ntt_inv_block_a<14>: 2 + 4 + 4 + 4; also k_split_special_fp's block tail (2 + 4 + 4) followed by k_split3_pass_fp (centre16 + 4)
    "whole14": (14, lambda b: _inv_block(14, b)),
    # N = 2^15: block tails 2 + 4 + 4, then CrossLds::inverse (re-centred load, 3 stages, re-centring, 2 stages)
    "tails15_cross": (15, lambda b: _red(b) + [2, C, 4, C, 4, C, 3, C, 2]),
}
# k_ntt_inv_fp<LB>, S0 = 0: one whole block
for _lb in (10, 11, 12, 13):
    INVERSE["whole%d" % _lb] = (_lb, lambda b, lb=_lb: _inv_block(lb, b))
# few limbs at N = 2^14: k_ntt_inv_fp<10> with S0 = 4 hands raw doubles (at most 8 q + 32: four stages from re-centred values) to
# k_ntt_inv_strided_fp<4>, whose load re-centres whatever the width
INVERSE["few14"] = (14, lambda b: _inv_block(10, b) + [C, 4])
# N = 2^15 / 2^16: k_ntt_inv_fp<12>, then k_ntt_inv_strided_fp<3> / <4>
for _logn in (15, 16):
    INVERSE["big%d" % _logn] = (_logn, lambda b, s0=_logn - BIG_BLOCK_LB: _inv_block(BIG_BLOCK_LB, b) + [C, s0])


def _inputs(n, q, kind, rng, few):
    top = {"canonical": q - 1, "sum": 2 * q - 2, "foreign": (1 << 50) - 1}[kind]
    mid_lo, mid_hi = (q - 1) // 2, (q + 1) // 2
    sets = {
        "all top": [top] * n,
        "runs": [(top, mid_hi, 0, mid_lo)[(i >> 5) & 3] for i in range(n)],
        "random": [int(v) for v in rng.integers(0, top + 1, size=n, dtype=np.uint64)],
    }
    if not few:
        sets["alternating"] = [top if i & 1 else 0 for i in range(n)]
        sets["halves"] = [mid_lo if i % 3 else mid_hi for i in range(n)]
    return sets


def _prime(n, bits):
    from oracle import oracle_py as om
    primes = om.create_primes(n, [bits, 40 if bits != 40 else 41])
    return primes[0], om.Oracle(om.CKKS, n, primes)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_schedules_are_exact_and_match_the_oracle(name, bits):
    logn, plan_of, kind, applies = FORWARD[name]
    if not applies(bits):
        return  # a form only smaller primes are compiled into
    plan, n = plan_of(bits), 1 << logn
    # the proof obligation: the worst case over the schedule stays below 2^53 for the largest prime of this width
    assert _forward_bound(plan, START[kind](bits), bits) < 2.0 ** 53, (name, bits)
    q, o = _prime(n, bits)
    tw, _ = _tables(n, q)
    rng = np.random.default_rng(11)
    for label, x in _inputs(n, q, kind, rng, few=(name not in FULL_INPUTS)).items():
        got, peak = _run_forward(x, q, tw, plan, canon=(name in STANDALONE))
        want = o.ntt(0, np.array([v % q for v in x], dtype=np.uint64))
        assert got == [int(v) for v in want], (name, bits, label)
        assert peak < LIMIT, (name, bits, label, peak / q)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", list(INVERSE))
def test_inverse_schedules_are_exact_and_match_the_oracle(name, bits):
    logn, plan_of = INVERSE[name]
    plan, n = plan_of(bits), 1 << logn
    # inputs: canonical residues, or products of two of them (fp_mulmod: |x| < q)
    bound = _inverse_bound(plan, _qmax(bits), bits)
    assert bound < 2.0 ** 53, (name, bits)
    if name in STANDALONE:
        # what fp_mul_lazy is handed is at most 8 q + 32 (four stages from re-centred values), behind a strided pass as behind a block;
        # its quotient c = rint(fl(y fl(w/q))) is off by at most 1/2 + |y w / q| 2^-52, so |y w - c q| <= q/2 + |y| q 2^-53 <= 1.5 q + 4,
        # and h - c q, which differs from that by the low product part (at most half an ulp of |y w| < 2^102), is exact
        qm = _qmax(bits)
        assert bound <= 8.0 * qm + 32.0
        assert qm / 2 + bound * qm * 2.0 ** -53 + 2.0 ** 49 < 2.0 ** 53
    q, o = _prime(n, bits)
    _, itw = _tables(n, q)
    rng = np.random.default_rng(13)
    finish = name in STANDALONE
    for label, x in _inputs(n, q, "canonical", rng, few=(name not in FULL_INPUTS)).items():
        got, peak = _run_inverse(x, q, itw, plan, finish)
        want = o.intt(0, np.array(x, dtype=np.uint64))
        assert got == [int(v) for v in want], (name, bits, label)
        assert peak < LIMIT, (name, bits, label, peak / q)
    # signed inputs too: what fp_mulmod hands the inverse transform of a product, |x| < q
    x = [int(v) - (q - 1) for v in rng.integers(0, 2 * q - 1, size=n, dtype=np.uint64)]
    got, _ = _run_inverse(x, q, itw, plan, finish)
    assert got == [int(v) for v in o.intt(0, np.array([v % q for v in x], dtype=np.uint64))], (name, bits, "signed")


@pytest.mark.parametrize("bits", BITS)
def test_conversions_at_the_ends_of_the_range(bits):
    """fp_to_canon (the store of every stand-alone transform) on 0, -0, +-1, +-(q-1)/2, +-(q+1)/2, +-q, +-8 q, 8 q + 32 and random
    lazy values up to the 8 q + 32 an inverse pass may leave; fp_from_u64 (their load) on 0, q - 1 and the largest words"""
    from oracle import oracle_py as om
    rng = np.random.default_rng(bits)
    for n in (1024, 65536):
        q = om.create_primes(n, [bits, 40 if bits != 40 else 41])[0]
        edge = [0, 1, -1, (q - 1) // 2, -((q - 1) // 2), (q + 1) // 2, -((q + 1) // 2), q - 1, 1 - q, q, -q, q + 1, -q - 1,
                8 * q, -8 * q, 8 * q + 32, -8 * q - 32]
        assert 8 * q + 32 < LIMIT  # q = 1 (mod 2N) keeps even a 50-bit prime far enough below 2^50
        vals = edge + [int(v) - (8 * q + 32) for v in rng.integers(0, 16 * q + 65, size=20000, dtype=np.uint64)]
        x = np.array([float(v) for v in vals] + [-0.0], dtype=np.float64)
        want = [v % q for v in vals] + [0]
        assert [int(v) for v in _to_canon(x, q)] == want, (bits, n)
        words = [0, 1, q - 1, (1 << 50) - 1, (1 << 52) - 1] + [int(v) for v in rng.integers(0, 1 << 52, size=1000, dtype=np.uint64)]
        back = _from_u64(words)
        assert [int(v) for v in back] == words and all(float(w) == b for w, b in zip(words, back)), (bits, n)


def _header_schedules(header=HEADER, kernels=NTT_KERNELS):
    """the Sched<LB> / TailSched<LB> specialisations of abc_ntt.hpp and kBigBlockLB of abc_kernels_ntt.hip, as compiled"""
    pat = re.compile(r"template\s*<>\s*struct\s+(Sched|TailSched)\s*<\s*(\d+)\s*>\s*\{\s*static\s+constexpr\s+int\s+"
                     r"R0\s*=\s*(\d+)\s*,\s*R1\s*=\s*(\d+)\s*,\s*R2\s*=\s*(\d+)\s*,\s*R3\s*=\s*(\d+)\s*;\s*\}\s*;")
    found = {"Sched": {}, "TailSched": {}}
    with open(header) as f:
        text = f.read()
    for kind, lb, r0, r1, r2, r3 in pat.findall(text):
        assert int(lb) not in found[kind], "two specialisations of %s<%s>" % (kind, lb)
        found[kind][int(lb)] = (int(r0), int(r1), int(r2), int(r3))
    # every specialisation must have been understood: count the declarations independently of the pattern above
    assert len(re.findall(r"struct\s+Sched\s*<\s*\d+\s*>", text)) == len(found["Sched"])
    assert len(re.findall(r"struct\s+TailSched\s*<\s*\d+\s*>", text)) == len(found["TailSched"])
    with open(kernels) as f:
        big = re.findall(r"constexpr\s+int\s+kBigBlockLB\s*=\s*(\d+)\s*;", f.read())
    assert len(big) == 1
    return found, int(big[0])


def _stages(plan):
    return [s for s in plan if s != C]


def _check_plans_against(found, big):
    assert found["Sched"] == SCHED, "abc_ntt.hpp's Sched<> changed: the plans of this file describe another schedule"
    assert found["TailSched"] == TAIL_SCHED, "abc_ntt.hpp's TailSched<> changed: the plans of this file describe another schedule"
    assert big == BIG_BLOCK_LB
    for bits in BITS:
        for lb, sc in found["Sched"].items():
            assert sum(sc) == lb
            passes = [r for r in sc if r]
            assert _stages(FORWARD["whole%d" % lb][1](bits)) == passes
            assert _stages(INVERSE["whole%d" % lb][1](bits)) == passes[::-1]
        s10, sbig = [r for r in found["Sched"][10] if r], [r for r in found["Sched"][big] if r]
        t10 = [r for r in found["TailSched"][10] if r]
        assert _stages(FORWARD["few14"][1](bits)) == [4] + s10 and _stages(INVERSE["few14"][1](bits)) == s10[::-1] + [4]
        assert _stages(FORWARD["split14_fparith"][1](bits)) == [4] + s10
        for logn in (15, 16):
            assert _stages(FORWARD["big%d" % logn][1](bits)) == [logn - big] + sbig
            assert _stages(INVERSE["big%d" % logn][1](bits)) == sbig[::-1] + [logn - big]
        assert _stages(FORWARD["split14_tail"][1](bits)) == [4] + t10 and _stages(FORWARD["cross15_tail"][1](bits)) == [5] + t10
        # FpTail's one re-centring sits before its pass 2 (fwd_begin<2>), 50-bit primes only
        assert _tail(bits) == t10[:2] + ([C] if bits == 50 else []) + t10[2:]


def test_plans_follow_the_header():
    """the stage counts of the plans above are the constants the kernels are compiled with"""
    _check_plans_against(*_header_schedules())


def test_four_plus_four_tail_breaks_the_bound_for_50_bit_primes():
    """The check on the bookkeeping above.  FpTail used to run 4 + 4 stages from centred values before its one re-centring
    (ntt_fwd_block_a<10>: 4 + 4 + 2).  Under the growth of a stored w/q, Y (1 + q 2^-53) + q/2, eight stages of a 50-bit prime
    stay below 2^53; under the single-word growth they do not, seven do -- hence 3 + 4 + 3.  A second re-centring (before
    passes 1 and 2) would also do, at 48 more DP instructions per lane."""
    old_tail = [4, 4, C, 2]
    q50, q49, lim = _qmax(50), _qmax(49), 2.0 ** 53
    half50, half49 = q50 / 2 + 2.0, q49 / 2 + 2.0
    assert _forward_bound(old_tail, half50, 50) > lim          # 9.86 q against 8 q
    assert _forward_bound(_tail(50), half50, 50) < lim         # 7.88 q
    assert _forward_bound([4, C, 4, C, 2], half50, 50) < lim   # the alternative that was not taken
    # the same schedule under the old growth, for the record of why it was allowed
    y = q50 / 2
    for _ in range(8):
        y = y * (1.0 + q50 * 2.0 ** -53) + q50 / 2
    assert y < lim
    # a 49-bit prime needs no re-centring in a ten-stage tail, and the output of a 50-bit tail stays below 2.64 q
    assert _forward_bound([3, 4, 3], half49, 49) < 9.0 * q49 < lim
    assert _forward_bound([3], half50, 50) < 2.64 * q50
    # a sum of two residues must be re-centred before a radix-32 cross pass of a 50-bit prime (CrossLds::forward)
    assert _forward_bound([5], 2.0 * q50, 50) > lim > _forward_bound([C, 5], 2.0 * q50, 50)
    # and a canonical residue of any prime below 2^50 may take even the radix-64 pass of N = 2^16 as it is
    assert _forward_bound([6], 2.0 ** 50, 50) < lim
