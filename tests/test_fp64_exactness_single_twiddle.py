"""CPU model of the fp64 butterflies with ONE double per twiddle (abc_amd/csrc/abc_ntt.hpp: fp_mul_tw, FpArith, FpTail).

The quotient of a twiddle product is estimated from the product itself, c = rint(fl(fl(y w) * fl(1/q))), so the table keeps
only w.  Three roundings instead of two: one stage grows a bound Y on |value| to Y (1 + 1.5 q 2^-53) + q/2 (it was
Y (1 + q 2^-53) + q/2 with a stored w/q).  The estimate only chooses WHICH representative comes out; everything else is exact
as long as magnitudes stay below 2^53.  This file replays, with Python integers for the exact parts and IEEE doubles for the
estimate, every stage schedule the kernels are compiled with:

  * whole 14-stage forward and inverse transforms (ntt_fwd_block_a<14> / ntt_inv_block_a<14>, FpArith);
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
not under the old one.  No GPU, no HIP library.
"""
import numpy as np
import pytest

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

    def centre(self, x):
        r = x - round(float(x) * self.qinv) * self.q
        assert abs(r) <= self.q // 2 + 1
        return r

    def see(self, xs):
        p = max(max(xs), -min(xs))
        if p > self.peak:
            self.peak = p
        assert p < LIMIT, "a value left the exact range"


def _run_forward(x, q, tw, plan):
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
    return [v % q for v in x], m.peak


def _run_inverse(x, q, itw, plan):
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


def _tail(bits):                       # FpTail, 3 + 4 + 3 from centred values
    return [3, 4] + _c50(bits) + [3]


# forward plans: name -> (logn, plan(bits), kind of input, applicable(bits))
FORWARD = {
    # ntt_fwd_block_a<14, FpArith>: 4 + 4 + 4 + 2 from a canonical input
    "whole14": (14, lambda b: [4] + _red(b) + [4] + _red(b) + [4] + _red(b) + [2], "canonical", lambda b: True),
    # register pass (k_split2_tensor_pass0_fp: residue of another prime; k_split3_pass_fp: t + fix), re-centred load
    # (packed limbs, 49/50-bit primes, the special prime), FpTail
    "split14_tail": (14, lambda b: [4, C] + _tail(b), "foreign", lambda b: True),
    "split14_tail_sum": (14, lambda b: [4, C] + _tail(b), "sum", lambda b: True),
    # the same without any re-centring: raw half-done limbs of primes of at most 48 bits
    "split14_raw": (14, lambda b: [4, 3, 4, 3], "foreign", lambda b: b <= 48),
    # k_split3_main_fp: ntt_fwd_block_a<10, FpArith>, 4 + 4 + 2 behind the register pass
    "split14_fparith": (14, lambda b: [4, C, 4] + _red(b) + [4] + _red(b) + [2], "sum", lambda b: True),
    # N = 2^15: CrossLds::forward (2 + 3 stages; a sum is re-centred first for 49/50-bit primes), then k_gsplit_main's FpTail
    "cross15_tail": (15, lambda b: [5, C] + _tail(b), "foreign", lambda b: True),
    "cross15_tail_sum": (15, lambda b: _red(b) + [5, C] + _tail(b), "sum", lambda b: True),
    # k_gsplit_main_deep: FpArith through ntt_fwd_tail1024_pairs, the load re-centred for 49/50-bit primes only
    "cross15_deep": (15, lambda b: _red(b) + [5] + _red(b) + [3] + _red(b) + [4] + _red(b) + [3], "sum", lambda b: True),
}
# what a plan may start from (the bound) -- "foreign": a canonical residue of another prime, |y| < 2^50 whatever q
START = {"canonical": lambda bits: _qmax(bits), "sum": lambda bits: 2.0 * _qmax(bits), "foreign": lambda bits: 2.0 ** 50}

# inverse plans: ntt_inv_block_a re-centres before every pass but the first, and before that one too for 49/50-bit primes
INVERSE = {
    # ntt_inv_block_a<14>: 2 + 4 + 4 + 4; also k_split_special_fp's block tail (2 + 4 + 4) followed by k_split3_pass_fp (centre16 + 4)
    "whole14": (14, lambda b: _red(b) + [2, C, 4, C, 4, C, 4]),
    # N = 2^15: block tails 2 + 4 + 4, then CrossLds::inverse (re-centred load, 3 stages, re-centring, 2 stages)
    "tails15_cross": (15, lambda b: _red(b) + [2, C, 4, C, 4, C, 3, C, 2]),
}


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
    for label, x in _inputs(n, q, kind, rng, few=(name != "whole14")).items():
        got, peak = _run_forward(x, q, tw, plan)
        want = o.ntt(0, np.array([v % q for v in x], dtype=np.uint64))
        assert got == [int(v) for v in want], (name, bits, label)
        assert peak < LIMIT, (name, bits, label, peak / q)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", list(INVERSE))
def test_inverse_schedules_are_exact_and_match_the_oracle(name, bits):
    logn, plan_of = INVERSE[name]
    plan, n = plan_of(bits), 1 << logn
    # inputs: canonical residues, or products of two of them (fp_mulmod: |x| < q)
    assert _inverse_bound(plan, _qmax(bits), bits) < 2.0 ** 53, (name, bits)
    q, o = _prime(n, bits)
    _, itw = _tables(n, q)
    rng = np.random.default_rng(13)
    for label, x in _inputs(n, q, "canonical", rng, few=(name != "whole14")).items():
        got, peak = _run_inverse(x, q, itw, plan)
        want = o.intt(0, np.array(x, dtype=np.uint64))
        assert got == [int(v) for v in want], (name, bits, label)
        assert peak < LIMIT, (name, bits, label, peak / q)
    # signed inputs too: what fp_mulmod hands the inverse transform of a product, |x| < q
    x = [int(v) - (q - 1) for v in rng.integers(0, 2 * q - 1, size=n, dtype=np.uint64)]
    got, _ = _run_inverse(x, q, itw, plan)
    assert got == [int(v) for v in o.intt(0, np.array([v % q for v in x], dtype=np.uint64))], (name, bits, "signed")


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
