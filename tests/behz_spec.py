"""The BFV multiply and decryption restated over the integers -- TEST INFRASTRUCTURE ONLY.

Python integers only; neither the product nor the oracle is imported.  The multiply is the ONE integer that the q-residues of its
operands fix: no auxiliary prime, no RNS arithmetic beyond reading and writing residues modulo the ciphertext primes.  With
Q = prod q_i, Q_i = Q / q_i and m~ = 2^32, per coefficient:

  extend   y_i = [a_i m~ Q_i^-1]_{q_i};  X = sum y_i Q_i;  alpha = X div Q;  r = [-X Q^-1]_{m~}, taken as r - m~ when r >= 2^31;
           Y = (X + Q r) / m~   (exact)
  tensor   D0 = Ya0 Yb0,  D1 = Ya0 Yb1 + Ya1 Yb0,  D2 = Ya1 Yb1   (negacyclic, over the integers)
  floor    z_i = [D t Q_i^-1]_{q_i};  S = sum z_i Q_i;  beta = S div Q;  E = (t D - S) / Q   (exact)
  result   limb i of the product is E mod q_i

The points where a residue is used as an integer -- the canonical summands y_i and z_i, r and its centring at 2^31, the overflow
counts alpha and beta -- are what the builders below aim at: each returns residues together with the (y, alpha, r) or (z, beta) the
model computes for them, so a test can check the construction and not trust it.

The second operand of `multiply_at` is a short list of terms c x^k per polynomial (a pair of monomials on the big rings), which
keeps the model O(positions x terms) on every ring.
"""
from collections import namedtuple

import numpy as np

M_TILDE = 1 << 32
HALF = 1 << 31
R_TARGETS = (0, 1, HALF - 1, HALF, HALF + 1, M_TILDE - 1)  # r before centring; HALF is the tie

Extended = namedtuple("Extended", "Y y alpha r")  # r: before centring, in [0, m~)
Floored = namedtuple("Floored", "E z beta")
Crafted = namedtuple("Crafted", "name res y alpha r")     # a coefficient whose extension is pinned
CraftedFloor = namedtuple("CraftedFloor", "name res z beta")  # a coefficient of a0 whose floor (with b0 = 1) is pinned


def extremes(q):
    return (0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1)


EXTREME_NAMES = ("0", "1", "(q-1)/2", "(q+1)/2", "q-2", "q-1")


class Behz:
    def __init__(self, data_primes, t):
        self.q = [int(p) for p in data_primes]
        self.L = len(self.q)
        self.t = int(t)
        self.Q = 1
        for p in self.q:
            self.Q *= p
        self.Qi = [self.Q // p for p in self.q]
        inv = [pow(Qi % p, -1, p) for Qi, p in zip(self.Qi, self.q)]
        self.ext_mul = [M_TILDE * v % p for v, p in zip(inv, self.q)]   # m~ Q_i^-1 mod q_i
        self.flr_mul = [self.t * v % p for v, p in zip(inv, self.q)]    # t Q_i^-1 mod q_i
        self.neg_inv_q = -pow(self.Q, -1, M_TILDE) % M_TILDE

    # ---- the model ----
    def extend(self, res, tie_up=False):
        """tie_up: the wrong centring, r = 2^31 kept positive (a `>` where SEAL has `>=`)"""
        y = [int(a) * m % p for a, m, p in zip(res, self.ext_mul, self.q)]
        X = sum(v * Qi for v, Qi in zip(y, self.Qi))
        r = X * self.neg_inv_q % M_TILDE
        rc = r - M_TILDE if (r > HALF if tie_up else r >= HALF) else r
        num = X + self.Q * rc
        assert num % M_TILDE == 0
        return Extended(num // M_TILDE, y, X // self.Q, r)

    def floor(self, D):
        z = [D % p * m % p for m, p in zip(self.flr_mul, self.q)]
        S = sum(v * Qi for v, Qi in zip(z, self.Qi))
        num = self.t * D - S
        assert num % self.Q == 0
        return Floored(num // self.Q, z, S // self.Q)

    def multiply_at(self, a, b_terms, positions, tie_up=False, trace=None):
        """a: uint64 [2][L][N]; b_terms: per polynomial of b a list of (k, residues of c) for the terms c x^k; the product's
        residues uint64 [3][L][len(positions)].  trace (a dict): filled with (component, position) -> Floored."""
        n = a.shape[-1]
        ya = {}

        def Ya(p, x):
            if (p, x) not in ya:
                ya[p, x] = self.extend([int(a[p, i, x]) for i in range(self.L)], tie_up).Y
            return ya[p, x]

        yb = [[(k, self.extend(c, tie_up).Y) for k, c in terms] for terms in b_terms]

        def conv(p, s, j):  # coefficient j of a_p b_s modulo x^N + 1
            acc = 0
            for k, Y in yb[s]:
                acc += Ya(p, j - k) * Y if j >= k else -Ya(p, j - k + n) * Y
            return acc

        out = np.empty((3, self.L, len(positions)), dtype=np.uint64)
        for col, j in enumerate(positions):
            j = int(j)
            D = (conv(0, 0, j), conv(0, 1, j) + conv(1, 0, j), conv(1, 1, j))
            for comp in range(3):
                f = self.floor(D[comp])
                if trace is not None:
                    trace[comp, j] = f
                for i, p in enumerate(self.q):
                    out[comp, i, col] = f.E % p
        return out

    def multiply(self, a, b_terms, tie_up=False):
        return self.multiply_at(a, b_terms, range(a.shape[-1]), tie_up)

    def dense(self, b_terms, n):
        """the operand multiply_at takes as terms, as residues uint64 [2][L][n]"""
        b = np.zeros((2, self.L, n), dtype=np.uint64)
        for s, terms in enumerate(b_terms):
            for k, c in terms:
                assert not b[s, :, k].any()
                b[s, :, k] = [int(v) for v in c]
        return b

    # ---- crafted coefficients: extension ----
    def from_y(self, name, y):
        res = [v * pow(m, -1, p) % p for v, m, p in zip(y, self.ext_mul, self.q)]
        e = self.extend(res)
        return Crafted(name, res, e.y, e.alpha, e.r)

    def _patterns(self):
        """choices of one extreme per limb: the same in every limb, then mixed ones"""
        L = self.L
        pats = [(EXTREME_NAMES[e] + " in every limb", [e] * L) for e in range(6)]
        pats.append(("q-1 / 0 alternating", [5 if i % 2 == 0 else 0 for i in range(L)]))
        pats.append(("0 / q-1 alternating", [0 if i % 2 == 0 else 5 for i in range(L)]))
        pats.append(("extremes in turn", [i % 6 for i in range(L)]))
        pats.append(("extremes in turn, reversed", [(5 - i) % 6 for i in range(L)]))
        return pats

    def extend_summands(self):
        """y_i at the extremes: 'q-1 in every limb' is alpha = L - 1, the largest sum a conversion out of q adds up; '0' is alpha = 0"""
        return [self.from_y("y: " + name, [extremes(p)[e] for e, p in zip(pat, self.q)]) for name, pat in self._patterns()]

    def r_ties(self):
        """for each target r: y_1 .. y_{L-1} at extremes, y_0 solved modulo 2^32 -- its smallest and its largest representative
        below q_0 (every chain prime here is above 2^32)"""
        assert self.q[0] > M_TILDE
        out = []
        inv_q0 = pow(self.Qi[0], -1, M_TILDE)
        for target in R_TARGETS:
            for name, pat in (("q-1", [5] * self.L), ("0", [0] * self.L), ("in turn", [(i + 2) % 6 for i in range(self.L)])):
                rest = [extremes(p)[e] for e, p in zip(pat, self.q)][1:]
                tail = sum(v * Qi for v, Qi in zip(rest, self.Qi[1:]))
                lo = (-target * self.Q - tail) * inv_q0 % M_TILDE
                hi = lo + (self.q[0] - 1 - lo) // M_TILDE * M_TILDE
                for rep, y0 in (("smallest", lo), ("largest", hi)):
                    out.append(self.from_y("r = %#x, other y at %s, %s y_0" % (target, name, rep), [y0] + rest))
        return out

    # ---- crafted coefficients: floor (as a coefficient of a0 against b0 = 1: D0 = a0 modulo Q) ----
    def floor_summands(self):
        out = []
        for name, pat in self._patterns():
            z = [extremes(p)[e] for e, p in zip(pat, self.q)]
            res = [v * pow(m, -1, p) % p for v, m, p in zip(z, self.flr_mul, self.q)]
            S = sum(v * Qi for v, Qi in zip(z, self.Qi))
            out.append(CraftedFloor("z: " + name, res, z, S // self.Q))
        return out

    # ---- decryption ----
    def decrypt(self, v):
        """exact rounding of t v / Q, modulo t"""
        return (2 * self.t * v + self.Q) // (2 * self.Q) % self.t

    def decrypt_is_pinned(self, v):
        """v is at least Q / (4t) away from every rounding boundary (k + 1/2) Q / t: there SEAL's gamma-corrected rounding is
        exact rounding (right at a boundary it is not, by design)"""
        w = 2 * self.t * v % (2 * self.Q)  # boundaries are the odd multiples of Q on this scale; the distance scales by 2t
        return 2 * abs(w - self.Q) >= self.Q

    def crt(self, res):
        return sum(int(v) * pow(Qi % p, -1, p) % p * Qi for v, Qi, p in zip(res, self.Qi, self.q)) % self.Q

    def residues(self, values):
        """integers -> uint64 [L][len(values)]"""
        return np.array([[v % p for v in values] for p in self.q], dtype=np.uint64)

    def decrypt_phases(self, n, gamma, rng):
        """n phases in [0, Q) and the family of each.  Only 'boundary', the two specials at Q/2 and about half of the handful of
        'gamma' phases lie where decrypt_is_pinned says no: 'random' phases are redrawn until they are pinned (the oracle is
        asserted on every phase; near-boundary phases are the 'boundary' family's job)."""
        Q, t = self.Q, self.t
        fam, v = [], []

        def put(name, x):
            fam.append(name)
            v.append(x % Q)

        for x in (0, 1, Q - 1, Q // 2, Q // 2 + 1):
            put("special", x)
        tg_mul = [t * gamma % p * pow(Qi % p, -1, p) % p for Qi, p in zip(self.Qi, self.q)]  # t gamma Q_i^-1 mod q_i
        for name, pat in self._patterns():
            w = [extremes(p)[e] for e, p in zip(pat, self.q)]
            put("gamma", self.crt([x * pow(m, -1, p) % p for x, m, p in zip(w, tg_mul, self.q)]))
        quarter = -(-Q // (4 * t)) + 1
        for _ in range(n // 32):
            k = int(rng.integers(0, t))
            edge = (2 * k + 1) * Q // (2 * t)
            for d in (-1, 0, 1, 2):
                put("boundary", edge + d)
        for _ in range(n // 32):
            k = int(rng.integers(0, t))
            edge = (2 * k + 1) * Q // (2 * t)
            put("quarter", edge + 1 + quarter)
            put("quarter", edge - quarter)
        while len(v) < n:
            x = int.from_bytes(rng.bytes((Q.bit_length() + 71) // 8), "little") % Q
            if self.decrypt_is_pinned(x):
                put("random", x)
        assert len(v) == n
        return v, fam


def kernel_positions(n):
    """where a crafted coefficient must also be tried: index 0 and N - 1, both sides of every 1024- and 4096-point block boundary,
    and in the split multiply's layout x = kb << 10 | pg P | p (2^R blocks of 1024, P = 512 >> R positions per group, R = log N - 10)
    kb, pg and p each at 0 and at their maximum"""
    pos = {0, n - 1}
    for step in (1024, 4096):
        for edge in range(step, n, step):
            pos.update((edge - 1, edge))
    logn = n.bit_length() - 1
    if logn >= 13:
        R = logn - 10
        P = 512 >> R
        npg = 1024 // P
        for kb in (0, (1 << R) - 1):
            for pg in (0, 1, npg // 2, npg - 1):
                for p in (0, P - 1):
                    pos.add((kb << 10) | (pg * P) | p)
    return sorted(pos)


def random_residues(spec, shape, rng):
    """uniform residues, uint64 [*shape[:-1]][L][shape[-1]] with the limb axis second to last"""
    return np.stack([rng.integers(0, p, size=shape, dtype=np.uint64) for p in spec.q], axis=-2)


def crafted_batch(spec, n, rng, sparse_terms=0):
    """Three operands a [3][2][L][n], the second operand of each as terms, and what was crafted where.

    Row 0: b0 = 1, b1 a monomial; a0 holds the floor summands, a1 the extension summands and the ties of r.  Row 1: random
    residues.  Row 2: b0 and b1 arbitrary monomials (sparse_terms > 0: that many terms each); a0 and a1 hold the extension
    coefficients, assigned in a different order.  Crafted coefficients go to kernel_positions(n) first, in turn, then to further
    random positions until each has been placed at least once; everything else is random.
    Returns (a, terms, marks): terms[row] = (terms of b0, terms of b1); marks = [(row, poly, position, crafted)]."""
    L = spec.L
    a = random_residues(spec, (3, 2, n), rng)
    ext = spec.extend_summands() + spec.r_ties()
    flo = spec.floor_summands()
    pos = kernel_positions(n)
    taken = set(pos)
    spare = [int(x) for x in rng.permutation(n) if int(x) not in taken]
    pos = pos + spare[:max(0, len(ext) - len(pos))]
    marks = []

    def put(row, poly, items, shift):
        for i, x in enumerate(pos):
            c = items[(i + shift) % len(items)]
            a[row, poly, :, x] = c.res
            marks.append((row, poly, x, c))

    put(0, 0, flo, 0)
    put(0, 1, ext, 0)
    put(2, 0, ext, 7)
    put(2, 1, ext, 19)

    def monomials(count):
        ks = [int(k) for k in rng.choice(n, size=count, replace=False)]
        return [(k, [int(rng.integers(1, p)) for p in spec.q]) for k in ks]

    count = sparse_terms or 1
    terms = [([(0, [1] * L)], monomials(1)), (monomials(1), monomials(1)), (monomials(count), monomials(count))]
    return a, terms, marks


def tie_outputs(n, terms, marks):
    """(row, component, position) of every product coefficient that a crafted r = 2^31 of `a` enters"""
    hit = set()
    for row, poly, x, c in marks:
        if isinstance(c, Crafted) and c.r == HALF:
            for s in (0, 1):
                for k, _ in terms[row][s]:
                    hit.add((row, poly + s, (x + k) % n))
    return hit
