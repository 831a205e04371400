"""The exact model of the RELAXED arithmetic on saturated 32-bit limbs (algebra_amd/csrc/fp.cuh: residues kept in [0, 2p), sometimes
2p itself, product operands of up to 2 NEG_BETA p; Fp, Fp2, Fp2Half) and of the XYZZ additions that run on it (ec.cuh:
xyzz_madd_relaxed, xyzz_add_relaxed, xyzz_canonical), in Python integers only.

Every op is restated from its DEFINITION -- a Montgomery reduction is (s + m p) / R with m = s (-p^-1) mod R, whatever the column
schedule; a conditional subtraction is a comparison of integers -- and carries its PRECONDITION as the header states it (operand
below 2p, at most 2p, below 4p, c2 at most 6p, sum of products at most R p or 3 R p).  A vector outside a precondition raises
OutOfContract: it fails the test, it is never skipped.  For every result `check_row` holds (b) the residue mod p it must
represent and (c) closure: the documented output class; (a) is the exact limbs, which the tests compare with the device and
with the header's host forms.  `vectors` builds the deterministic edge rows and the seeded random rows both test modules send;
`DOCUMENTED` is the table of the header's bounds with file and line, re-derived exactly from p.

Values are plain integers (the N-limb number), Fp2 / Fp2Half elements are (c0, c1) tuples of them."""
import functools
import random

import numpy as np

import pyref as P


class OutOfContract(Exception):
    pass


def need(cond, what):
    if not cond:
        raise OutOfContract(what)


FIELD_ID = {f: i for i, f in enumerate(P.FIELD_ORDER)}
NEG_BETA = {"BLS12_381_FQ": 1, "BLS12_377_FQ": 5}
M_BASE, M_SCALAR, M_ALL, M_EXT = 0x15, 0x2A, 0x3F, 0x14
U_FP, U_FP2, U_HALF = 0, 1, 2

# name -> (op, arity, unit, fields, operand classes): csrc/relaxtest_api.hpp THE TABLE (compared with the header through the host
# runner's --table).  Classes: "p" < p, "=p" <= p, "2p" < 2p, "=2p" <= 2p, "4p" < 4p, "=6p" <= 6p.
TABLE = {
    "mul_r": (0, 2, U_FP, M_BASE, ("=2p", "=2p")),
    "sqr_r": (1, 1, U_FP, M_BASE, ("=2p",)),
    "mul_r1": (2, 2, U_FP, M_SCALAR, ("2p", "p")),
    "mul": (3, 2, U_FP, M_ALL, ("2p", "p")),
    "add_r": (4, 2, U_FP, M_BASE, ("2p", "2p")),
    "add_r2": (5, 2, U_FP, M_SCALAR, ("2p", "2p")),
    "dbl_r": (6, 1, U_FP, M_BASE, ("2p",)),
    "sub_r": (7, 2, U_FP, M_ALL, ("2p", "=2p")),
    "neg_r": (8, 1, U_FP, M_BASE, ("=2p",)),
    "sop2_r": (9, 4, U_FP, M_BASE, ("=2p", "=2p", "=2p", "=2p")),
    "sop2": (10, 4, U_FP, M_EXT, ("p", "p", "=6p", "p")),
    "reduce_2p": (11, 1, U_FP, M_BASE, ("4p",)),
    "is_zero_mod_p": (12, 1, U_FP, M_BASE, ("2p",)),
    "canonical": (13, 1, U_FP, M_ALL, ("=2p",)),
    "reduce_full": (14, 1, U_FP, M_EXT, ("=6p",)),
    "neg_beta_times_neg": (20, 1, U_FP2, M_EXT, ("=p",)),
    "fp2_mul": (21, 2, U_FP2, M_EXT, ("p", "p")),
    "fp2_sqr": (22, 1, U_FP2, M_EXT, ("p",)),
    "fp2_mul_karatsuba": (23, 2, U_FP2, M_EXT, ("p", "p")),
    "half_mul_r": (30, 2, U_HALF, M_EXT, ("=2p", "=2p")),
    "half_sqr_r": (31, 1, U_HALF, M_EXT, ("2p",)),
    "half_sop2_r": (32, 4, U_HALF, M_EXT, ("=2p", "=2p", "=2p", "=2p")),
    "half_beta_times": (33, 1, U_HALF, M_EXT, ("=2p",)),
    "half_neg_r": (34, 1, U_HALF, M_EXT, ("=2p",)),
    "half_is_zero_mod_p": (35, 1, U_HALF, M_EXT, ("2p",)),
    "half_is_zero": (36, 1, U_HALF, M_EXT, ("=2p",)),
    "half_canonical": (37, 1, U_HALF, M_EXT, ("=2p",)),
    "half_mul": (38, 2, U_HALF, M_EXT, ("=2p", "=2p")),
    "half_sqr": (39, 1, U_HALF, M_EXT, ("2p",)),
}
ACC_KIND = {"madd": 0, "add": 1, "canonical": 2}
# the header's host forms are bit-identical to the device for these; the products return canonical values on the host
HOST_EXACT = {"add_r", "add_r2", "dbl_r", "sub_r", "neg_r", "reduce_2p", "is_zero_mod_p", "canonical", "reduce_full",
              "neg_beta_times_neg", "mul", "sop2", "fp2_mul", "fp2_sqr", "fp2_mul_karatsuba"}


def ops_of(field, units=(U_FP, U_FP2, U_HALF)):
    return [n for n, r in TABLE.items() if (r[3] >> FIELD_ID[field]) & 1 and r[2] in units]


class Geo:
    """one field on N saturated 32-bit limbs; `fold` / `beta_2p` exist for the value-level mutants of the tests only"""

    def __init__(self, field, fold=None, beta_2p=True):
        self.field = field
        self.p = P.MODULI[field][0]
        self.N = 8 if self.p.bit_length() <= 256 else 12
        self.R = 1 << (32 * self.N)
        self.ninv = (-pow(self.p, -1, self.R)) % self.R
        self.rinv = pow(self.R, -1, self.p)
        self.one = self.R % self.p
        self.nb = NEG_BETA.get(field, 0)
        self.fold_override, self.beta_2p = fold, beta_2p

    # ---- limbs
    def words(self, x):
        need(0 <= x < self.R, "value does not fit %d limbs" % self.N)
        return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(self.N)]

    def from_words(self, w):
        return sum(int(v) << (32 * i) for i, v in enumerate(w))

    def cmax(self, cls):
        p = self.p
        return {"p": p - 1, "=p": p, "2p": 2 * p - 1, "=2p": 2 * p, "4p": 4 * p - 1, "=6p": 6 * p}[cls]

    def mont(self, s):
        """(s + m p) / R, m = s (-p^-1) mod R: what N columns of an interleaved reduction leave; it must fit the N limbs"""
        m = (s * self.ninv) % self.R
        t = (s + m * self.p) // self.R
        need(t < self.R, "reduced value does not fit N limbs")
        return t

    # ---- Fp (fp.cuh)
    def reduce_once(self, t):
        need(t < self.R, "reduce_once: N limbs")
        return t - self.p if t >= self.p else t

    def reduce_2p(self, t):                               # fp.cuh:473  t (< 4p)
        need(4 * self.p <= self.R and 0 <= t < 4 * self.p, "reduce_2p: t < 4p <= R")
        return t - 2 * self.p if t >= 2 * self.p else t

    def mul_r(self, a, b):                                # fp.cuh:453-458  operands <= 2p (neg_r's 2p is an operand), 4p <= R
        need(4 * self.p <= self.R, "mul_r: 4p <= R")
        need(0 <= a <= 2 * self.p and 0 <= b <= 2 * self.p, "mul_r: operands <= 2p")
        return self.mont(a * b)

    def sqr_r(self, a):
        return self.mul_r(a, a)

    def mul_r1(self, a, b):                               # fp.cuh:552  relaxed a (< 2p) times canonical b (< p), p < R/2
        need(2 * self.p < self.R and 0 <= a < 2 * self.p and 0 <= b < self.p, "mul_r1: a < 2p, b < p")
        return self.mont(a * b)

    def mul(self, a, b):                                  # fp.cuh:404, fed a relaxed a at fft.cuh:390: t < 2p, one subtraction
        need(0 <= a < 2 * self.p and 0 <= b < self.p, "mul: a < 2p, b < p")
        t = self.mont(a * b)
        need(t < 2 * self.p, "mul: t < 2p before reduce_once")
        return self.reduce_once(t)

    def add_r(self, a, b):                                # fp.cuh:489
        need(0 <= a < 2 * self.p and 0 <= b < 2 * self.p, "add_r: operands < 2p")
        return self.reduce_2p(a + b)

    def dbl_r(self, a):
        need(0 <= a < 2 * self.p, "dbl_r: operand < 2p")
        return self.reduce_2p(2 * a)

    def sub_r(self, a, b):                                # fp.cuh:507  a - b (+ 2p if negative); 2p fits N limbs.  b = 2p occurs:
        # the y of an accumulator that a first madd set to y2 = neg_r(0) (a zero component of a base's y over Fp2)
        need(2 * self.p < self.R and 0 <= a < 2 * self.p and 0 <= b <= 2 * self.p, "sub_r: a < 2p, b <= 2p")
        return a - b if a >= b else a - b + 2 * self.p

    def add_r2(self, a, b):                               # fp.cuh:528-530  4p may exceed R; a carry-out means >= 2p
        need(2 * self.p < self.R and 0 <= a < 2 * self.p and 0 <= b < 2 * self.p, "add_r2: operands < 2p")
        t = a + b
        return t if t < 2 * self.p else t - 2 * self.p

    def neg_r(self, a):                                   # fp.cuh:566  a <= 2p -> 2p - a in [0, 2p]
        need(2 * self.p < self.R and 0 <= a <= 2 * self.p, "neg_r: operand <= 2p")
        return 2 * self.p - a

    def sop2_r(self, a, b, c, d):                         # fp.cuh:579-582  all <= 2p
        need(4 * self.p <= self.R and all(0 <= v <= 2 * self.p for v in (a, b, c, d)), "sop2_r: operands <= 2p")
        t = self.mont(a * b + c * d)
        return t if 8 * self.p <= self.R else self.reduce_2p(t)

    def sop4_r(self, fold, pairs, apply_fold=None):       # fp.cuh:602-605  sum <= R p (no fold) or <= 3 R p (fold)
        s = sum(x * y for x, y in pairs)
        need(all(0 <= v < self.R for xy in pairs for v in xy), "sop4_r: N-limb operands")
        need(s <= (3 if fold else 1) * self.R * self.p, "sop4_r: sum of products <= %s R p" % (3 if fold else 1))
        t = self.mont(s)
        return self.reduce_2p(t) if (fold if apply_fold is None else apply_fold) else t

    def sop2(self, a, b, c2, d):                          # fp.cuh:624-626  a, b, d < p; c2 any N-limb value up to 6p
        need(all(0 <= v < self.p for v in (a, b, d)) and 0 <= c2 <= 6 * self.p and c2 < self.R, "sop2: a, b, d < p, c2 <= 6p")
        t = self.mont(a * b + c2 * d)
        need(t < 2 * self.p, "sop2: t < 2p before reduce_once")
        return self.reduce_once(t)

    def reduce_full(self, a):                             # fp.cuh:639  up to 8 subtractions of p
        need(0 <= a < self.R and a // self.p <= 8, "reduce_full: a small multiple of p")
        return a % self.p

    def is_zero_mod_p(self, a):                           # fp.cuh:657  relaxed value (< 2p: a sub_r result): 0 or p
        need(0 <= a < 2 * self.p, "is_zero_mod_p: relaxed value < 2p")
        return int(a == 0 or a == self.p)

    def canonical(self, a):                               # fp.cuh:667-669  [0, 2p] -> [0, p), two conditional subtractions
        need(0 <= a <= 2 * self.p and 2 * self.p < self.R, "canonical: relaxed value <= 2p")
        return self.reduce_once(self.reduce_once(a))

    # ---- Fp2 on one lane, canonical components (fp.cuh:733-837)
    def neg_beta_times_neg(self, x):                      # fp.cuh:771-773  NEG_BETA (p - x)
        need(self.nb and 0 <= x <= self.p, "neg_beta_times_neg: x <= p")
        r = self.nb * (self.p - x)
        need(r < self.R, "NEG_BETA p fits N limbs")
        return r

    def fp2_mul(self, a, b):                              # fp.cuh:800
        return (self.sop2(a[0], b[0], self.neg_beta_times_neg(a[1]), b[1]), self.sop2(a[0], b[1], a[1], b[0]))

    def _c(self, v):
        return v % self.p

    def fp2_mul_karatsuba(self, a, b):                    # fp.cuh:806  canonical arithmetic throughout
        need(all(0 <= v < self.p for v in a + b), "Fp2: canonical components")
        v0, v1 = self.mul(a[0], b[0]), self.mul(a[1], b[1])
        s = self.mul(self._c(a[0] + a[1]), self._c(b[0] + b[1]))
        return (self._c(v0 - self.nb * v1), self._c(s - v0 - v1))

    def fp2_sqr(self, a):                                 # fp.cuh:815
        need(all(0 <= v < self.p for v in a), "Fp2: canonical components")
        t = self.mul(a[0], a[1])
        s = self.mul(self._c(a[0] + a[1]), self._c(a[0] - self.nb * a[1]))
        return (self._c(s + (self.nb - 1) * t), self._c(2 * t))

    # ---- Fp2Half: even lane c0, odd lane c1 (fp.cuh:849-985)
    def beta_times(self, x):                              # fp.cuh:887-888  NEG_BETA (2p - x) for a relaxed x
        need(self.nb and 0 <= x <= 2 * self.p, "beta_times: x <= 2p")
        if not self.beta_2p:
            return (self.nb * (self.p - x)) % self.R      # (the tests' mutant: p - x wraps for x > p)
        r = self.nb * self.neg_r(x)
        need(r < self.R, "2 NEG_BETA p fits N limbs")
        return r

    def half_fold(self):
        return (8 + 8 * self.nb) * self.p > self.R        # fp.cuh:923-925

    def half_mul_r(self, a, b):                           # fp.cuh:905-907: B::sop2_r with a beta_times operand
        need(8 * self.p <= self.R and all(0 <= v <= 2 * self.p for v in a + b), "Fp2Half::mul_r: components <= 2p, 8p <= R")
        return (self.sop4_r(False, [(a[0], b[0]), (self.beta_times(a[1]), b[1])]),
                self.sop4_r(False, [(a[0], b[1]), (a[1], b[0])]))

    def half_sop2_r(self, a, b, c, d):                    # fp.cuh:921-924
        need(all(0 <= v <= 2 * self.p for v in a + b + c + d), "Fp2Half::sop2_r: components <= 2p")
        f, m = self.half_fold(), self.fold_override       # (m: the tests' mutant, the same contract with the fold left out)
        return (self.sop4_r(f, [(a[0], b[0]), (self.beta_times(a[1]), b[1]), (c[0], d[0]), (self.beta_times(c[1]), d[1])], m),
                self.sop4_r(f, [(a[0], b[1]), (a[1], b[0]), (c[0], d[1]), (c[1], d[0])], m))

    def half_sqr_r(self, a):                              # fp.cuh:940-943
        need(all(0 <= v < 2 * self.p for v in a), "Fp2Half::sqr_r: components < 2p")
        sm = self.add_r(a[0], a[1])
        wide = a[0] + self.beta_times(a[1])               # unreduced, a product operand only
        need(wide < self.R, "a0 + beta a1 fits N limbs")
        s = self.sop4_r(False, [(sm, wide)])              # B::mul_r on a wide operand: its sum bound, not its operand class
        t = self.sop4_r(False, [(a[0], a[1])])
        even = s if self.nb == 1 else self.add_r(s, self.dbl_r(self.dbl_r(t)))
        return (even, self.dbl_r(t))

    def half_neg_r(self, a):
        return (self.neg_r(a[0]), self.neg_r(a[1]))

    def half_canonical(self, a):
        return (self.canonical(a[0]), self.canonical(a[1]))

    def half_mul(self, a, b):
        return self.half_canonical(self.half_mul_r(a, b))

    def half_sqr(self, a):
        return self.half_canonical(self.half_sqr_r(a))


GEO = {f: Geo(f) for f in P.FIELD_ORDER}


# ---- one row through the model -------------------------------------------------------------------------------------------------
def apply_fp(g, name, v):
    """Fp op on one lane: operand values -> (result value, flag)"""
    if name == "is_zero_mod_p":
        return 0, g.is_zero_mod_p(v[0])
    return getattr(g, name)(*v), 0


def apply_pair(g, name, e):
    """Fp2 / Fp2Half op on one element: operands as (c0, c1) -> ((c0, c1) result, flag)"""
    if name == "neg_beta_times_neg":
        return (g.neg_beta_times_neg(e[0][0]), g.neg_beta_times_neg(e[0][1])), 0
    if name == "half_beta_times":
        return (g.beta_times(e[0][0]), g.beta_times(e[0][1])), 0
    if name == "half_is_zero_mod_p":
        return (0, 0), int(g.is_zero_mod_p(e[0][0]) and g.is_zero_mod_p(e[0][1]))
    if name == "half_is_zero":
        need(all(0 <= v <= 2 * g.p for v in e[0]), "is_zero: relaxed value")
        return (0, 0), int(e[0] == (0, 0))
    return getattr(g, name)(*e), 0


def closure_bound(g, name):
    """the documented output class: the largest value the op may return"""
    p = g.p
    if name in ("mul", "sop2", "canonical", "reduce_full", "fp2_mul", "fp2_sqr", "fp2_mul_karatsuba", "half_canonical", "half_mul",
                "half_sqr"):
        return p - 1
    if name in ("neg_r", "half_neg_r"):
        return 2 * p
    if name == "neg_beta_times_neg":
        return g.nb * p
    if name == "half_beta_times":
        return g.nb * 2 * p
    if name in ("is_zero_mod_p", "half_is_zero_mod_p", "half_is_zero"):
        return 0
    return 2 * p - 1


def want_residue(g, name, v):
    """the residue mod p (Fp2: the pair) the result must represent, from the definition of the operation"""
    p, ri, nb = g.p, g.rinv, g.nb
    f2 = P.Fld(p, -nb) if nb else None
    m2 = lambda a, b: tuple(c * ri % p for c in f2.mul((a[0] % p, a[1] % p), (b[0] % p, b[1] % p)))
    if name in ("mul_r", "mul_r1", "mul"):
        return v[0] * v[1] * ri % p
    if name == "sqr_r":
        return v[0] * v[0] * ri % p
    if name in ("add_r", "add_r2"):
        return (v[0] + v[1]) % p
    if name == "dbl_r":
        return 2 * v[0] % p
    if name == "sub_r":
        return (v[0] - v[1]) % p
    if name == "neg_r":
        return -v[0] % p
    if name in ("sop2_r", "sop2"):
        return (v[0] * v[1] + v[2] * v[3]) * ri % p
    if name in ("reduce_2p", "canonical", "reduce_full"):
        return v[0] % p
    if name in ("neg_beta_times_neg", "half_beta_times"):
        return tuple(-nb * c % p for c in v[0])
    if name in ("fp2_mul", "fp2_mul_karatsuba", "half_mul_r", "half_mul"):
        return m2(v[0], v[1])
    if name in ("fp2_sqr", "half_sqr_r", "half_sqr"):
        return m2(v[0], v[0])
    if name == "half_sop2_r":
        return f2.add(m2(v[0], v[1]), m2(v[2], v[3]))
    if name == "half_neg_r":
        return tuple(-c % p for c in v[0])
    if name == "half_canonical":
        return tuple(c % p for c in v[0])
    raise KeyError(name)


def check_row(g, name, v, res, flag):
    """(b) residue and (c) closure of ONE result -- the model's own or the device's -- for operands v; raises AssertionError"""
    pair = TABLE[name][2] != U_FP
    comps = res if pair else (res,)
    bound = closure_bound(g, name)
    assert all(0 <= c <= bound for c in comps), "%s %s: result %s leaves its class (<= %x) for %s" % (g.field, name, comps, bound, v)
    if name == "is_zero_mod_p":
        assert flag == int(v[0] % g.p == 0), (g.field, name, v)
    elif name in ("half_is_zero_mod_p", "half_is_zero"):
        z = all(c % g.p == 0 for c in v[0])
        assert flag == int(z if name == "half_is_zero_mod_p" else v[0] == (0, 0)), (g.field, name, v)
    else:
        want = want_residue(g, name, v)
        got = tuple(c % g.p for c in comps) if pair else res % g.p
        assert got == want, "%s %s: residue %s, wanted %s, for %s" % (g.field, name, got, want, v)


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def edges(g, cls):
    """the deterministic edge list of an operand class, most telling values first"""
    p, M, s = g.p, g.cmax(cls), 32 * (g.N - 1)
    low = (1 << s) - 1
    top = ((M + 1) >> s) - 1                                  # the largest top limb under which all-ones low limbs stay in class
    cand = [M, 0, p, 2 * p - 1, (top << s) | low if top >= 0 else low, 1, p - 1, p + 1, 2 * p, g.one, low,
            2 * p + 1, M - 1] + [0xFFFFFFFF << (32 * i) for i in range(g.N)]
    out = []
    for v in cand:
        if 0 <= v <= M and v not in out:
            out.append(v)
    return out


def _cross(lists, cap):
    """the full cross product where it has at most `cap` rows; otherwise the cross product of the longest prefixes (the edge
    lists put the most telling values first) that fits, plus every value of every operand against the others at their maxima"""
    total = 1
    for l in lists:
        total *= len(l)
    if total <= cap:
        k = max(len(l) for l in lists)
    else:
        k = 2
        while (k + 1) ** len(lists) <= cap:
            k += 1
    rows = [[]]
    for l in lists:
        rows = [r + [v] for r in rows for v in l[:k]]
    if total > cap:
        for i, l in enumerate(lists):
            for v in l[k:]:
                rows.append([m[0] if j != i else v for j, m in enumerate(lists)])
                rows.append([m[1] if j != i else v for j, m in enumerate(lists)])
    return rows


def directed_pairs(g, name):
    """sums and differences placed exactly on the decisions of add_r / add_r2 / sub_r"""
    p, R = g.p, g.R
    hi = 2 * p - 1
    rows = []
    if name in ("add_r", "add_r2"):
        for S in (2 * p - 1, 2 * p, 2 * p + 1, R - 1, R, R + 1, 4 * p - 2):
            if S > 2 * hi or (name == "add_r" and S >= 4 * p):
                continue   # the field does not admit it (R - 1 .. R + 1 as a sum of two relaxed values: BLS12-381 Fr only)
            for a in (S // 2, min(S, hi), max(S - hi, 0), p if 0 <= S - p <= hi else S // 2, (S + 1) // 2):
                rows += [[a, S - a], [S - a, a]]
    if name == "sub_r":
        for D in (0, 1, p, hi):
            for b in (0, 1, p - 1, p, hi - D):
                if 0 <= b and b + D <= hi:
                    rows += [[b + D, b], [b, b + D]]      # a - b = D and a - b = -D
    return rows


def vectors(field, name, nrand, seed=11, cap=8192):
    """operand rows of one op: Fp ops -> [values per lane]; pair ops -> [(c0, c1) per operand] per ELEMENT"""
    g = GEO[field]
    op, arity, unit, _, classes = TABLE[name]
    rng = random.Random("%s/%s/%d" % (field, name, seed))
    slots = [edges(g, c) for c in classes for _ in range(1 if unit == U_FP else 2)]
    rows = _cross(slots, cap) + directed_pairs(g, name)
    if name == "reduce_2p":
        rows += [[t] for t in (2 * g.p - 1, 2 * g.p, 2 * g.p + 1, 4 * g.p - 1)]
    bounds = [g.cmax(c) for c in classes for _ in range(1 if unit == U_FP else 2)]
    for i in range(nrand):
        row = [rng.randrange(b + 1) for b in bounds]
        if name in ("is_zero_mod_p", "half_is_zero_mod_p", "half_is_zero") and i % 4 == 0:
            row = [rng.choice((0, g.p)) for _ in bounds]   # random rows would never be zero: every 0 / p pattern, and near misses
            if i % 16 == 0:
                row[rng.randrange(len(row))] ^= 1 << rng.randrange(32 * g.N - 8)
        rows.append(row)
    if unit == U_FP:
        return rows
    return [[(r[2 * j], r[2 * j + 1]) for j in range(arity)] for r in rows]


def expected(field, name, rows, g=None):
    """[(result, flag)] per row; OutOfContract on a row outside the op's precondition.  Every result is checked for residue and
    closure against the op's definition: the reference alone stays inside every contract"""
    g = g or GEO[field]
    f = apply_fp if TABLE[name][2] == U_FP else apply_pair
    out = []
    for r in rows:
        res, flag = f(g, name, r)
        check_row(g, name, r, res, flag)
        out.append((res, flag))
    return out


@functools.lru_cache(maxsize=None)
def case(field, name, nrand):
    """(rows, expected) of one (field, op): built once per session, shared by every test that needs them, never modified"""
    rows = vectors(field, name, nrand)
    return rows, expected(field, name, rows)


def rows_to_array(field, name, rows):
    """lane rows of u32 words as ark_hip_test_relaxed_raw_op reads them (pair ops: even lane c0 slots, odd lane c1 slots)"""
    g = GEO[field]
    lanes = []
    for r in rows:
        if TABLE[name][2] == U_FP:
            lanes.append([w for v in r for w in g.words(v)])
        else:
            lanes.append([w for e in r for w in g.words(e[0])])
            lanes.append([w for e in r for w in g.words(e[1])])
    return np.array(lanes, dtype=np.uint64).astype(np.uint32)


def expected_to_array(field, name, exp):
    g = GEO[field]
    lanes = []
    for res, flag in exp:
        for c in (res if TABLE[name][2] != U_FP else (res,)):
            lanes.append(g.words(c) + [flag])
    return np.array(lanes, dtype=np.uint64).astype(np.uint32)


def array_to_results(field, name, arr):
    """device / host output words -> [(result, flag)] in the shape of `expected`"""
    g = GEO[field]
    vals = [(g.from_words(r[:g.N]), int(r[g.N])) for r in np.asarray(arr).tolist()]
    if TABLE[name][2] == U_FP:
        return vals
    assert len(vals) % 2 == 0
    out = []
    for i in range(0, len(vals), 2):
        assert vals[i][1] == vals[i + 1][1], "pair-uniform flag differs between the lanes of pair %d" % (i // 2)
        out.append(((vals[i][0], vals[i + 1][0]), vals[i][1]))
    return out


# ---- the XYZZ additions of ec.cuh on relaxed residues ---------------------------------------------------------------------------
class _FpOps:
    """F = Fp<P>: elements are integers"""

    def __init__(self, g):
        self.g, self.ext = g, 1
        for n in ("mul_r", "sqr_r", "sub_r", "dbl_r", "neg_r", "sop2_r", "canonical"):
            setattr(self, n, getattr(g, n))
        self.one, self.zero = g.one, 0

    def is_zero(self, a):
        return a == 0

    def is_zero_mod_p(self, a):
        return bool(self.g.is_zero_mod_p(a))

    def comps(self, a):
        return (a,)

    # canonical arithmetic (the doubling branch): operands < p, unique results
    def cmul(self, a, b):
        return self.g.mul(a, b)

    def cadd(self, a, b):
        need(a < self.g.p and b < self.g.p, "canonical add")
        return (a + b) % self.g.p

    def csub(self, a, b):
        need(a < self.g.p and b < self.g.p, "canonical sub")
        return (a - b) % self.g.p


class _HalfOps:
    """F = Fp2Half<P, NEG_BETA>: elements are (c0, c1)"""

    def __init__(self, g):
        self.g, self.ext = g, 2
        self.mul_r, self.sqr_r, self.sop2_r = g.half_mul_r, g.half_sqr_r, g.half_sop2_r
        self.neg_r, self.canonical = g.half_neg_r, g.half_canonical
        self.one, self.zero = (g.one, 0), (0, 0)

    def sub_r(self, a, b):
        return (self.g.sub_r(a[0], b[0]), self.g.sub_r(a[1], b[1]))

    def dbl_r(self, a):
        return (self.g.dbl_r(a[0]), self.g.dbl_r(a[1]))

    def is_zero(self, a):
        return a == (0, 0)

    def is_zero_mod_p(self, a):
        return bool(self.g.is_zero_mod_p(a[0]) and self.g.is_zero_mod_p(a[1]))

    def comps(self, a):
        return a

    def cmul(self, a, b):                                  # Fp2Half::mul = mul_r + canonical
        return self.g.half_mul(a, b)

    def cadd(self, a, b):
        need(all(v < self.g.p for v in a + b), "canonical add")
        return ((a[0] + b[0]) % self.g.p, (a[1] + b[1]) % self.g.p)

    def csub(self, a, b):
        need(all(v < self.g.p for v in a + b), "canonical sub")
        return ((a[0] - b[0]) % self.g.p, (a[1] - b[1]) % self.g.p)


class AccModel:
    """XYZZ accumulators (x, y, zz, zzz) of raw limb values over F = C::FA, and the three functions of ec.cuh on them"""

    def __init__(self, curve, g=None):
        self.curve, self.cid = curve, P.CURVE_ORDER.index(curve)
        self.C = P.Curve(curve)
        bf, _, self.ext, _, _ = P.CURVE_PARAMS[curve]
        self.g = g or GEO[bf]
        self.F = _FpOps(self.g) if self.ext == 1 else _HalfOps(self.g)
        self.trace = None   # (P, R) of the last addition that computed them

    def infinity(self):
        F = self.F
        return (F.one, F.one, F.zero, F.zero)

    def _mdbl(self, x1, y1):                               # ec.cuh:155-170, canonical arithmetic
        F = self.F
        u = F.cadd(y1, y1)
        v = F.cmul(u, u)
        w = F.cmul(u, v)
        s = F.cmul(x1, v)
        xx = F.cmul(x1, x1)
        m = F.cadd(F.cadd(xx, xx), xx)
        x3 = F.csub(F.cmul(m, m), F.cadd(s, s))
        y3 = F.csub(F.cmul(m, F.csub(s, x3)), F.cmul(w, y1))
        return x3, y3, v, w

    def _dbl(self, a):                                     # ec.cuh:172-188
        F = self.F
        if F.is_zero(a[2]):
            return a
        x3, y3, v, w = self._mdbl(a[0], a[1])
        return (x3, y3, F.cmul(v, a[2]), F.cmul(w, a[3]))

    def canonical(self, a):                                # ec.cuh:246-250
        F = self.F
        if F.is_zero(a[2]):
            return self.infinity()
        return tuple(F.canonical(c) for c in a)

    def _tail(self, x1, y1, zz, zzz, p, r):
        F = self.F
        pp = F.sqr_r(p)
        ppp = F.mul_r(p, pp)
        q = F.mul_r(x1, pp)
        x3 = F.sub_r(F.sub_r(F.sqr_r(r), ppp), F.dbl_r(q))
        y3 = F.sop2_r(r, F.sub_r(q, x3), F.neg_r(y1), ppp)
        return (x3, y3, F.mul_r(zz, pp), F.mul_r(zzz, ppp))

    def madd(self, acc, x2, y2):                           # ec.cuh:216-245  x2 canonical, y2 canonical or 2p - y
        F, g = self.F, self.g
        need(all(c < g.p for c in F.comps(x2)) and all(c <= 2 * g.p for c in F.comps(y2)), "madd: x2 canonical, y2 <= 2p")
        self._state_ok(acc)
        if F.is_zero(acc[2]):
            return (x2, y2, F.one, F.one)
        p = F.sub_r(F.mul_r(x2, acc[2]), acc[0])
        r = F.sub_r(F.mul_r(y2, acc[3]), acc[1])
        self.trace = (p, r)
        if F.is_zero_mod_p(p):
            return self._mdbl(x2, F.canonical(y2)) if F.is_zero_mod_p(r) else self.infinity()
        return self._tail(acc[0], acc[1], acc[2], acc[3], p, r)

    def add(self, acc, b):                                 # ec.cuh:279-311
        F = self.F
        self._state_ok(acc)
        self._state_ok(b)
        if F.is_zero(b[2]):
            return acc
        if F.is_zero(acc[2]):
            return b
        u1, u2 = F.mul_r(acc[0], b[2]), F.mul_r(b[0], acc[2])
        s1, s2 = F.mul_r(acc[1], b[3]), F.mul_r(b[1], acc[3])
        p, r = F.sub_r(u2, u1), F.sub_r(s2, s1)
        self.trace = (p, r)
        if F.is_zero_mod_p(p):
            return self._dbl(self.canonical(acc)) if F.is_zero_mod_p(r) else self.infinity()
        return self._tail(u1, s1, F.mul_r(acc[2], b[2]), F.mul_r(acc[3], b[3]), p, r)

    def _state_ok(self, a):
        """a relaxed accumulator: every coordinate below 2p; zz = 0 exactly only at infinity (never p: a valid point has
        zz != 0 mod p); a first madd leaves y = y2 <= 2p"""
        F, g = self.F, self.g
        need(all(c < 2 * g.p for i in (0, 2, 3) for c in F.comps(a[i])) and all(c <= 2 * g.p for c in F.comps(a[1])),
             "accumulator coordinate outside the relaxed class")
        need(F.is_zero(a[2]) or any(c % g.p for c in F.comps(a[2])), "zz = 0 mod p in a representative other than 0")

    def apply(self, kind, acc, other):
        if kind == "madd":
            return self.madd(acc, other[0], other[1])
        if kind == "add":
            return self.add(acc, other)
        return self.canonical(acc)

    # ---- interpretation
    def elem(self, a):
        """raw limbs -> the field element of pyref (standard form)"""
        g = self.g
        return a * g.rinv % g.p if self.ext == 1 else (a[0] * g.rinv % g.p, a[1] * g.rinv % g.p)

    def raw(self, e, j=0):
        """pyref element -> Montgomery limbs + j p per component (j an int or one per component)"""
        g = self.g
        if self.ext == 1:
            return e * g.R % g.p + j * g.p
        js = j if isinstance(j, tuple) else (j, j)
        return (e[0] * g.R % g.p + js[0] * g.p, e[1] * g.R % g.p + js[1] * g.p)

    def affine(self, a):
        Fd = self.C.F
        zz, zzz = self.elem(a[2]), self.elem(a[3])
        if zz == Fd.zero():
            return None
        return (Fd.mul(self.elem(a[0]), Fd.inv(zz)), Fd.mul(self.elem(a[1]), Fd.inv(zzz)))

    def consistent(self, a):
        Fd = self.C.F
        zz, zzz = self.elem(a[2]), self.elem(a[3])
        return Fd.mul(Fd.mul(zz, zz), zz) == Fd.mul(zzz, zzz)

    def closed(self, a):
        """every coordinate below 2p: a legal operand of the next addition"""
        return all(c < 2 * self.g.p for co in a for c in self.F.comps(co))

    def state(self, pt, z, js):
        """the XYZZ of affine pt with ZZ = z^2, ZZZ = z^3, coordinate i as value + js[i] p"""
        Fd = self.C.F
        zz = Fd.mul(z, z)
        zzz = Fd.mul(zz, z)
        return (self.raw(Fd.mul(pt[0], zz), js[0]), self.raw(Fd.mul(pt[1], zzz), js[1]), self.raw(zz, js[2]), self.raw(zzz, js[3]))

    def words(self, a):
        return [w for co in a for c in self.F.comps(co) for w in self.g.words(c)]

    def from_words(self, w):
        n = self.g.N
        v = [self.g.from_words(w[i * n:(i + 1) * n]) for i in range(4 * self.ext)]
        return tuple(v) if self.ext == 1 else tuple((v[2 * i], v[2 * i + 1]) for i in range(4))

    def other_words(self, kind, o):
        if kind == "madd":
            return [w for co in o for c in self.F.comps(co) for w in self.g.words(c)]
        return self.words(o)


def sqrt_mod(a, p):
    """a square root of a mod p, or None (Tonelli-Shanks)"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) == 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


def point_with_zero_y_component(C):
    """a point of the curve over Fp2 whose y has a ZERO component (the curve's, not necessarily the subgroup's: the addition
    formulas do not care): choose x1, solve Im(x^3 + b) = 0 for x0 (a square root in Fp), then x^3 + b = w is in Fp and y is
    (sqrt w, 0) or (0, sqrt(w / beta)), beta being a non-residue"""
    p, beta, (b0, b1) = C.p, C.F.beta, C.b
    for x1 in range(1, 200):
        x0 = sqrt_mod(-(beta * x1 ** 3 + b1) * pow(3 * x1, -1, p), p)
        if x0 is None:
            continue
        w = (x0 ** 3 + 3 * beta * x0 * x1 * x1 + b0) % p
        y0 = sqrt_mod(w, p)
        y = (y0, 0) if y0 is not None else (0, sqrt_mod(w * pow(beta, -1, p), p))
        pt = ((x0, x1), y)
        assert C.on_curve(pt)
        return pt
    raise AssertionError("no such point found")


def _rand_z(A, rng):
    e = lambda: rng.randrange(1, A.g.p)
    return e() if A.ext == 1 else (e(), e())


def _js_list(A, rng, count):
    """representative choices: every coordinate canonical, every coordinate value + p, then mixed ones"""
    n = A.ext
    one = lambda j: j if n == 1 else (j, j)
    out = [tuple(one(0) for _ in range(4)), tuple(one(1) for _ in range(4))]
    for _ in range(count):
        out.append(tuple(rng.randrange(2) if n == 1 else (rng.randrange(2), rng.randrange(2)) for _ in range(4)))
    return out


def base_forms(A, B):
    """the two operand forms of an affine base B: (x, y) canonical, and (x, 2p - y') with y' = -y canonical (F::neg_r of the
    negated base, msm.cuh:967) -- a zero component of y' becomes 2p"""
    x, y = A.raw(B[0]), A.raw(B[1])
    yn = A.raw(A.C.F.neg(B[1]))
    return [(x, y), (x, A.F.neg_r(yn))]


def acc_edge_cases(A, G, seed=3):
    """-> [(kind, acc, other, expected affine point, tag)]: every branch, with the accumulator's coordinates value + j p"""
    C, rng = A.C, random.Random("%s/%d" % (A.curve, seed))
    pts = {k: C.mul(G, k) for k in (2, 3, 5, 7)}
    cases = []
    accs = {ka: [A.state(pts[ka], z, js) for z in (_rand_z(A, rng), A.C.F.from_int(1)) for js in _js_list(A, rng, 3)] for ka in (3, 7)}
    for ka in (3, 7):
        pa = pts[ka]
        for acc in accs[ka]:
            for B, tag in ((pts[5], "other"), (C.neg(pts[5]), "other"), (pa, "equal"), (C.neg(pa), "inverse")):
                for form in base_forms(A, B):
                    cases.append(("madd", acc, form, C.add(pa, B), tag))
            for kb, sign in ((2, 1), (ka, 1), (ka, -1)):
                pb = pts[kb] if sign > 0 else C.neg(pts[kb])
                for js in _js_list(A, rng, 1):
                    cases.append(("add", acc, A.state(pb, _rand_z(A, rng), js), C.add(pa, pb),
                                  "other" if kb != ka else "equal" if sign > 0 else "inverse"))
            cases.append(("add", acc, A.infinity(), pa, "operand at infinity"))
            cases.append(("canonical", acc, None, pa, "canonical"))
    for k in (2, 5):
        for form in base_forms(A, pts[k]):
            cases.append(("madd", A.infinity(), form, pts[k], "from infinity"))
        cases.append(("add", A.infinity(), accs[3][1], pts[3], "from infinity"))
    cases.append(("add", A.infinity(), A.infinity(), None, "from infinity"))
    cases.append(("canonical", A.infinity(), None, None, "canonical"))
    if A.ext == 2:
        B0 = point_with_zero_y_component(C)
        for acc in accs[3][:3]:
            for B in (B0, C.neg(B0)):
                for form in base_forms(A, B):
                    cases.append(("madd", acc, form, C.add(pts[3], B), "zero component"))
        for js in _js_list(A, rng, 2):       # the accumulator IS that point: the doubling and the inverse through it
            acc = A.state(B0, _rand_z(A, rng), js)
            for B, tag in ((B0, "equal"), (C.neg(B0), "inverse")):
                for form in base_forms(A, B):
                    cases.append(("madd", acc, form, C.add(B0, B), tag))
    return cases


def acc_chain(A, G, lanes, steps, seed=4):
    """-> (start states, their multiples of G, [(kind, [operand per lane], [operand multiple per lane])], pt): `steps` mixed
    madd / add steps per lane; operands are small multiples of G, often the accumulated point or its inverse"""
    C, rng = A.C, random.Random("%s/chain/%d" % (A.curve, seed))
    cache = {}

    def pt(m):
        if m not in cache:
            cache[m] = C.mul(G, m % C.r) if m % C.r else None
        return cache[m]

    starts, mult = [], []
    for i in range(lanes):
        m = 2 + i if i else 0
        starts.append(A.state(pt(m), _rand_z(A, rng), _js_list(A, rng, 1)[1 + i % 2]) if m else A.infinity())
        mult.append(m)
    sched, cur = [], list(mult)
    for _ in range(steps):
        kind = rng.choice(("madd", "add", "madd"))
        ops, ms = [], []
        for i in range(lanes):
            r = rng.randrange(6)
            m = cur[i] if r == 0 else -cur[i] if r == 1 else rng.randrange(1, 9) * (1 if r < 4 else -1)
            if kind == "madd":
                if m % C.r == 0:
                    m = 1
                ops.append(base_forms(A, pt(m))[rng.randrange(2)])
            else:
                ops.append(A.infinity() if m % C.r == 0 else A.state(pt(m), _rand_z(A, rng), _js_list(A, rng, 1)[rng.randrange(3)]))
                if m % C.r == 0:
                    m = 0
            ms.append(m)
            cur[i] += m
        sched.append((kind, ops, ms))
    return starts, mult, sched, pt


# ---- THE TABLE OF DOCUMENTED BOUNDS --------------------------------------------------------------------------------------------
# (file:line, the words of the comment or assertion that must still stand on that line, fields, exact re-derivation from p).
# tests/test_relaxed_model_host.py checks that the line still says so and that the derivation holds on every field named.
BASE = ("BN254_FQ", "BLS12_381_FQ", "BLS12_377_FQ")
EXT = ("BLS12_381_FQ", "BLS12_377_FQ")
SCALAR = ("BN254_FR", "BLS12_381_FR", "BLS12_377_FR")


def _top(g):
    return g.p >> (32 * (g.N - 1))


def _ratio(g, digits):
    return round(g.p / g.R, digits)


DOCUMENTED = [
    ("fp.cuh:453", "4p <= 2^(32N)", BASE, lambda g: 4 * g.p <= g.R),
    ("fp.cuh:453", "p/R = 0.10, 0.007, 0.19", BASE,
     lambda g: {"BLS12_381_FQ": _ratio(g, 2) == 0.10, "BLS12_377_FQ": _ratio(g, 3) == 0.007, "BN254_FQ": _ratio(g, 2) == 0.19}[g.field]),
    ("fp.cuh:455", "(a b + m p)/R < p (4p/R + 1) <= 2p", BASE, lambda g: (4 * g.p * g.p + (g.R - 1) * g.p) // g.R < 2 * g.p),
    ("fp.cuh:459", "(P::P[N - 1] >> 30) == 0", BASE, lambda g: (_top(g) >> 30) == 0 and ((_top(g) >> 30) == 0) == (4 * g.p < g.R)),
    ("fp.cuh:528", "BLS12-381 Fr: p = 0.45 R", ("BLS12_381_FR",), lambda g: _ratio(g, 2) == 0.45 and 4 * g.p > g.R and 2 * g.p < g.R),
    ("fp.cuh:529", "it is then certainly >= 2p", SCALAR, lambda g: g.R >= 2 * g.p and (4 * g.p - 2) - 2 * g.p < g.R),
    ("fp.cuh:552", "(2p^2 + R p) / R < 2p for every p < R/2", SCALAR + BASE,
     lambda g: 2 * g.p < g.R and ((2 * g.p - 1) * (g.p - 1) + (g.R - 1) * g.p) // g.R < 2 * g.p),
    ("fp.cuh:579", "(8p^2 + m p)/R < p (8p/R + 1)", BASE, lambda g: (8 * g.p * g.p + (g.R - 1) * g.p) // g.R < 4 * g.p),
    ("fp.cuh:580", "already < 2p when 8p <= R (BLS12-381, BLS12-377); otherwise (BN254: < 2.6p)", BASE,
     lambda g: ((8 * g.p <= g.R) == (g.field != "BN254_FQ")) and ((_top(g) >> 29 == 0) == (8 * g.p <= g.R))
     and (8 * g.p * g.p + (g.R - 1) * g.p) * 10 < (20 if 8 * g.p <= g.R else 26) * g.p * g.R),
    ("fp.cuh:603", "FOLD = false: sum <= R p, result < 2p as it stands; FOLD = true: sum <= 3 R p, one conditional -2p", BASE,
     lambda g: (g.R * g.p + (g.R - 1) * g.p) // g.R < 2 * g.p and (3 * g.R * g.p + (g.R - 1) * g.p) // g.R < 4 * g.p and 4 * g.p <= g.R),
    ("fp.cuh:625", "(p^2 + 6p^2 + m p)/R < p (7p/R + 1) < 2p", EXT, lambda g: (7 * g.p * g.p + (g.R - 1) * g.p) // g.R < 2 * g.p),
    ("fp.cuh:774", "NEG_BETA * p must fit N limbs", EXT,
     lambda g: g.nb * g.p < g.R and (1 + g.nb) * (_top(g) + 1) < 1 << 32),
    ("fp.cuh:889", "2 NEG_BETA p must fit N limbs", EXT, lambda g: 2 * g.nb * g.p < g.R and (1 + 2 * g.nb) * (_top(g) + 1) < 1 << 32),
    ("fp.cuh:905", "(4 + 4 NEG_BETA) p^2", EXT, lambda g: 2 * g.p * 2 * g.p + 2 * g.nb * g.p * 2 * g.p == (4 + 4 * g.nb) * g.p * g.p),
    ("fp.cuh:906", "BLS12-377, 8 p^2 for beta = -1 over BLS12-381): (sum + m p) / R < 2p for both fields (p/R = 0.0066, 0.102)", EXT,
     lambda g: (4 + 4 * g.nb) == {"BLS12_377_FQ": 24, "BLS12_381_FQ": 8}[g.field] and (4 + 4 * g.nb) * g.p <= g.R
     and {"BLS12_377_FQ": _ratio(g, 4) == 0.0066, "BLS12_381_FQ": _ratio(g, 3) == 0.102}[g.field]),
    ("fp.cuh:908", "sop2_r without a final subtraction needs 8p <= R", EXT, lambda g: 8 * g.p <= g.R and _top(g) >> 29 == 0),
    ("fp.cuh:923", "bound (8 + 8 NEG_BETA) p^2: within R p over BLS12-377 (48 p < R); over BLS12-381 (16 p^2 > R p) one fold follows", EXT,
     lambda g: ((8 + 8 * g.nb) * g.p < g.R) == (g.field == "BLS12_377_FQ") and (8 + 8 * g.nb) * g.p <= 3 * g.R
     and (8 + 8 * g.nb) == {"BLS12_377_FQ": 48, "BLS12_381_FQ": 16}[g.field]),
    ("fp.cuh:925", "constexpr bool FOLD = ((u64)(8 + 8 * NEG_BETA) * ((u64)P::P[N - 1] + 1)) > (1ull << 32)", EXT,
     lambda g: ((8 + 8 * g.nb) * (_top(g) + 1) > 1 << 32) == ((8 + 8 * g.nb) * g.p > g.R)),
    ("fp.cuh:926", "<= 3 * (1ull << 32)", EXT, lambda g: (8 + 8 * g.nb) * (_top(g) + 1) <= 3 << 32),
    ("fp.cuh:944", "2p * (2 + 2 NEG_BETA) p must stay below R p", EXT,
     lambda g: (4 + 4 * g.nb) * g.p < g.R and (4 + 4 * g.nb) * (_top(g) + 1) < 1 << 32),
    ("fp.cuh:949", "(<= (2 + 2 NEG_BETA) p < 2^(32N))", EXT, lambda g: (2 + 2 * g.nb) * g.p < g.R),
]
