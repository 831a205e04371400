"""Exact model of the carry-free limb arithmetic (csrc/fp28.cuh FpL, fp28x2.cuh Fp2L, fft.cuh Fft29) in plain Python integers.

Every operation is restated from its DEFINITION, not from the header's loops:

  products   T = the exact sum of the integer products, m = -T p^-1 mod 2^(W L); the result is the integer (T + m p) / 2^(W L)
             written with limbs 0..L-2 below 2^W and the rest in the top limb.  Unique, so the device must match limb for limb.
  differences  the integer a - b (- 2 c) + K p; the swept forms have unique limbs, the semi-normalised ones are limb-wise
             a_i - b_i + spread_i with spread = K p re-written so that every limb lends H 2^W to the one below it.

and carries its PRECONDITION: an operation raises OutOfContract when its input is outside what the code is written for --
a column of a product reaching 2^64 (computed exactly), a limb of a limb-wise difference negative or reaching 2^32, a value
outside the documented range.  A test vector that raises fails the test; generators build in-class inputs by construction.

Built on tests/pyref.py (MODULI, Curve).  Limb vectors are Python lists of ints; numpy only carries them to the device."""
import os
import re
from fractions import Fraction

import numpy as np

import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algebra_amd", "csrc")
U32 = 1 << 32
U64 = 1 << 64


class OutOfContract(AssertionError):
    pass


def need(cond, msg):
    if not cond:
        raise OutOfContract(msg)


# ---- op codes and template parameters: THE TABLE of csrc/lazytest_api.hpp, parsed -----------------------------------------
def parse_api():
    txt = open(os.path.join(CSRC, "lazytest_api.hpp")).read()
    enum = {}
    for body in re.findall(r"enum \w+ : int \{(.*?)\};", txt, re.S):
        body = re.sub(r"//[^\n]*", "", body)
        for name, val in re.findall(r"(\w+)\s*=\s*(\d+)", body):
            enum[name] = int(val)
    rows = {}
    table = re.search(r"constexpr Row TABLE\[\] = \{(.*?)\n\};", txt, re.S).group(1)
    for m in re.finditer(r"\{(\w+), \"(\w+)\", (\d+), (\d+), \{([^}]*)\}, \{([^}]*)\}\}", table):
        op, name, arity, nk, ks, hs = m.groups()
        ks = [int(v) for v in ks.split(",") if v.strip()]
        hs = [int(v) for v in hs.split(",") if v.strip()]
        hs += [0] * (len(ks) - len(hs))
        assert len(ks) == int(nk), name
        rows[name] = dict(op=enum[op], arity=int(arity), params=list(zip(ks, hs)) if ks else [(0, 0)], templated=bool(ks))
    return enum, rows


ENUM, TABLE = parse_api()
FIELD_ID = {n: i for i, n in enumerate(P.FIELD_ORDER)}
FR_FIELDS = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
FQ_FIELDS = ["BN254_FQ", "BLS12_381_FQ", "BLS12_377_FQ"]
NEG_BETA = {"BLS12_381_FQ": 1, "BLS12_377_FQ": 5}   # Fp2 = Fp[u] / (u^2 + NB)


def parse_params_lz():
    """LZ_* of csrc/params.hpp per field"""
    txt = open(os.path.join(CSRC, "params.hpp")).read()
    out = {}
    for m in re.finditer(r"struct (\w+) \{(.*?)\n\};", txt, re.S):
        body = m.group(2)
        d = {k: int(re.search(r"int %s = (\d+);" % k, body).group(1)) for k in ("N", "LZ_W", "LZ_L", "LZ_RP")}
        d["LZ_INV"] = int(re.search(r"LZ_INV = (0x[0-9a-f]+)u;", body).group(1), 16)
        cin = re.search(r"LZ_CIN\[\d+\] = \{(.*?)\};", body).group(1)
        d["LZ_CIN"] = sum(int(t.strip().rstrip("u"), 16) << (32 * i) for i, t in enumerate(cin.split(",")))
        kp = re.search(r"LZ_KP\[\d+\]\[\d+\] = \{(.*?)\};", body).group(1)
        d["LZ_KP"] = [[int(t.strip().rstrip("u"), 16) for t in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", kp)]
        out[m.group(1)] = d
    return out


class Geo:
    """Limb geometry of one field, derived from p alone: 384-bit fields 14 x 28 bits, 256-bit fields 9 x 29 bits."""

    def __init__(self, name):
        self.name = name
        self.p = p = P.MODULI[name][0]
        self.N = 2 * P.nlimbs(p)                 # 32-bit words of the canonical form
        self.W = 28 if self.N == 12 else 29
        self.L = -(-32 * self.N // self.W)       # fewest W-bit limbs that hold every N x 32-bit value
        self.WL = self.W * self.L
        self.SH = self.WL - 32 * self.N
        self.MASK = (1 << self.W) - 1
        self.R = 1 << self.WL
        self.INV = (-pow(p, -1, 1 << self.W)) % (1 << self.W)
        self.RP = self.R // p
        self.CIN = self.R % p
        self.SEMI2 = 10 * self.L < (1 << (64 - 2 * self.W))
        self.PINV = pow(p, -1, self.R)
        self.NB = NEG_BETA.get(name)

    # ---- limbs <-> integers ----
    def limbs(self, v):
        """the unique form with limbs 0..L-2 below 2^W and the rest in the top limb"""
        need(v >= 0, "negative value")
        out = [(v >> (self.W * i)) & self.MASK for i in range(self.L - 1)]
        top = v >> (self.W * (self.L - 1))
        need(top < U32, "top limb does not fit 32 bits")
        return out + [top]

    def val(self, l):
        return sum(int(x) << (self.W * i) for i, x in enumerate(l))

    def normalised(self, l):
        return all(0 <= x <= self.MASK for x in l)

    def kp(self, k):
        return self.limbs(k * self.p)

    def spread(self, k, h):
        """k p with every limb lending h 2^W to the one below it (kp_spread / kp_spread_any): the same integer"""
        base = self.kp(k)
        return [base[i] + ((h << self.W) if i < self.L - 1 else 0) - (h if i > 0 else 0) for i in range(self.L)]

    def one(self):
        return self.limbs(self.CIN)

    # ---- products ----
    def _columns_ok(self, pairs, T, m):
        """every 64-bit column accumulator of the product-scanning form, computed exactly, stays below 2^64"""
        L, W = self.L, self.W
        # cheap sufficient condition first: L terms per pair at the limb maxima + L reduction terms + the carry
        worst = sum(L * max(a) * max(b) for a, b in pairs) + L * self.MASK * self.MASK
        if worst + (worst >> W) + 1 < U64:
            return True
        pl = self.kp(1)
        ml = [(m >> (W * i)) & self.MASK for i in range(L)]
        carry = 0
        for k in range(2 * L - 1):
            lo, hi = max(0, k - L + 1), min(k, L - 1)
            t = carry
            for a, b in pairs:
                for i in range(lo, hi + 1):
                    t += a[i] * b[k - i]
            for i in range(lo, hi + 1):
                t += ml[i] * pl[k - i]
            if t >= U64:
                return False
            carry = t >> W
        return True

    def sop(self, pairs):
        """sum of products under ONE reduction: (T + m p) / 2^(W L) with m = -T p^-1 mod 2^(W L)"""
        for a, b in pairs:
            need(len(a) == self.L and len(b) == self.L, "limb count")
            need(all(0 <= x < U32 for x in a) and all(0 <= x < U32 for x in b), "limb outside 32 bits")
        T = sum(self.val(a) * self.val(b) for a, b in pairs)
        m = (-T * self.PINV) % self.R
        need(self._columns_ok(pairs, T, m), "a column of the product reaches 2^64")
        q, rem = divmod(T + m * self.p, self.R)
        assert rem == 0
        return self.limbs(q)

    def mul(self, a, b):
        return self.sop([(a, b)])

    def sqr(self, a):
        need(all(2 * x < U32 for x in a), "doubled limb does not fit 32 bits")   # the cross products use a_i << 1
        return self.sop([(a, a)])

    def sop2(self, a, b, c, d):
        return self.sop([(a, b), (c, d)])

    def sop4(self, a, b, c, d, e, f, g, h):
        return self.sop([(a, b), (c, d), (e, f), (g, h)])

    # ---- sums and differences ----
    def add_lazy(self, a, b):
        r = [x + y for x, y in zip(a, b)]
        need(all(x < U32 for x in r), "limb-wise sum reaches 2^32")
        return r

    def _signed_sweep(self, terms, value):
        """FpL::normalise: signed limbs, |d_i + carry| inside 31 bits, value in [0, 2^(W L))"""
        need(0 <= value < self.R, "value outside [0, 2^(W L))")
        carry = 0
        for i, d in enumerate(terms):
            v = d + carry
            need(-(1 << 31) <= v < (1 << 31), "signed limb leaves 32 bits")
            carry = v >> self.W
        return self.limbs(value)

    def sub(self, k, a, b):
        need(all(x < (3 << 29) for x in a + b), "sub: limbs below 3 2^29")
        kp = self.kp(k)
        return self._signed_sweep([x - y + z for x, y, z in zip(a, b, kp)], self.val(a) - self.val(b) + k * self.p)

    def negsub(self, k, a, b):
        need(all(x < (1 << 30) for x in a + b), "negsub: limbs below 2^30")
        kp = self.kp(k)
        return self._signed_sweep([z - x - y for x, y, z in zip(a, b, kp)], k * self.p - self.val(a) - self.val(b))

    def neg(self, k, a):
        need(all(x < (1 << 30) for x in a), "neg: limbs below 2^30")
        kp = self.kp(k)
        return self._signed_sweep([z - x for x, z in zip(a, kp)], k * self.p - self.val(a))

    def _limbwise(self, terms, what):
        need(all(0 <= t < U32 for t in terms), what + ": a limb is negative or reaches 2^32")
        return list(terms)

    def _unsigned_sweep(self, terms, what):
        """carry sweep over unsigned 32-bit limbs that may neither go negative nor wrap"""
        carry, value = 0, 0
        for i, t in enumerate(terms):
            v = t + carry
            need(0 <= v < U32, what + ": a swept limb is negative or reaches 2^32")
            value += t << (self.W * i)
            carry = v >> self.W if i < self.L - 1 else 0
        return self.limbs(value)

    def sub_semi(self, k, a, b):
        sp = self.spread(k, 1)
        return self._limbwise([x - y + s for x, y, s in zip(a, b, sp)], "sub_semi")

    def sub_sweep(self, k, a, b):
        sp = self.spread(k, 1)
        return self._unsigned_sweep([x - y + s for x, y, s in zip(a, b, sp)], "sub_sweep")

    def sub_op(self, k, a, b):
        return self.sub_semi(k, a, b) if self.SEMI2 else self.sub_sweep(k, a, b)

    def sub_b_2c_norm(self, k, a, b, c):
        sp = self.spread(k, 3)
        return self._unsigned_sweep([x - y - 2 * z + s for x, y, z, s in zip(a, b, c, sp)], "sub_b_2c_norm")

    def neg_semi(self, k, a):
        sp = self.spread(k, 1)
        return self._limbwise([s - x for x, s in zip(a, sp)], "neg_semi")

    def cond_neg_semi(self, k, a, neg):
        return self.neg_semi(k, a) if neg else self._limbwise(a, "cond_neg_semi")

    def beta_neg(self, k, a):
        """NB (k p - a), limb-wise from the spread NB k p (Fp2L::beta_neg)"""
        nb = self.NB
        sp = self.spread(nb * k, nb)
        return self._limbwise([s - nb * x for x, s in zip(a, sp)], "beta_neg")

    # ---- divisions by powers of two, exact tests, the boundary with 32-bit words ----
    def shr_mod(self, k, a):
        need(1 <= k <= 24, "shr_mod: single-limb step")
        need(all(0 <= x <= self.MASK for x in a[:-1]) and 0 <= a[-1] < U32, "shr_mod: normalised limbs")
        v = self.val(a)
        need(v < self.R, "shr_mod: value below 2^(W L)")
        m = (-v * pow(self.p, -1, 1 << k)) % (1 << k)
        q, rem = divmod(v + m * self.p, 1 << k)
        assert rem == 0
        return self.limbs(q)

    def to_canonical_bits(self, a):
        need(self.normalised(a), "to_canonical_bits: normalised limbs")
        v = self.val(a)
        need(v < 2 * self.p and v < (1 << (32 * self.N)), "to_canonical_bits: value below 2 p")
        return self.words(v % self.p)

    def is_zero_or_p(self, a):
        need(self.normalised(a), "is_zero_or_p: normalised limbs")
        v = self.val(a)
        need(v < 2 * self.p, "is_zero_or_p: value below 2 p")
        return int(v % self.p == 0)

    def is_zero_mod_p(self, a):
        need(self.normalised(a), "is_zero_mod_p: normalised limbs")
        v = self.val(a)
        need(v < 9 * self.p, "is_zero_mod_p: value below 9 p")
        return int(v % self.p == 0)

    def words(self, v):
        need(0 <= v < (1 << (32 * self.N)), "value does not fit N words")
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(self.N)]

    def from_words(self, w):
        return sum(int(x) << (32 * i) for i, x in enumerate(w[:self.N]))

    def unpack32(self, w):
        return self.limbs(self.from_words(w))

    def unpack32_shl(self, w):
        return self.limbs(self.from_words(w) << self.SH)

    def pack32(self, a):
        need(self.normalised(a), "pack32: normalised limbs")
        return self.words(self.val(a))

    # ---- Fft29 (9 x 29 bits) ----
    def fft_dif(self, k, h, a, b):
        sp = self.spread(k, h)
        return self._limbwise([x - y + s for x, y, s in zip(a, b, sp)], "dif")

    def fft_q(self, a):
        ptop = self.kp(1)[8]
        return (a[8] * (U32 // (ptop + 1))) >> 32

    def fft_reduce_sweep(self, a):
        """V - q p with q the multiply-high estimate of floor(V / p) from the top limb; all nine limbs normalised"""
        need(self.W == 29 and self.L == 9, "Fft29 geometry")
        v = self.val(a)
        need(v < self.R, "reduce_sweep: value below 2^261")
        q = self.fft_q(a)
        comp = self.limbs(self.R - self.p)
        carry = 0
        for i in range(9):
            need(a[i] + carry < U32, "reduce_sweep: limb + carry reaches 2^32")
            carry = (q * comp[i] + a[i] + carry) >> 29
        r = v - q * self.p
        need(0 <= r < self.R, "reduce_sweep: estimate exceeds the quotient")
        out = self.limbs(r)
        need(self.normalised(out), "reduce_sweep: output normalised")
        return out

    def fft_sweep(self, a):
        carry = 0
        for i in range(8):
            need(a[i] + carry < U32, "sweep: limb + carry reaches 2^32")
            carry = (a[i] + carry) >> 29
        need(a[8] + carry < U32, "sweep: top limb reaches 2^32")
        return self.limbs(self.val(a))

    def fft_cond_sub_p(self, a):
        need(self.normalised(a), "cond_sub_p: normalised limbs")
        v = self.val(a)
        return self.limbs(v - self.p if v >= self.p else v)

    def fft_canon(self, a):
        r = self.val(self.fft_reduce_sweep(a))
        need(r < 3 * self.p, "canon: reduce_sweep leaves 3 p or more")
        return self.limbs(self.val(a) % self.p)

    # ---- Fp2L: an element is the pair (c0 limbs, c1 limbs); results per lane through the product rule above ----
    def x2_mul(self, ka, A, B):
        bz = self.beta_neg(ka, A[1])
        return (self.sop2(A[0], B[0], bz, B[1]), self.sop2(A[0], B[1], A[1], B[0]))

    def x2_sqr(self, kw, A):
        """(value, zero flag): complex squaring, one product per lane"""
        nb = self.NB
        bz = self.beta_neg(kw, A[1])
        s = self.mul(self.add_lazy(A[0], A[1]), self.add_lazy(A[0], bz))
        need(all(2 * x < U32 for x in A[0]), "x2_sqr: 2 a0 fits 32 bits")
        c1 = self.mul([2 * x for x in A[0]], A[1])
        zero = int(self.is_zero_or_p(s) and self.is_zero_or_p(c1))
        if nb == 1:
            return (s, c1), zero
        return (self._limbwise([x + ((nb - 1) // 2) * y for x, y in zip(s, c1)], "x2_sqr"), c1), zero

    def x2_mul_sub(self, ka, ky, A, B, Y, D):
        nb = self.NB
        bz = self.beta_neg(ka, A[1])
        ny0, ny1 = self.neg_semi(ky, Y[0]), self.neg_semi(ky, Y[1])
        nby1 = self._limbwise([nb * x for x in Y[1]], "x2_mul_sub")
        return (self.sop4(A[0], B[0], bz, B[1], ny0, D[0], nby1, D[1]),
                self.sop4(A[0], B[1], A[1], B[0], ny0, D[1], ny1, D[0]))

    def x2_reduce_small(self, A):
        return (self.mul(A[0], self.one()), self.mul(A[1], self.one()))

    def x2_to_canonical(self, A):
        return tuple(self.to_canonical_bits(self.shr_mod(self.SH, c)) for c in A)

    # the Fp2 element a pair of lanes stands for, as residues (radix 2^(W L) removed)
    def residue(self, a):
        return self.val(a) * pow(self.R, -1, self.p) % self.p


GEO = {name: Geo(name) for name in P.FIELD_ORDER}


# ---- operand classes and their generators --------------------------------------------------------------------------------
class Cls:
    """An operand class: every limb below `limb_max` (exclusive; the top limb below `top_max`), the value below `vmax`."""

    def __init__(self, g, limb_max, vmax=None, name=""):
        self.g, self.M, self.name = g, limb_max, name
        full = sum((limb_max - 1) << (g.W * i) for i in range(g.L))
        self.vmax = full + 1 if vmax is None else min(int(vmax), full + 1)
        self.capped = vmax is not None

    def contains(self, l):
        return len(l) == self.g.L and all(0 <= x < self.M for x in l) and self.g.val(l) < self.vmax

    def reshape(self, l, mask):
        """the same value in another limb shape: limb i borrows 2^W from limb i+1 where bit i of mask is set and the class allows"""
        g = self.g
        l = list(l)
        for i in range(g.L - 1):
            if (mask >> i) & 1 and l[i + 1] >= 1 and l[i] + (1 << g.W) < self.M:
                l[i] += 1 << g.W
                l[i + 1] -= 1
        return l

    def from_value(self, v):
        v = min(max(v, 0), self.vmax - 1)
        return self.g.limbs(v)

    def extremes(self):
        g, M = self.g, self.M
        L, W = g.L, g.W
        out = []
        if not self.capped:   # limb extremes: the class is its limb bound
            out.append([M - 1] * L)
            for i in range(L):
                out.append([M - 1 if j == i else 0 for j in range(L)])
            out.append([M - 1 if j % 2 == 0 else 0 for j in range(L)])
            out.append([M - 1 if j % 2 == 1 else 0 for j in range(L)])
        else:                 # the largest limbs the value bound admits, greedily from the top / from each position
            for start in range(L):
                l, v = [0] * L, 0
                for i in list(range(start, -1, -1)) + list(range(L - 1, start, -1)):
                    room = (self.vmax - 1 - v) >> (W * i)
                    l[i] = min(M - 1, room)
                    v += l[i] << (W * i)
                out.append(l)
            for ph in (0, 1):
                l, v = [0] * L, 0
                for i in range(L - 1, -1, -1):
                    if i % 2 == ph:
                        l[i] = min(M - 1, (self.vmax - 1 - v) >> (W * i))
                        v += l[i] << (W * i)
                out.append(l)
        out.append([0] * L)
        # value extremes
        vals = {0, 1, g.p - 1, g.p, g.p + 1, self.vmax - 1}
        j = 2
        while j * g.p - 1 < self.vmax and j <= 300:
            vals.update((j * g.p - 1, j * g.p, j * g.p + 1))
            j = j + 1 if j < 16 else j * 2
        for i in range(L):
            vals.update(((1 << (W * i)), (1 << (W * i)) - 1))
        for v in sorted(vals):
            if 0 <= v < self.vmax:
                n = g.limbs(v)
                if all(x < M for x in n):
                    out.append(n)
                    if M > (1 << W) + 1:   # the same value in other limb shapes
                        for mask in ((1 << L) - 1, 0x5555, 0x2AAA):
                            r = self.reshape(n, mask)
                            if r != n:
                                out.append(r)
        for l in out:
            assert self.contains(l), (self.name, l)
        return out

    def random(self, rng, n):
        g = self.g
        out = []
        for _ in range(n):
            if not self.capped:
                l = [int(x) for x in rng.integers(0, self.M, size=g.L)]
            else:
                v = int.from_bytes(rng.bytes(64), "little") % self.vmax
                l = g.limbs(v)
                if self.M > (1 << g.W) + 1:
                    l = self.reshape(l, int(rng.integers(0, 1 << g.L)))
            out.append(l)
        return out


def classes(g):
    """the operand classes the comments of fp28.cuh / fp28x2.cuh / fft.cuh name"""
    W = g.W
    c = {
        "n": Cls(g, 1 << W, None, "n"),                         # normalised
        "s": Cls(g, 3 << W, None, "s"),                         # semi-normalised (sub_semi output)
        "l2": Cls(g, 2 << W, None, "l2"),                       # add_lazy of two normalised / neg_semi output
        "l30": Cls(g, 1 << 30, None, "l30"),                    # what sub / neg / negsub accept
        "n31": Cls(g, 1 << 31, None, "n31"),                    # beside a normalised operand of a product
    }
    for k in (1, 2, 3, 4, 6, 7, 8, 9, 10):   # normalised, value below (k - 1/2) p: a legal subtrahend of a K = k difference
        c["n<%d" % k] = Cls(g, 1 << W, (2 * k - 1) * g.p // 2, "n<%d" % k)
    c["n<2p"] = Cls(g, 1 << W, 2 * g.p, "n<2p")
    c["n<9p"] = Cls(g, 1 << W, 9 * g.p, "n<9p")
    c["n<p"] = Cls(g, 1 << W, g.p, "n<p")
    c["n<1.16"] = Cls(g, 1 << W, 116 * g.p // 100, "n<1.16")   # PPP, Q of a bucket addition (documented < 1.06)
    c["w32"] = Cls(g, 1 << W, 1 << (32 * g.N), "w32")           # what pack32 accepts
    if g.NB:
        c["bn"] = Cls(g, (g.NB + 1) << W, None, "bn")           # beta_neg output
        c["nby"] = Cls(g, max(g.NB << W, 2), None, "nby")       # NB y (mul_sub)
    if W == 29:
        c["f30"] = Cls(g, 1 << 30, None, "f30")                 # s = x + x'
        c["f31"] = Cls(g, 1 << 31, None, "f31")                 # y0 = s0 + s1
        c["f2.5"] = Cls(g, 5 << 29, None, "f2.5")               # the tail differences: limbs below 2.5 2^30
        c["f30<6"] = Cls(g, 1 << 30, 13 * g.p // 2, "f30<6")    # s1 as the subtrahend of dif<7, 2> (value below 6.02 p)
        c["f31<13"] = Cls(g, 1 << 31, 1302 * g.p // 100, "f31<13")   # what reduce_sweep / canon meet (value below 13.02 p)
    return c


# ---- vectors: (inputs, expected) of one (field, op, k, h) -------------------------------------------------------------------
def _zip_cases(lists, rng, nrand, cls_list):
    """extreme lists paired position-wise (cycled to the longest) + the all-maximum row first + random rows"""
    n = max(len(x) for x in lists)
    rows = [[x[i % len(x)] for x in lists] for i in range(n)]
    # every operand at its first extreme simultaneously comes first by construction (index 0); add shifted pairings
    for shift in (1, 3):
        rows += [[x[(i + shift * j) % len(x)] for j, x in enumerate(lists)] for i in range(n)]
    rnd = [c.random(rng, nrand) for c in cls_list]
    rows += [[r[i] for r in rnd] for i in range(nrand)]
    return rows


def op_classes(g, name, k, h):
    """the legal operand-class combinations of an op, as the comments list them: a list of tuples of class names"""
    s2 = g.SEMI2
    if name == "mul":
        out = [("n", "n"), ("n", "s"), ("s", "n"), ("n", "n31"), ("n31", "n"), ("n", "l2")]
        if s2:
            out.append(("s", "s"))
        if g.W == 29:
            out.append(("f2.5", "n<p"))    # the FFT's tail difference times a canonical twiddle
        return out
    if name == "sqr":
        return [("n",), ("s",)] if s2 else [("n",)]   # 9 x 29 bits: sub_op sweeps P and R before they are squared
    if name == "sop2":
        # Y3 of the mixed addition: R t + (2p - Y1) PPP
        out = [("n", "n", "n", "n"), ("s", "s", "l2", "n") if s2 else ("n", "s", "l2", "n")]
        if g.NB:   # Fp2L::mul: even lane a0 b0 + (beta a1) b1, odd lane a0 b1 + a1 b0; A0 / B0 up to semi-normalised
            out += [("s", "s", "bn", "n"), ("s", "n", "n", "s")]
        return out
    if name == "sop4":   # Fp2L::mul_sub, 14 x 28 bits only
        return [("n", "n", "bn", "n", "l2", "n", "nby", "n")] if g.NB else []
    if name == "add_lazy":
        return [("n", "n"), ("l2", "n")]
    if name in ("sub_semi",):
        return [("n", "n<%d" % k)]
    if name == "sub_sweep":
        return [("s", "n<%d" % k), ("n", "n<%d" % k)]
    if name == "sub_op":
        return [("n", "n<%d" % k)]
    if name == "sub_b_2c_norm":
        out = [("n", "n<1.16", "n<1.16")]
        if g.NB:   # Fp2L: the c0 of R^2 is semi-normalised
            out.append(("s", "n<1.16", "n<1.16"))
        return out
    if name == "neg_semi":
        return [("n<%d" % k,)]
    if name == "neg":
        return [("n<%d" % k,)]
    if name == "shr_mod":
        return [("n",)]
    if name in ("to_canonical_bits", "is_zero_or_p"):
        return [("n<2p",)]
    if name == "is_zero_mod_p":
        return [("n<9p",)]
    if name == "pack32":
        return [("w32",)]
    if name == "dif":
        return {(4, 1): [("n", "n<4")], (7, 2): [("f30", "f30<6")], (2, 1): [("n", "n<2")]}[(k, h)]
    if name in ("reduce_sweep", "canon"):
        return [("f31<13",)]
    if name == "sweep":
        return [("f31",)]
    if name == "cond_sub_p":
        return [("n",)]
    raise KeyError(name)


def apply_model(g, name, k, h, ops):
    """-> (limbs (L, zero-padded), flag)"""
    L = g.L
    pad = lambda w: list(w) + [0] * (L - len(w))
    if name in ("mul", "sop2", "sop4", "add_lazy"):
        return getattr(g, name)(*ops), 0
    if name == "sqr":
        return g.sqr(ops[0]), 0
    if name in ("sub", "sub_semi", "sub_sweep", "sub_op", "sub_b_2c_norm", "negsub", "neg", "neg_semi"):
        return getattr(g, name)(k, *ops), 0
    if name == "cond_neg_semi":
        return g.cond_neg_semi(k, ops[0], ops[1][0] != 0), 0
    if name == "shr_mod":
        return g.shr_mod(k, ops[0]), 0
    if name == "to_canonical_bits":
        return pad(g.to_canonical_bits(ops[0])), 0
    if name == "pack32":
        return pad(g.pack32(ops[0])), 0
    if name == "unpack32":
        return g.unpack32(ops[0]), 0
    if name == "unpack32_shl":
        return g.unpack32_shl(ops[0]), 0
    if name == "is_zero_or_p":
        return [0] * L, g.is_zero_or_p(ops[0])
    if name == "is_zero_mod_p":
        return [0] * L, g.is_zero_mod_p(ops[0])
    if name == "dif":
        return g.fft_dif(k, h, *ops), 0
    if name in ("reduce_sweep", "sweep", "canon", "cond_sub_p"):
        return getattr(g, "fft_" + name)(ops[0]), 0
    raise KeyError(name)


def near_miss_zero(g, kmax):
    """exact-zero tests: k p for every k, and values that pass the one-limb filter (low limb of some k p) but differ from
    every multiple of p in one bit of another limb"""
    out = []
    for k in range(kmax + 1):
        kp = g.kp(k)
        out.append(kp)
        for i in range(1, g.L):
            for bit in (0, g.W - 1) if i < g.L - 1 else (0,):
                l = list(kp)
                l[i] ^= 1 << bit
                out.append(l)
    return out


def field_vectors(field, name, k, h, nrand=4096, seed=1):
    """Rows of operand limb vectors for one op: the deterministic extreme list of every legal class combination, then
    `nrand` random in-class rows spread over the combinations.  -> list of rows (each: `arity` limb vectors)"""
    g = GEO[field]
    rng = np.random.default_rng([seed, FIELD_ID[field], TABLE[name]["op"], k, h])
    cl = classes(g)
    L = g.L
    rows = []
    if name in ("unpack32", "unpack32_shl"):
        top = (1 << (32 * g.N)) - 1
        vals = [0, 1, g.p - 1, g.p, g.p + 1, top, top - 1, 2 * g.p if 2 * g.p <= top else g.p] + [1 << i for i in range(0, 32 * g.N, 7)]
        vals += [(1 << i) - 1 for i in range(1, 32 * g.N, 5)]
        vals += [int.from_bytes(rng.bytes(4 * g.N), "little") for _ in range(nrand)]
        return [[g.words(v) + [0] * (L - g.N)] for v in vals]
    if name == "sub":            # a - b + 0 p: b below a limb by limb, limbs below 2^30
        c = Cls(g, 3 << 29, g.R, "l3")   # limbs below 3 2^29 (3 xx of the doubling); FpL::normalise: the value stays below 2^(W L)
        a_list = c.extremes() + c.random(rng, nrand)
        for a in a_list:
            rows.append([a, [0] * L])
            rows.append([a, [int(rng.integers(0, x + 1)) for x in a]])
        return rows
    if name == "negsub":         # k p - a - b >= 0
        half = Cls(g, 1 << g.W, k * g.p // 2, "half")
        return _zip_cases([half.extremes(), half.extremes()[::-1]], rng, nrand, [half, half])
    if name == "cond_neg_semi":
        c = cl["n<%d" % k]
        rows = []
        for i, a in enumerate(c.extremes() + c.random(rng, nrand)):
            rows.append([a, [i & 1] + [0] * (L - 1)])
            rows.append([a, [1 - (i & 1)] + [0] * (L - 1)])
        return rows
    combos = op_classes(g, name, k, h)
    per = -(-nrand // max(len(combos), 1))
    for combo in combos:
        cs = [cl[c] for c in combo]
        rows += _zip_cases([c.extremes() for c in cs], rng, per, cs)
    if name == "is_zero_or_p":
        rows += [[l] for l in near_miss_zero(g, 1) if cl["n<2p"].contains(l)]
    if name == "is_zero_mod_p":
        rows += [[l] for l in near_miss_zero(g, 8) if cl["n<9p"].contains(l)]
    if name in ("reduce_sweep", "canon", "sweep"):   # sums of up to four tile elements (normalised, below 3.01 p)
        t = Cls(g, 1 << g.W, 301 * g.p // 100, "tile")
        ex = t.extremes()
        for i in range(len(ex)):
            acc = [0] * L
            for j in range(4):
                acc = g.add_lazy(acc, ex[(i + 5 * j) % len(ex)])
            rows.append([acc])
    return rows


def expected(field, name, k, h, rows):
    g = GEO[field]
    return [apply_model(g, name, k, h, r) for r in rows]


def rows_to_array(g, rows):
    return np.array(rows, dtype=np.uint64).astype(np.uint32).reshape(len(rows), -1)


def expected_to_array(g, exp):
    return np.array([list(l) + [f] for l, f in exp], dtype=np.uint64).astype(np.uint32)


def all_field_ops(field):
    """every (name, k, h) of THE TABLE that this field's unit serves (FpL everywhere, Fft29 on the scalar fields)"""
    g = GEO[field]
    out = []
    for name, row in TABLE.items():
        if name.startswith("x2_"):
            continue
        if row["op"] >= ENUM["FFT_FIRST"] and field not in FR_FIELDS:
            continue
        if name == "sop4" and not g.NB:
            continue
        for k, h in row["params"]:
            if name == "shr_mod" and k != g.SH:
                continue
            out.append((name, k, h))
    return out


# ---- Fp2L: vectors in LANE layout (lane 2 e: c0 of element e, lane 2 e + 1: its c1) ---------------------------------------
X2_LANEWISE = {"x2_reduce_small": None, "x2_to_canonical": None, "x2_from_canonical": "unpack32_shl", "x2_beta_neg": None,
               "x2_sub_sweep": "sub_sweep", "x2_sub_b_2c_norm": "sub_b_2c_norm"}


def x2_vectors(field, name, k, h, nrand=4096, seed=2):
    """-> (lane rows, expected per lane as (limbs, flag)); an even number of lanes"""
    g = GEO[field]
    assert g.NB
    rng = np.random.default_rng([seed, FIELD_ID[field], TABLE[name]["op"], k, h])
    cl = classes(g)
    L = g.L
    pad = lambda w: list(w) + [0] * (L - len(w))
    if name in X2_LANEWISE:     # the lanes are independent: the FpL vectors of the same function, two to a pair
        if X2_LANEWISE[name]:
            rows = field_vectors(field, X2_LANEWISE[name], k, h, nrand, seed)
            exp = [apply_model(g, X2_LANEWISE[name], k, h, r) for r in rows]
        elif name == "x2_beta_neg":
            c = cl["n<%d" % k]
            rows = [[a] for a in c.extremes() + c.random(rng, nrand)]
            exp = [(g.beta_neg(k, r[0]), 0) for r in rows]
        elif name == "x2_reduce_small":
            rows = [[a] for a in cl["n"].extremes() + cl["n"].random(rng, nrand)]
            exp = [(g.mul(r[0], g.one()), 0) for r in rows]
        else:                   # to_canonical: a normalised value below 256 p
            c = Cls(g, 1 << g.W, 256 * g.p, "n<256p")
            rows = [[a] for a in c.extremes() + c.random(rng, nrand)]
            exp = [(pad(g.to_canonical_bits(g.shr_mod(g.SH, r[0]))), 0) for r in rows]
        if len(rows) & 1:
            rows.append(rows[0])
            exp.append(exp[0])
        return rows, exp
    if name == "x2_both":
        rows = [[[b] + [0] * (L - 1)] for pair in ((0, 0), (0, 1), (1, 0), (1, 1), (7, 0), (1 << 31, 3)) for b in pair]
        exp = []
        for i in range(0, len(rows), 2):
            both = int(rows[i][0][0] != 0 and rows[i + 1][0][0] != 0)
            exp += [([0] * L, both), ([0] * L, both)]
        return rows, exp
    # the pair ops: elements as (c0 class, c1 class) per operand
    if name == "x2_mul":
        shapes = [[("s", "n<%d" % k), ("s", "n")], [("n", "n<%d" % k), ("n", "n")], [("s", "n<%d" % k), ("n", "n")]]
    elif name == "x2_sqr":
        shapes = [[("n<%d" % k, "n<%d" % k)]]
    elif name == "x2_mul_sub":
        shapes = [[("n", "n<%d" % k), ("n", "n"), ("n<%d" % h, "n<%d" % h), ("n", "n")]]
    else:
        raise KeyError(name)
    elems = []
    per = -(-nrand // len(shapes))
    for shape in shapes:
        flat = [cl[c] for pair in shape for c in pair]
        for row in _zip_cases([c.extremes() for c in flat], rng, per, flat):
            elems.append([(row[2 * j], row[2 * j + 1]) for j in range(len(shape))])
    if name == "x2_sqr":        # the zero flag: every (i p, j p) the class admits, and near misses on either component
        zs = [l for l in near_miss_zero(g, 8) if cl["n<%d" % k].contains(l)]
        mult = [g.kp(j) for j in range(9) if cl["n<%d" % k].contains(g.kp(j))]
        for a in mult:
            for b in mult:
                elems.append([(a, b)])
        for i, z in enumerate(zs):
            elems.append([(z, mult[i % len(mult)])])
            elems.append([(mult[i % len(mult)], z)])
    rows, exp = [], []
    for e in elems:
        if name == "x2_mul":
            r, flag = g.x2_mul(k, *e), 0
        elif name == "x2_sqr":
            r, flag = g.x2_sqr(k, e[0])
        else:
            r, flag = g.x2_mul_sub(k, h, *e), 0
        rows.append([op[0] for op in e])
        rows.append([op[1] for op in e])
        exp += [(r[0], flag), (r[1], flag)]
    return rows, exp


def all_x2_ops():
    return [(name, k, h) for name, row in TABLE.items() if name.startswith("x2_") for k, h in row["params"]]


# ---- the bucket additions on carry-free limbs (ec28.cuh, ec28x2.cuh) composed from the ops above ---------------------------
# An accumulator is a dict x / y / zz / zzz (G1: limb lists; G2: pairs of limb lists) + inf.  Every step goes through the
# model ops, so every intermediate is checked against its precondition, and the result is exact limb for limb.
CURVE_FIELD = {"BN254_G1": "BN254_FQ", "BLS12_381_G1": "BLS12_381_FQ", "BLS12_377_G1": "BLS12_377_FQ",
               "BLS12_377_G2": "BLS12_377_FQ", "BLS12_381_G2": "BLS12_381_FQ"}
# the accumulator invariant, units of p (normalised limbs): ec28.cuh XYZZL (14 x 28 bits) and its header (9 x 29 bits: BN254),
# ec28x2.cuh XYZZL2.  zz / zzz: what from_bucket and the first full addition leave (one product with the residue 1).
ACC_INVARIANT = {
    "BLS12_381_G1": dict(x="5.01", y="1.13", zz="1.13", zzz="1.13", src="ec28.cuh XYZZL"),
    "BLS12_377_G1": dict(x="5.01", y="1.13", zz="1.13", zzz="1.13", src="ec28.cuh XYZZL"),
    "BN254_G1": dict(x="5.07", y="1.21", zz="1.21", zzz="1.21", src="ec28.cuh header (9 x 29 bits)"),
    "BLS12_377_G2": dict(x="7.2", y="1.11", zz="1.11", zzz="1.11", src="ec28x2.cuh XYZZL2"),
    "BLS12_381_G2": dict(x="7.2", y="1.11", zz="1.11", zzz="1.11", src="ec28x2.cuh XYZZL2"),
}


class AccModel:
    def __init__(self, curve):
        self.curve = curve
        self.cid = P.CURVE_ORDER.index(curve)
        self.C = P.Curve(curve)
        self.g = g = GEO[CURVE_FIELD[curve]]
        self.ext = 2 if curve.endswith("G2") else 1
        self.words = (4 * self.ext) * g.L + 1     # LazyK::WORDS
        self.R32 = (1 << (32 * g.N)) % g.p
        self.zero_l = [0] * g.L
        self.bound = {c: Fraction(v) for c, v in ACC_INVARIANT[curve].items() if c != "src"}

    # -- coordinates: G1 limbs, G2 (c0, c1) --
    def comps(self, c):
        return [c] if self.ext == 1 else list(c)

    def mk(self, comps):
        return comps[0] if self.ext == 1 else tuple(comps)

    def one(self):
        return self.mk([self.g.one()] + [self.zero_l] * (self.ext - 1))

    def zero(self):
        return self.mk([self.zero_l] * self.ext)

    def residue(self, c):
        """the field element a coordinate stands for (radix 2^(W L) removed)"""
        r = [self.g.residue(x) for x in self.comps(c)]
        return r[0] if self.ext == 1 else tuple(r)

    def lift(self, e, js=None, shape=0):
        """field element -> coordinate limbs of value (e R' mod p) + j p per component, in limb shape `shape`"""
        g = self.g
        es = [e] if self.ext == 1 else list(e)
        js = js or [0] * self.ext
        out = []
        for x, j in zip(es, js):
            out.append(g.limbs(x * g.R % g.p + j * g.p))
        return self.mk(out)

    # -- canonical words (the memory form: Montgomery residues with radix 2^(32 N)) --
    def canon_words(self, e):
        g = self.g
        es = [e] if self.ext == 1 else list(e)
        return [w for x in es for w in g.words(x * self.R32 % g.p)]

    def from_canon_words(self, w):
        g = self.g
        inv = pow(self.R32, -1, g.p)
        r = [g.from_words(w[i * g.N:(i + 1) * g.N]) * inv % g.p for i in range(self.ext)]
        return r[0] if self.ext == 1 else tuple(r)

    def operand(self, w):
        """canonical words -> multiplication operand (unpack32_shl / Fp2L::from_canonical): the residue itself, below 2^SH p"""
        g = self.g
        return self.mk([g.unpack32_shl(w[i * g.N:(i + 1) * g.N]) for i in range(self.ext)])

    def neg_words(self, w):
        g = self.g
        out = []
        for i in range(self.ext):
            v = g.from_words(w[i * g.N:(i + 1) * g.N])
            need(v < g.p, "canonical input")
            out += g.words((g.p - v) % g.p)
        return out

    # -- field ops on coordinates --
    def reduce_small(self, a):
        g = self.g
        return self.mk([g.mul(x, g.one()) for x in self.comps(a)])

    def mul(self, ka, a, b):
        return self.g.mul(a, b) if self.ext == 1 else self.g.x2_mul(ka, a, b)

    def lanewise(self, fn, *args):
        return self.mk([fn(*[self.comps(a)[i] for a in args]) for i in range(self.ext)])

    def is_zero_sq(self, kw, a):
        """(a^2, a = 0 mod p): asked of the square, as the kernels do"""
        g = self.g
        if self.ext == 1:
            s = g.sqr(a)
            return s, bool(g.is_zero_or_p(s))
        s, z = g.x2_sqr(kw, a)
        return s, bool(z)

    # -- doubling of an affine point given as small coordinates --
    def _mdbl_small(self, x1, y1):
        g = self.g
        Z = self.zero()
        if self.ext == 1:
            u = g.sub(0, g.add_lazy(y1, y1), Z)
            v = g.sqr(u)
            w = g.mul(u, v)
            s = g.mul(x1, v)
            xx = g.sqr(x1)
            m = g.sub(0, g.add_lazy(g.add_lazy(xx, xx), xx), Z)
            x3 = g.sub_b_2c_norm(4, g.sqr(m), Z, s)
            t = g.sub_semi(6, s, x3)
            y3 = g.sop2(m, t, g.neg_semi(2, w), y1)
            return dict(x=x3, y=y3, zz=v, zzz=w, inf=False)
        dbl = lambda c: g.sub(0, g.add_lazy(c, c), self.zero_l)
        u = self.lanewise(dbl, y1)
        v = g.x2_sqr(4, u)[0]
        w = g.x2_mul(4, u, v)
        s = g.x2_mul(2, x1, v)
        xx = self.reduce_small(g.x2_sqr(2, x1)[0])
        m = self.lanewise(lambda c: g.sub(0, g.add_lazy(g.add_lazy(c, c), c), self.zero_l), xx)
        x3 = self.lanewise(lambda a, b, c: g.sub_b_2c_norm(4, a, b, c), g.x2_sqr(4, m)[0], Z, s)
        t = self.lanewise(lambda a, b: g.sub_sweep(8, a, b), s, x3)
        y3 = g.x2_mul_sub(4, 2, m, t, y1, w)
        return dict(x=x3, y=y3, zz=self.reduce_small(v), zzz=w, inf=False)

    def mdbl(self, aff_words, neg):
        """acc = +-2 base (xyzz_mdbl_lazy / lazy2_mdbl)"""
        n = self.g.N * self.ext
        xw, yw = aff_words[:n], aff_words[n:]
        if neg:
            yw = self.neg_words(yw)
        x2, y2 = self.operand(xw), self.operand(yw)
        if self.ext == 1:   # xyzz_mdbl_lazy_xy brings them below 1.13 itself
            g = self.g
            return self._mdbl_small(g.mul(x2, g.one()), g.mul(y2, g.one()))
        return self._mdbl_small(self.reduce_small(x2), self.reduce_small(y2))

    def dbl(self, acc):
        if acc["inf"]:
            return dict(acc)
        g = self.g
        if self.ext == 1:
            d = self._mdbl_small(g.mul(acc["x"], g.one()), g.mul(acc["y"], g.one()))
            return dict(x=d["x"], y=d["y"], zz=g.mul(d["zz"], acc["zz"]), zzz=g.mul(d["zzz"], acc["zzz"]), inf=False)
        d = self._mdbl_small(self.reduce_small(acc["x"]), acc["y"])
        return dict(x=d["x"], y=d["y"], zz=g.x2_mul(2, d["zz"], acc["zz"]), zzz=g.x2_mul(2, d["zzz"], acc["zzz"]), inf=False)

    # -- mixed addition: acc +- affine base; "equal points" doubles the base --
    def madd(self, acc, aff_words, neg):
        g = self.g
        if not any(aff_words):
            return dict(acc)
        n = g.N * self.ext
        xw, yw = aff_words[:n], aff_words[n:]
        if neg:
            yw = self.neg_words(yw)
        x2, y2 = self.operand(xw), self.operand(yw)
        if acc["inf"]:
            return dict(x=self.reduce_small(x2), y=self.reduce_small(y2), zz=self.one(), zzz=self.one(), inf=False)
        if self.ext == 1:
            u2 = g.mul(x2, acc["zz"])
            s2 = g.mul(y2, acc["zzz"])
            pd = g.sub_op(6, u2, acc["x"])
            rd = g.sub_op(2, s2, acc["y"])
            pp, pz = self.is_zero_sq(0, pd)
            if pz:
                if self.is_zero_sq(0, rd)[1]:
                    return self.mdbl(aff_words, neg)
                return dict(acc, inf=True)
            ppp = g.mul(pd, pp)
            q = g.mul(acc["x"], pp)
            x3 = g.sub_b_2c_norm(4, g.sqr(rd), ppp, q)
            t = g.sub_semi(6, q, x3)
            y3 = g.sop2(rd, t, g.neg_semi(2, acc["y"]), ppp)
            return dict(x=x3, y=y3, zz=g.mul(acc["zz"], pp), zzz=g.mul(acc["zzz"], ppp), inf=False)
        sw = lambda k: (lambda a, b: g.sub_sweep(k, a, b))
        u2 = g.x2_mul(2, acc["zz"], x2)
        s2 = g.x2_mul(2, acc["zzz"], y2)
        pd = self.lanewise(sw(8), u2, acc["x"])
        rd = self.lanewise(sw(2), s2, acc["y"])
        pp, pz = g.x2_sqr(10, pd)
        if pz:
            if g.x2_sqr(4, rd)[1]:
                return self.mdbl(aff_words, neg)
            return dict(acc, inf=True)
        ppp = g.x2_mul(10, pd, pp)
        q = g.x2_mul(8, acc["x"], pp)
        rr = g.x2_sqr(4, rd)[0]
        x3 = self.lanewise(lambda a, b, c: g.sub_b_2c_norm(4, a, b, c), rr, ppp, q)
        t = self.lanewise(sw(8), q, x3)
        y3 = g.x2_mul_sub(4, 2, rd, t, acc["y"], ppp)
        return dict(x=x3, y=y3, zz=g.x2_mul(2, acc["zz"], pp), zzz=g.x2_mul(2, acc["zzz"], ppp), inf=False)

    # -- full addition: acc += b, b's coordinates multiplication operands (a repacked stored bucket, or an accumulator) --
    def add_operands(self, acc, b):
        g = self.g
        if b["inf"]:
            return dict(acc)
        if acc["inf"]:
            return dict(x=self.reduce_small(b["x"]), y=self.reduce_small(b["y"]), zz=self.reduce_small(b["zz"]),
                        zzz=self.reduce_small(b["zzz"]), inf=False)
        if self.ext == 1:
            u1 = g.mul(acc["x"], b["zz"])
            u2 = g.mul(b["x"], acc["zz"])
            s1 = g.mul(acc["y"], b["zzz"])
            s2 = g.mul(b["y"], acc["zzz"])
            pd = g.sub_op(3, u2, u1)
            rd = g.sub_op(2, s2, s1)
            pp, pz = self.is_zero_sq(0, pd)
            if pz:
                if self.is_zero_sq(0, rd)[1]:
                    return self.dbl(acc)
                return dict(acc, inf=True)
            ppp = g.mul(pd, pp)
            q = g.mul(u1, pp)
            x3 = g.sub_b_2c_norm(4, g.sqr(rd), ppp, q)
            t = g.sub_semi(6, q, x3)
            y3 = g.sop2(rd, t, g.neg_semi(2, s1), ppp)
            return dict(x=x3, y=y3, zz=g.mul(g.mul(acc["zz"], b["zz"]), pp), zzz=g.mul(g.mul(acc["zzz"], b["zzz"]), ppp),
                        inf=False)
        sw = lambda k: (lambda a, c: g.sub_sweep(k, a, c))
        u1 = g.x2_mul(8, acc["x"], b["zz"])
        u2 = g.x2_mul(2, acc["zz"], b["x"])
        s1 = g.x2_mul(2, acc["y"], b["zzz"])
        s2 = g.x2_mul(2, acc["zzz"], b["y"])
        pd = self.lanewise(sw(4), u2, u1)
        rd = self.lanewise(sw(2), s2, s1)
        pp, pz = g.x2_sqr(6, pd)
        if pz:
            if g.x2_sqr(4, rd)[1]:
                return self.dbl(acc)
            return dict(acc, inf=True)
        ppp = g.x2_mul(6, pd, pp)
        q = g.x2_mul(4, u1, pp)
        rr = g.x2_sqr(4, rd)[0]
        x3 = self.lanewise(lambda a, c, d: g.sub_b_2c_norm(4, a, c, d), rr, ppp, q)
        t = self.lanewise(sw(8), q, x3)
        y3 = g.x2_mul_sub(4, 2, rd, t, s1, ppp)
        return dict(x=x3, y=y3, zz=g.x2_mul(2, g.x2_mul(2, acc["zz"], b["zz"]), pp),
                    zzz=g.x2_mul(2, g.x2_mul(2, acc["zzz"], b["zzz"]), ppp), inf=False)

    def bucket_operands(self, xyzz_words):
        n = self.g.N * self.ext
        c = [self.operand(xyzz_words[i * n:(i + 1) * n]) for i in range(4)]
        return dict(x=c[0], y=c[1], zz=c[2], zzz=c[3], inf=not any(xyzz_words[2 * n:3 * n]))

    def add(self, acc, xyzz_words):
        return self.add_operands(acc, self.bucket_operands(xyzz_words))

    def add_acc(self, acc, other):
        return self.add_operands(acc, other)

    def from_bucket(self, xyzz_words):
        b = self.bucket_operands(xyzz_words)
        return dict(x=self.reduce_small(b["x"]), y=self.reduce_small(b["y"]), zz=self.reduce_small(b["zz"]),
                    zzz=self.reduce_small(b["zzz"]), inf=b["inf"])

    def to_bucket(self, acc):
        g = self.g
        n = g.N * self.ext
        if acc["inf"]:   # XYZZ::zero(): (1, 1, 0, 0) in canonical Montgomery words
            one = self.canon_words(1 if self.ext == 1 else (1, 0))
            return one + one + [0] * (2 * n)
        out = []
        for c in ("x", "y", "zz", "zzz"):
            for comp in self.comps(acc[c]):
                out += g.to_canonical_bits(g.shr_mod(g.SH, comp))
        return out

    # -- the parked layout (LazyK::park): coordinate k, component c at words [(ext k + c) L, ..), then the infinity flag --
    def park(self, acc):
        out = []
        for c in ("x", "y", "zz", "zzz"):
            for comp in self.comps(acc[c]):
                out += list(comp)
        return out + [1 if acc["inf"] else 0]

    def unpark(self, w):
        L = self.g.L
        w = [int(x) for x in w]
        cs = [self.mk([w[(self.ext * k + c) * L:(self.ext * k + c + 1) * L] for c in range(self.ext)]) for k in range(4)]
        return dict(x=cs[0], y=cs[1], zz=cs[2], zzz=cs[3], inf=w[4 * self.ext * L] != 0)

    # -- what an accumulator stands for --
    def affine(self, acc):
        """the affine point (pyref form) of an XYZZ accumulator: x = X / ZZ, y = Y / ZZZ"""
        if acc["inf"]:
            return None
        F = self.C.F
        X, Y, ZZ, ZZZ = (self.residue(acc[c]) for c in ("x", "y", "zz", "zzz"))
        return (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))

    def consistent(self, acc):
        """ZZ^3 = ZZZ^2"""
        if acc["inf"]:
            return True
        F = self.C.F
        ZZ, ZZZ = self.residue(acc["zz"]), self.residue(acc["zzz"])
        return F.mul(F.mul(ZZ, ZZ), ZZ) == F.mul(ZZZ, ZZZ)

    def in_invariant(self, acc):
        """every coordinate normalised and below the documented bound: a legal input again"""
        if acc["inf"]:
            return True
        g = self.g
        for c in ("x", "y", "zz", "zzz"):
            for comp in self.comps(acc[c]):
                if not g.normalised(comp) or not (g.val(comp) < self.bound[c] * g.p):
                    return False
        return True

    def make(self, pt, z, js, shape=None):
        """the accumulator (X, Y, ZZ, ZZZ) = (x z^2, y z^3, z^2, z^3) of the affine point pt, every component stored as
        (residue R' mod p) + j p with j from js (a list of 4 x ext multiples)"""
        F = self.C.F
        zz = F.mul(z, z)
        zzz = F.mul(zz, z)
        vals = [F.mul(pt[0], zz), F.mul(pt[1], zzz), zz, zzz]
        e = self.ext
        return dict(x=self.lift(vals[0], js[0:e]), y=self.lift(vals[1], js[e:2 * e]), zz=self.lift(vals[2], js[2 * e:3 * e]),
                    zzz=self.lift(vals[3], js[3 * e:4 * e]), inf=False)

    def infinity(self):
        return dict(x=self.zero(), y=self.zero(), zz=self.zero(), zzz=self.zero(), inf=True)

    def max_j(self, c):
        """the largest j with (p - 1) + j p below the coordinate's bound"""
        b = self.bound[c]
        j = int(b) + 1
        while not (self.g.p - 1 + j * self.g.p < b * self.g.p):
            j -= 1
        return j


ACC_KIND = {k[4:].lower(): v for k, v in ENUM.items() if k.startswith("ACC_") and k != "ACC_KINDS"}


def acc_apply(A, kind, acc, other):
    """one accumulator op of csrc/lazytest_api.hpp (AccKind) on the model; acc / other in the form the ABI takes them:
    a model accumulator, canonical words (affine base / XYZZ bucket) or None"""
    if kind in ("madd", "msub"):
        return A.madd(acc, other, kind == "msub")
    if kind in ("mdbl", "mdbl_neg"):
        return A.mdbl(other, kind == "mdbl_neg")
    if kind == "add":
        return A.add(acc, other)
    if kind == "add_acc":
        return A.add_acc(acc, other)
    if kind == "dbl":
        return A.dbl(acc)
    if kind == "from_bucket":
        return A.from_bucket(acc)
    raise KeyError(kind)


def acc_states(A, pt, zs, rng, few=False):
    """accumulators of the affine point pt at the edge of the invariant: X = (x zz R' mod p) + j p for EVERY j the bound admits,
    and y / zz / zzz lifted by p wherever their residue leaves room below the bound"""
    out = []
    e = A.ext
    for z in zs:
        base = A.make(pt, z, [0] * (4 * e))
        top = {}
        for ci, c in enumerate(("x", "y", "zz", "zzz")):
            top[c] = []
            for comp in A.comps(base[c]):
                j = 0
                while A.g.val(comp) + (j + 1) * A.g.p < A.bound[c] * A.g.p:
                    j += 1
                top[c].append(j)
        jx = range(max(top["x"]) + 1)
        for j in (jx if not few else (0, max(top["x"]))):
            js = []
            for c in ("x", "y", "zz", "zzz"):
                for t in top[c]:
                    js.append(min(j, t) if c == "x" else (t if j % 2 == 0 else 0))
            out.append(A.make(pt, z, js))
        if e == 2:   # the two components at different multiples
            js = [top["x"][0], 0] + [0, top["y"][1]] + [0] * 4
            out.append(A.make(pt, z, js))
    for a in out:
        assert A.in_invariant(a)
    return out


def small_residue_zs(A, rng, count, tries=400):
    """z values whose zz / zzz have a stored integer below (bound - 1) p, so that zz + p is still inside the invariant"""
    F, g = A.C.F, A.g
    out = []
    for _ in range(tries):
        z = F.from_int(tuple(int.from_bytes(rng.bytes(48), "little") for _ in range(2)) if A.ext == 2
                       else int.from_bytes(rng.bytes(48), "little"))
        zz = F.mul(z, z)
        zzz = F.mul(zz, z)
        for v, c in ((zz, "zz"), (zzz, "zzz")):
            comps = [v] if A.ext == 1 else list(v)
            if any((x * g.R % g.p) + g.p < A.bound[c] * g.p for x in comps):
                out.append(z)
                break
        if len(out) >= count:
            break
    return out


def acc_edge_cases(A, G, seed=3):
    """-> list of (kind, acc, other, expected affine point or None): the branches at the edge of the invariant"""
    C = A.C
    rng = np.random.default_rng([seed, A.cid])
    F = C.F
    rz = lambda: F.from_int(tuple(int.from_bytes(rng.bytes(48), "little") for _ in range(2)) if A.ext == 2
                            else int.from_bytes(rng.bytes(48), "little"))
    pts = {k: C.mul(G, k) for k in (1, 2, 3, 5, 7, 11)}
    zs = [F.from_int(1), rz()] + small_residue_zs(A, rng, 2)
    aff = lambda pt: [int(w) for w in _u32(C.enc(pt))]
    bucket = lambda pt, z: A.canon_words(F.mul(pt[0], F.mul(z, z))) + A.canon_words(F.mul(pt[1], F.mul(F.mul(z, z), z))) + \
        A.canon_words(F.mul(z, z)) + A.canon_words(F.mul(F.mul(z, z), z))
    n = A.g.N * A.ext
    inf_bucket = A.to_bucket(A.infinity())
    cases = []
    for ka in (3, 7):
        pa = pts[ka]
        for acc in acc_states(A, pa, zs, rng):
            # mixed addition: another point, the same point (double the base), the inverse (to infinity), nothing
            for kb, sign in ((5, +1), (5, -1), (ka, +1), (ka, -1)):
                for kind in ("madd", "msub"):
                    eff = sign if kind == "madd" else -sign
                    want = C.add(pa, pts[kb] if eff > 0 else C.neg(pts[kb]))
                    base = pts[kb] if sign > 0 else C.neg(pts[kb])
                    cases.append((kind, acc, aff(base), want))
            cases.append(("madd", acc, [0] * (2 * n), pa))
            cases.append(("dbl", acc, None, C.add(pa, pa)))
            # full addition with a stored bucket and with another accumulator
            for kb, sign in ((2, +1), (ka, +1), (ka, -1)):
                pb = pts[kb] if sign > 0 else C.neg(pts[kb])
                cases.append(("add", acc, bucket(pb, zs[1]), C.add(pa, pb)))
                for other in acc_states(A, pb, zs[1:3], rng, few=True)[:3]:
                    cases.append(("add_acc", acc, other, C.add(pa, pb)))
            cases.append(("add", acc, inf_bucket, pa))
            cases.append(("add_acc", acc, A.infinity(), pa))
    # out of infinity and back into it
    inf = A.infinity()
    for k in (1, 11):
        cases.append(("madd", inf, aff(pts[k]), pts[k]))
        cases.append(("msub", inf, aff(pts[k]), C.neg(pts[k])))
        cases.append(("mdbl", inf, aff(pts[k]), C.add(pts[k], pts[k])))
        cases.append(("mdbl_neg", inf, aff(pts[k]), C.neg(C.add(pts[k], pts[k]))))
        cases.append(("add", inf, bucket(pts[k], zs[1]), pts[k]))
        for other in acc_states(A, pts[k], zs[:2], rng, few=True):
            cases.append(("add_acc", inf, other, pts[k]))
        cases.append(("from_bucket", bucket(pts[k], zs[1]), None, pts[k]))
    cases.append(("madd", inf, [0] * (2 * n), None))
    cases.append(("add", inf, inf_bucket, None))
    cases.append(("add_acc", inf, inf, None))
    cases.append(("dbl", inf, None, None))
    cases.append(("from_bucket", inf_bucket, None, None))
    return cases


def _u32(a):
    """numpy u64 limbs -> u32 words (little endian)"""
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.uint32).reshape(-1)


def bucket_point(A, words):
    """the affine point of a canonical XYZZ bucket (x | y | zz | zzz words)"""
    n = A.g.N * A.ext
    x, y, zz, zzz = (A.from_canon_words(words[i * n:(i + 1) * n]) for i in range(4))
    F = A.C.F
    if zz == F.zero():
        return None
    return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))


def acc_pack(A, kind, accs, others):
    """-> (acc array, other array or None, output words per bucket) as ark_hip_test_lazy_acc_op takes them"""
    nw = 4 * A.g.N * A.ext
    a = np.array([x if kind == "from_bucket" else A.park(x) for x in accs], dtype=np.uint64).astype(np.uint32)
    if kind == "add_acc":
        o = np.array([A.park(x) for x in others], dtype=np.uint64).astype(np.uint32)
    elif kind in ("dbl", "from_bucket", "to_bucket"):
        o = None
    else:
        o = np.array(others, dtype=np.uint64).astype(np.uint32)
    return a, o, (nw if kind == "to_bucket" else A.words)


def acc_chain_ops(A, G, lanes, steps, seed=4):
    """the operand schedule of `lanes` chains of `steps` random mixed ops from edge states: -> (start states with their
    scalar multiples, [(kind, [operand per lane], [operand multiple per lane])]).  Operands are small multiples of G, often
    the accumulated point itself or its inverse, so the doubling and infinity branches recur."""
    C = A.C
    F = C.F
    rng = np.random.default_rng([seed, A.cid])
    rz = lambda: F.from_int(tuple(int.from_bytes(rng.bytes(48), "little") for _ in range(2)) if A.ext == 2
                            else int.from_bytes(rng.bytes(48), "little"))
    cache = {}

    def pt(m):
        if m not in cache:
            cache[m] = C.mul(G, m % C.r) if m % C.r else None
        return cache[m]

    starts, mult = [], []
    for i in range(lanes):
        m = 2 + i
        st = acc_states(A, pt(m), [rz()], rng)
        starts.append(st[-1 - (i % 2)] if i else A.infinity())
        mult.append(m if i else 0)
    sched = []
    cur = list(mult)
    for s in range(steps):
        kind = ["madd", "msub", "add", "add_acc", "dbl", "madd", "add_acc"][int(rng.integers(0, 7))]
        ops, ms = [], []
        for i in range(lanes):
            r = int(rng.integers(0, 6))
            m = cur[i] if r == 0 else -cur[i] if r == 1 else int(rng.integers(1, 9)) * (1 if r < 4 else -1)
            if kind in ("madd", "msub"):
                if m % C.r == 0:
                    m = 1
                ops.append([int(w) for w in _u32(C.enc(pt(m)))])
            elif kind == "add":
                if m % C.r == 0:
                    ops.append(A.to_bucket(A.infinity()))
                else:
                    z = rz()
                    zz = F.mul(z, z)
                    zzz = F.mul(zz, z)
                    ops.append(A.canon_words(F.mul(pt(m)[0], zz)) + A.canon_words(F.mul(pt(m)[1], zzz)) + A.canon_words(zz)
                               + A.canon_words(zzz))
            elif kind == "add_acc":
                ops.append(A.infinity() if m % C.r == 0 else acc_states(A, pt(m), [rz()], rng, few=True)[int(rng.integers(0, 2))])
            else:
                ops.append(None)
                m = cur[i]
            ms.append(m)
            cur[i] = cur[i] - m if kind == "msub" else cur[i] + m
        sched.append((kind, ops, ms))
    return starts, mult, sched, pt


# ---- THE TABLE OF DOCUMENTED BOUNDS ------------------------------------------------------------------------------------------
# Operand classes and output bounds exactly as the comments of the kernels state them, units of p, each citing file and line.
# documented_bounds(curve) re-derives every figure from the accumulator invariant with exact rational arithmetic -- a product
# of operands below A p and B p is below (A B p / R' + 1) p, a difference a - b + K p lies in (a_lo - b_hi + K, a_hi - b_lo + K)
# -- and returns (where, what, documented (lo, hi), derived (lo, hi)); a documented figure must CONTAIN the derived one.
def _F(x):
    return Fraction(str(x))


DOC_G1_28 = {   # ec28.cuh, 14 x 28 bits (BLS12-381 / BLS12-377 Fq); input x2, y2 < 256
    "first": (0, "1.13", "ec28.cuh:120"), "u2": (0, "1.13", "ec28.cuh:127"), "s2": (0, "1.13", "ec28.cuh:128"),
    "pd": ("0.99", "7.13", "ec28.cuh:129"), "rd": ("0.87", "3.13", "ec28.cuh:130"), "pp": (0, "1.03", "ec28.cuh:131"),
    "ppp": (0, "1.01", "ec28.cuh:137"), "q": (0, "1.01", "ec28.cuh:138"), "x3": ("0.97", "5.01", "ec28.cuh:139"),
    "t": ("0.99", "7.01", "ec28.cuh:140"), "y3": (0, "1.02", "ec28.cuh:141"), "zz3": (0, "1.01", "ec28.cuh:144"),
    "zzz3": (0, "1.01", "ec28.cuh:145"),
    "d.x1": (0, "1.13", "ec28.cuh:86"), "d.u": (0, "2.3", "ec28.cuh:88"), "d.v": (0, "1.01", "ec28.cuh:89"),
    "d.w": (0, "1.01", "ec28.cuh:90"), "d.s": (0, "1.01", "ec28.cuh:91"), "d.xx": (0, "1.01", "ec28.cuh:92"),
    "d.m": (0, "3.03", "ec28.cuh:93"), "d.x3": ("1.9", "5.01", "ec28.cuh:94"), "d.t": ("0.9", "7.02", "ec28.cuh:95"),
    "d.y3": (0, "1.02", "ec28.cuh:96"),
    "a.u1": (0, "1.63", "ec28.cuh:154"), "a.u2": (0, "1.13", "ec28.cuh:154"), "a.s1": (0, "1.15", "ec28.cuh:154"),
    "a.s2": (0, "1.13", "ec28.cuh:154"), "a.pd": ("1.37", "4.13", "ec28.cuh:155"), "a.rd": ("0.85", "3.13", "ec28.cuh:155"),
    "a.pp": (0, "1.01", "ec28.cuh:155"), "a.x3": ("0.99", "5.01", "ec28.cuh:156"), "a.y3": (0, "1.02", "ec28.cuh:156"),
    "bucket": (0, "2", "ec28.cuh:70"),
}
DOC_G1_29 = {   # ec28.cuh header, 9 x 29 bits (BN254 Fq); input x2, y2 < 32
    "first": (0, "1.21", "ec28.cuh:22"), "u2": (0, "1.23", "ec28.cuh:22"), "s2": (0, "1.23", "ec28.cuh:22"),
    "pd": ("0.9", "7.23", "ec28.cuh:23"), "rd": ("0.78", "3.23", "ec28.cuh:23"), "pp": (0, "1.31", "ec28.cuh:25"),
    "ppp": (0, "1.06", "ec28.cuh:25"), "q": (0, "1.04", "ec28.cuh:26"), "x3": ("0.8", "5.07", "ec28.cuh:26"),
    "t": (0, "7.04", "ec28.cuh:26"), "y3": (0, "1.15", "ec28.cuh:27"), "zz3": (0, "1.01", "ec28.cuh:27"),
    "zzz3": (0, "1.01", "ec28.cuh:27"),
    "a.u1": (0, "1.97", "ec28.cuh:29"), "a.s1": (0, "1.23", "ec28.cuh:29"), "a.pd": ("1.03", "4.23", "ec28.cuh:30"),
    "a.pp": (0, "1.11", "ec28.cuh:30"), "bucket": (0, "2", "ec28.cuh:30"),
}
DOC_G2 = {      # ec28x2.cuh (worst case over BLS12-381: NB = 1, and BLS12-377: NB = 5)
    "first": (0, "1.11", "ec28x2.cuh:36"), "u2": (0, "1.32", "ec28x2.cuh:108"), "s2": (0, "1.32", "ec28x2.cuh:109"),
    "pd": ("0.8", "9.32", "ec28x2.cuh:110"), "rd": ("0.89", "3.32", "ec28x2.cuh:111"), "pp.s": (0, "1.15", "ec28x2.cuh:113"),
    "pp.c1": (0, "1.07", "ec28x2.cuh:113"), "pp.c0": (0, "3.1", "ec28x2.cuh:113"), "ppp": (0, "1.02", "ec28x2.cuh:121"),
    "q": (0, "1.02", "ec28x2.cuh:122"), "rr.c0": (0, "3.1", "ec28x2.cuh:123"), "rr.c1": (0, "1.01", "ec28x2.cuh:123"),
    "x3": ("0.9", "7.1", "ec28x2.cuh:124"), "t": ("0.9", "9.02", "ec28x2.cuh:125"), "y3": (0, "1.04", "ec28x2.cuh:126"),
    "zz3": (0, "1.01", "ec28x2.cuh:127"), "zzz3": (0, "1.01", "ec28x2.cuh:128"),
    "a.u1": (0, "2.55", "ec28x2.cuh:135"), "a.s1": (0, "1.32", "ec28x2.cuh:135"), "a.pd": ("1.45", "5.32", "ec28x2.cuh:136"),
    "a.rd": ("0.68", "3.32", "ec28x2.cuh:136"), "bucket": (0, "2", "ec28x2.cuh:46"),
}
DOC_FFT = {     # fft.cuh, the Fft29 table (2^261 / p >= 64)
    "tile": (0, "3.01", "fft.cuh:416"), "s": (0, "6.02", "fft.cuh:417"), "d": (0, "1.11", "fft.cuh:419"),
    "y0": (0, "12.04", "fft.cuh:420"), "y1": (0, "1.21", "fft.cuh:422"), "y2": (0, "2.22", "fft.cuh:423"),
    "y3": (0, "1.05", "fft.cuh:424"),
}


def documented_bounds(curve):
    """-> [(where, name, (doc lo, doc hi), (derived lo, derived hi))] for one curve, all in units of p"""
    A = AccModel(curve)
    g = A.g
    rp = Fraction(g.R, g.p)
    inv = A.bound
    IN = Fraction(1 << g.SH)                       # a repacked canonical coordinate: below 2^SH p
    prod = lambda *pairs: sum(a * b for a, b in pairs) / rp + 1
    out = {}
    if A.ext == 1:
        doc = DOC_G1_28 if g.W == 28 else DOC_G1_29
        K_ADD = 3
        out["first"] = (0, prod((IN, 1)))
        u2 = out["u2"] = (0, prod((IN, inv["zz"])))
        s2 = out["s2"] = (0, prod((IN, inv["zzz"])))
        pd = out["pd"] = (6 - inv["x"], u2[1] + 6)
        rd = out["rd"] = (2 - inv["y"], s2[1] + 2)
        pp = out["pp"] = (0, prod((pd[1], pd[1])))
        ppp = out["ppp"] = (0, prod((pd[1], pp[1])))
        q = out["q"] = (0, prod((inv["x"], pp[1])))
        x3 = out["x3"] = (4 - ppp[1] - 2 * q[1], prod((rd[1], rd[1])) + 4)
        t = out["t"] = (6 - x3[1], q[1] + 6 - x3[0])
        out["y3"] = (0, prod((rd[1], t[1]), (2, ppp[1])))
        out["zz3"] = (0, prod((inv["zz"], pp[1])))
        out["zzz3"] = (0, prod((inv["zzz"], ppp[1])))
        # the doubling of a base (x2, y2 below 2^SH p)
        x1 = out["d.x1"] = (0, prod((IN, 1)))
        u = out["d.u"] = (0, 2 * x1[1])
        v = out["d.v"] = (0, prod((u[1], u[1])))
        w = out["d.w"] = (0, prod((u[1], v[1])))
        s = out["d.s"] = (0, prod((x1[1], v[1])))
        xx = out["d.xx"] = (0, prod((x1[1], x1[1])))
        m = out["d.m"] = (0, 3 * xx[1])
        dx = out["d.x3"] = (4 - 2 * s[1], prod((m[1], m[1])) + 4)
        dt = out["d.t"] = (6 - dx[1], s[1] + 6 - dx[0])
        out["d.y3"] = (0, prod((m[1], dt[1]), (2, x1[1])))
        # the full addition with a stored bucket (coordinates below 2^SH p)
        u1 = out["a.u1"] = (0, prod((inv["x"], IN)))
        au2 = out["a.u2"] = (0, prod((IN, inv["zz"])))
        s1 = out["a.s1"] = (0, prod((inv["y"], IN)))
        as2 = out["a.s2"] = (0, prod((IN, inv["zzz"])))
        apd = out["a.pd"] = (K_ADD - u1[1], au2[1] + K_ADD)
        ard = out["a.rd"] = (2 - s1[1], as2[1] + 2)
        app = out["a.pp"] = (0, prod((apd[1], apd[1])))
        appp = (0, prod((apd[1], app[1])))
        aq = (0, prod((u1[1], app[1])))
        ax3 = out["a.x3"] = (4 - appp[1] - 2 * aq[1], prod((ard[1], ard[1])) + 4)
        at = (6 - ax3[1], aq[1] + 6 - ax3[0])
        out["a.y3"] = (0, prod((ard[1], at[1]), (2, appp[1])))
        out["bucket"] = (0, max(inv.values()) / IN + 1)
        closure = {"x": max(out["x3"][1], out["d.x3"][1], out["a.x3"][1], out["first"][1]),
                   "y": max(out["y3"][1], out["d.y3"][1], out["a.y3"][1], out["first"][1]),
                   "zz": max(out["zz3"][1], out["d.v"][1], out["first"][1]),
                   "zzz": max(out["zzz3"][1], out["d.w"][1], out["first"][1])}
    else:
        doc = DOC_G2
        nb = g.NB
        mul = lambda ka, a, b: (prod((a[0], b[0]), (nb * ka, b[1])), prod((a[0], b[1]), (a[1], b[0])))
        sq = lambda kw, a: (prod((a[0] + a[1], a[0] + nb * kw)), prod((2 * a[0], a[1])))
        two = lambda v: (v, v)
        out["first"] = (0, prod((IN, 1)))
        u2 = mul(2, two(inv["zz"]), two(IN))
        out["u2"] = (0, max(u2))
        s2 = mul(2, two(inv["zzz"]), two(IN))
        out["s2"] = (0, max(s2))
        pd = out["pd"] = (8 - inv["x"], max(u2) + 8)
        rd = out["rd"] = (2 - inv["y"], max(s2) + 2)
        s, c1 = sq(10, two(pd[1]))
        out["pp.s"], out["pp.c1"] = (0, s), (0, c1)
        c0 = s + Fraction(nb - 1, 2) * c1
        out["pp.c0"] = (0, c0)
        ppp = out["ppp"] = (0, max(mul(10, two(pd[1]), (c0, c1))))
        q = out["q"] = (0, max(mul(8, two(inv["x"]), (c0, c1))))
        rs, rc1 = sq(4, two(rd[1]))
        rc0 = rs + Fraction(nb - 1, 2) * rc1
        out["rr.c0"], out["rr.c1"] = (0, rc0), (0, rc1)
        x3 = out["x3"] = (4 - ppp[1] - 2 * q[1], max(rc0, rc1) + 4)
        t = out["t"] = (8 - x3[1], q[1] + 8 - x3[0])
        ev = prod((rd[1], t[1]), (nb * 4, t[1]), (2, ppp[1]), (nb * inv["y"], ppp[1]))
        od = prod((rd[1], t[1]), (rd[1], t[1]), (2, ppp[1]), (2, ppp[1]))
        out["y3"] = (0, max(ev, od))
        out["zz3"] = (0, max(mul(2, two(inv["zz"]), (c0, c1))))
        out["zzz3"] = (0, max(mul(2, two(inv["zzz"]), two(ppp[1]))))
        u1 = out["a.u1"] = (0, max(mul(8, two(inv["x"]), two(IN))))
        s1 = out["a.s1"] = (0, max(mul(2, two(inv["y"]), two(IN))))
        out["a.pd"] = (4 - u1[1], max(u2) + 4)
        out["a.rd"] = (2 - s1[1], max(s2) + 2)
        out["bucket"] = (0, max(inv.values()) / IN + 1)
        closure = {"x": max(x3[1], out["first"][1]), "y": max(out["y3"][1], out["first"][1]),
                   "zz": max(out["zz3"][1], out["first"][1]), "zzz": max(out["zzz3"][1], out["first"][1])}
    rows = []
    for name, (lo, hi, where) in doc.items():
        rows.append((where, name, (_F(lo), _F(hi)), out[name]))
    for c, v in closure.items():   # closure of the invariant itself
        rows.append((ACC_INVARIANT[curve]["src"], "invariant." + c, (0, inv[c]), (0, v)))
    return rows


def documented_fft_bounds(field):
    g = GEO[field]
    rp = Fraction(g.R, g.p)
    tile = _F("3.01")
    out = {"s": 2 * tile, "d": (tile + 4) / rp + 1}
    out["y0"] = 2 * out["s"]
    out["y1"] = (out["s"] + 7) / rp + 1
    out["y2"] = 2 * out["d"]
    out["y3"] = (out["d"] + 2) / rp + 1
    out["tile"] = max(out["d"], out["y1"], out["y2"], out["y3"], 3)   # reduce_sweep leaves less than 3 p (checked on the model)
    return [(w, n, (0, _F(hi)), (0, out[n])) for n, (lo, hi, w) in DOC_FFT.items()]
