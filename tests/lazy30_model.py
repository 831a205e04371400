"""Big-integer model of the signed 13 x 30-bit arithmetic of the plain accumulate kernel (csrc/fp30s.cuh, ec30s.cuh), in the
manner of tests/lazy_model.py for the 28-bit forms.

Three things live here:
  * the operations digit for digit (`mul`, `sqr`, `sop2`, `sub`, `add_2b`, `from_canonical_shl`, `to_canonical`, `madd`): a
    product is the integer (T + m p) / 2^390 with m the BALANCED 13-digit representative of -T / p mod 2^390 -- unique digit for
    digit, whatever the column schedule -- so the header's host twins and the device's asm chains must give exactly these;
  * the WORST CASE of every column (`column_bounds`): the sum of the magnitudes of all its terms, built from the digit limits of
    the operand classes and the real digits of p (not sampled), with the carry bound propagated column to column.  It must stay
    below 2^63 for every product of the mixed addition (`MADD_PRODUCTS`);
  * the value bounds of the mixed addition (`madd_value_chain`): exact rationals in units of p, from the accumulator invariant
    through one addition and back into the invariant.
"""
import os
import re
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algebra_amd", "csrc")

W, L, N32 = 30, 13, 12
HALF = 1 << (W - 1)
RBITS = W * L                   # 390
SH = RBITS - 32 * N32           # 6
P_INT = 4002409555221667393417789825735904156556882819939007885332058136124031650490837864442687629129015664037894272559787


def consts():
    """S30_BLS12_381_FQ of csrc/curve_consts.hpp"""
    txt = open(os.path.join(CSRC, "curve_consts.hpp")).read()
    body = re.search(r"struct S30_BLS12_381_FQ \{(.*?)\n\};", txt, re.S).group(1)
    arr = lambda name: [int(t) for t in re.search(r"%s\[\d+\] = \{(.*?)\};" % name, body).group(1).split(",")]
    return dict(W=int(re.search(r"W = (\d+)", body).group(1)), L=int(re.search(r"L = (\d+)", body).group(1)), P=arr("P"), ONE=arr("ONE"),
                OUT_KP=arr("OUT_KP"), OUT_K=int(re.search(r"OUT_K = (\d+)", body).group(1)),
                INV=int(re.search(r"INV = (0x[0-9a-f]+)u", body).group(1), 16))


def val(d):
    return sum(int(x) << (W * i) for i, x in enumerate(d))


def balanced(x, n=L, top_free=True):
    """digits 0..n-2 in [-2^29, 2^29); the top digit takes what is left (top_free) or is balanced too (x taken mod 2^(W n))"""
    out = []
    for i in range(n):
        if i == n - 1 and top_free:
            out.append(x)
            break
        d = x & ((1 << W) - 1)
        if d >= HALF:
            d -= 1 << W
        out.append(d)
        x = (x - d) >> W
    return out


PD = balanced(P_INT)            # the signed digits of p
PINV = pow(P_INT, -1, 1 << RBITS)


class Overflow(Exception):
    pass


def montgomery(T):
    """(T + m p) / 2^390 with m = -T / p mod 2^390 in 13 balanced digits"""
    m = val(balanced((-T * PINV) % (1 << RBITS), top_free=False))
    q, rem = divmod(T + m * P_INT, 1 << RBITS)
    assert rem == 0 and abs(m) <= HALF * ((1 << RBITS) - 1) // ((1 << W) - 1)
    return balanced(q)


def columns(a, b, x=None, y=None, square=False):
    """The product column by column as fp30s.cuh schedules it, every partial sum of every column checked against the signed 64-bit
    accumulator (Overflow).  Returns the digits; they equal montgomery(...) whenever nothing overflows."""
    lim = 1 << 63
    m, r, t = [0] * L, [0] * L, 0

    def acc(t, v):
        t += v
        if not -lim <= t < lim:
            raise Overflow(t)
        return t
    for k in range(2 * L - 1):
        lo, hi = (0, k) if k < L else (k - L + 1, L - 1)
        if square:
            for i in range(lo, hi + 1):
                if 2 * i < k:
                    t = acc(t, a[i] * (2 * a[k - i]))
            if k % 2 == 0:
                t = acc(t, a[k // 2] * a[k // 2])
        else:
            for i in range(lo, hi + 1):
                t = acc(t, a[i] * b[k - i])
                if x is not None:
                    t = acc(t, x[i] * y[k - i])
        for i in range(lo, (k - 1 if k < L else L - 1) + 1):
            t = acc(t, m[i] * PD[k - i])
        if k < L:
            m[k] = balanced(((t % (1 << 32)) * consts()["INV"]) % (1 << W), 1, top_free=False)[0]
            t = acc(t, m[k] * PD[0])
            assert t % (1 << W) == 0
        else:
            r[k - L] = balanced(t % (1 << W), 1, top_free=False)[0]
            t = acc(t, HALF)
        t >>= W
    r[L - 1] = t
    assert -(1 << 31) <= t < (1 << 31)
    return r


def mul(a, b):
    return montgomery(val(a) * val(b))


def sqr(a):
    return montgomery(val(a) ** 2)


def sop2(a, b, c, d):
    return montgomery(val(a) * val(b) + val(c) * val(d))


def sweep(d, wide=False):
    """FpS::sweep: |d_i| <= 2^30 (wide: 3 2^29); every partial sum inside 32 bits"""
    lim = 3 * HALF if wide else 2 * HALF
    assert all(abs(v) <= lim for v in d[:-1]), "sweep operand outside its class"
    out = balanced(val(d))
    assert -(1 << 31) <= out[-1] < (1 << 31)
    return out


def sub(a, b):
    return sweep([u - v for u, v in zip(a, b)])


def add_2b(a, b):
    return sweep([u + 2 * v for u, v in zip(a, b)], wide=True)


def neg(a):
    return [-v for v in a]


def from_words(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def to_words(x):
    return [(x >> (32 * i)) & 0xffffffff for i in range(N32)]


def from_canonical_shl(w):
    return balanced(from_words(w) << SH)


def to_canonical(a):
    """signed residue v R' (|v| < OUT_K p) -> canonical words of v R in [0, p)"""
    c = consts()
    wv = val(a) + c["OUT_K"] * P_INT
    assert 0 < wv < 2 * c["OUT_K"] * P_INT, "to_canonical operand outside (-OUT_K p, OUT_K p)"
    m = (wv * c["INV"]) % (1 << SH)
    q, rem = divmod(wv + m * P_INT, 1 << SH)
    assert rem == 0 and q < 2 * P_INT
    return to_words(q - P_INT if q >= P_INT else q)


def madd(acc, x2w, y2w):
    """xyzz_madd_s on (x, y, zz, zzz, inf) and a base in canonical words -> (accumulator, equal-points flag)"""
    x, y, zz, zzz, inf = acc
    x2, y2 = from_canonical_shl(x2w), from_canonical_shl(y2w)
    one = consts()["ONE"]
    if inf:
        return (mul(x2, one), mul(y2, one), list(one), list(one), 0), 0
    u2, s2 = mul(x2, zz), mul(y2, zzz)
    pd, rd = sub(u2, x), sub(s2, y)
    pp = sqr(pd)
    if not any(pp):
        if not any(sqr(rd)):
            return (x, y, zz, zzz, 0), 1
        return (x, y, zz, zzz, 1), 0
    ppp, q = mul(pd, pp), mul(x, pp)
    x3 = sub(sqr(rd), add_2b(ppp, q))
    t = sub(q, x3)
    return (x3, sop2(rd, t, neg(y), ppp), mul(zz, pp), mul(zzz, ppp), 0), 0


# ---- worst cases --------------------------------------------------------------------------------------------------------------
def top_digit_bound(v):
    """largest |top digit| of a normalised value with |value| <= v p (v a Fraction)"""
    low = sum(HALF << (W * i) for i in range(L - 1))
    return int((v * P_INT + low) // (1 << (W * (L - 1)))) + 1


def digit_class(v, low=HALF):
    """digit limits of a normalised operand with |value| <= v p: `low` for digits 0..11, the value's share for the top digit"""
    return [low] * (L - 1) + [top_digit_bound(Fraction(v))]


def column_bounds(ops, square=False):
    """ops: digit-limit vectors (a, b[, c, d]).  The sum of the magnitudes of every term of every column, with |m_i| <= 2^29, the
    real |p_j|, and the carry's bound carried from column to column -> list of 25 bounds (Overflow if one reaches 2^63)."""
    out, carry = [], 0
    for k in range(2 * L - 1):
        lo, hi = (0, k) if k < L else (k - L + 1, L - 1)
        s = carry
        if square:
            a = ops[0]
            s += sum(a[i] * 2 * a[k - i] for i in range(lo, hi + 1) if 2 * i < k) + (a[k // 2] ** 2 if k % 2 == 0 else 0)
        else:
            for j in range(0, len(ops), 2):
                s += sum(ops[j][i] * ops[j + 1][k - i] for i in range(lo, hi + 1))
        s += sum(HALF * abs(PD[k - i]) for i in range(lo, (k if k < L else L - 1) + 1))   # the m_k p_0 term included
        if k >= L:
            s += HALF                                                                     # the rounding add
        if s >= 1 << 63:
            raise Overflow("column %d: 2^%.3f" % (k, __import__("math").log2(s)))
        out.append(s)
        carry = (s >> W) + 1
    assert carry < 1 << 31                                                                # the top digit fits its word
    return out


RHO = Fraction(1 << RBITS, P_INT)                                     # R' / p > 629.9
HALF_P = Fraction(1, 2) * (1 + Fraction(1, 1 << W)) + Fraction(1, 1 << 40)   # |m p| / R' in units of p, rounded up


def prod_bound(*pairs):
    """|sum a_i b_i / R'| + |m p / R'| in units of p"""
    return sum(Fraction(a) * Fraction(b) for a, b in pairs) / RHO + HALF_P


# the accumulator invariant of ec30s.cuh (|value| in units of p) and the base's class
INV_X, INV_Y, INV_Z = Fraction(202, 100), Fraction(61, 100), Fraction(1)
BASE = Fraction(64)


def madd_value_chain(x=INV_X, y=INV_Y, z=INV_Z, base=BASE):
    """value bounds of every intermediate of one mixed addition from the invariant -> dict"""
    b = {}
    b["u2"] = prod_bound((base, z))
    b["s2"] = prod_bound((base, z))
    b["pd"] = b["u2"] + x
    b["rd"] = b["s2"] + y
    b["pp"] = prod_bound((b["pd"], b["pd"]))
    b["rr"] = prod_bound((b["rd"], b["rd"]))
    b["ppp"] = prod_bound((b["pd"], b["pp"]))
    b["q"] = prod_bound((x, b["pp"]))
    b["e"] = b["ppp"] + 2 * b["q"]
    b["x3"] = b["rr"] + b["e"]
    b["t"] = b["q"] + b["x3"]
    b["y3"] = prod_bound((b["rd"], b["t"]), (y, b["ppp"]))
    b["zz3"] = prod_bound((z, b["pp"]))
    b["zzz3"] = prod_bound((z, b["ppp"]))
    b["first"] = prod_bound((base, 1))       # the first point of a bucket and from_bucket: one product with the residue 1 (< p)
    return b


def madd_products(b=None, x=INV_X, y=INV_Y, z=INV_Z, base=BASE, low=HALF):
    """every product of the mixed addition (and of from_bucket) with the digit limits of its operands: (name, square?, operands)"""
    b = b or madd_value_chain(x, y, z, base)
    c = lambda v: digit_class(v, low)
    return [
        ("first: x2 * 1", False, [c(base), c(1)]),
        ("u2 = x2 zz", False, [c(base), c(z)]),
        ("s2 = y2 zzz", False, [c(base), c(z)]),
        ("pp = pd^2", True, [c(b["pd"])]),
        ("rr = rd^2", True, [c(b["rd"])]),
        ("ppp = pd pp", False, [c(b["pd"]), c(b["pp"])]),
        ("q = x1 pp", False, [c(x), c(b["pp"])]),
        ("y3 = rd t - y1 ppp", False, [c(b["rd"]), c(b["t"]), c(y), c(b["ppp"])]),
        ("zz3 = zz pp", False, [c(z), c(b["pp"])]),
        ("zzz3 = zzz ppp", False, [c(z), c(b["ppp"])]),
    ]


MADD_PRODUCTS = madd_products


# ---- vectors: the class limits and random rows, as the raw-digit hooks of csrc/s30test.cuh take them ----------------------------
OPS = dict(mul=0, sqr=1, sop2=2, sub=3, add_2b=4, from_canonical_shl=5, to_canonical=6, madd=7)
ARITY = dict(mul=2, sqr=1, sop2=4, sub=2, add_2b=2, from_canonical_shl=1, to_canonical=1)
MADD_IN, MADD_OUT = 4 * L + 1 + 2 * L, 4 * L + 2


def edge_digits():
    """every digit at +-2^29, alternating signs, the digits a product can really leave, 0, +-1, +-(p - 1), +-2 p, +-2.5 p, and the
    largest repacked base (63 p + p - 1); top digits up to 2^23 (|value| < 2.63 p < 2^383: what ec30s.cuh's operands reach)"""
    out = []
    for top in (1 << 23, -(1 << 23), 0):
        out += [[HALF] * 12 + [top], [-HALF] * 12 + [top], [HALF if i & 1 else -HALF for i in range(12)] + [top],
                [-HALF if i & 1 else HALF for i in range(12)] + [top], [HALF - 1 if i & 1 else -HALF for i in range(12)] + [top]]
    out += [[0] * L, [1] + [0] * 12, [-1] + [0] * 12]
    for v in (P_INT - 1, 1 - P_INT, 2 * P_INT, -2 * P_INT, 5 * P_INT // 2, -(5 * P_INT // 2), (P_INT - 1) << SH):
        out.append(balanced(v))
    return out


def random_digits(rng, n, scale=1):
    """normalised rows with |value| <= about scale p"""
    out = []
    for _ in range(n):
        v = int.from_bytes(rng.bytes(48), "little") % (2 * scale * P_INT) - scale * P_INT
        out.append(balanced(v))
    return out


def op_rows(op, rng, nrand=64):
    """list of input rows (each a list of `arity` digit vectors, or of 12 canonical words for from_canonical_shl)"""
    e = edge_digits()
    if op == "from_canonical_shl":
        vals = [0, 1, P_INT - 1, P_INT >> 1, (1 << 380) - 1] + [int.from_bytes(rng.bytes(48), "little") % P_INT for _ in range(nrand)]
        return [[to_words(v)] for v in vals]
    if op == "to_canonical":
        k = consts()["OUT_K"]
        vals = [0, 1, -1, P_INT - 1, 1 - P_INT, P_INT, -P_INT, 2 * P_INT + 1, k * P_INT - 1, 1 - k * P_INT]
        return [[balanced(v)] for v in vals] + [[r] for r in random_digits(rng, nrand, 2)]
    a = ARITY[op]
    rnd = random_digits(rng, a * nrand, 2)
    rows = [[e[(i * (3 + j) + 5 * j + (i // len(e)) * (j + 1)) % len(e)] for j in range(a)] for i in range(len(e) * len(e) if a > 1 else len(e))]
    if a == 2:
        rows = [[x, y] for x in e for y in e]
    return rows + [rnd[i * a:(i + 1) * a] for i in range(nrand)]


def apply(op, row):
    f = dict(mul=mul, sqr=sqr, sop2=sop2, sub=sub, add_2b=add_2b)
    if op == "from_canonical_shl":
        return from_canonical_shl(row[0])
    if op == "to_canonical":
        return to_canonical(row[0]) + [0]
    return f[op](*row)


def pack_rows(op, rows):
    import numpy as np
    a = np.zeros((len(rows), ARITY[op] * L), dtype=np.int64)
    for t, row in enumerate(rows):
        for j, d in enumerate(row):
            a[t, j * L:j * L + len(d)] = d
    return (a & 0xffffffff).astype(np.uint32).view(np.int32)


def pack_madd(acc, xw, yw):
    x, y, zz, zzz, inf = acc
    return list(x) + list(y) + list(zz) + list(zzz) + [inf] + list(xw) + [0] + list(yw) + [0]


def madd_rows(points):
    """points: [(x words, y words)] affine, canonical.  A chain that reaches every branch: infinity -> first point, distinct points,
    the SAME point (equal: flag), P then -P (to infinity) and on from there.  -> (input rows, expected output rows)"""
    neg_y = lambda yw: to_words(P_INT - from_words(yw))
    zero = [0] * L
    acc = (zero, zero, zero, zero, 1)
    seq = []
    for i, (xw, yw) in enumerate(points):
        seq.append((xw, yw))
        if i % 4 == 1:
            seq.append((xw, neg_y(yw)))                # back out again
        if i % 4 == 2:
            seq.append((points[0][0], points[0][1]))   # some earlier point once more
    ins, outs = [], []
    # the same point onto itself, and P - P from a one-point accumulator
    first, _ = madd((zero, zero, zero, zero, 1), *points[0])
    for base in (points[0], (points[0][0], neg_y(points[0][1]))):
        nxt, eq = madd(first, *base)
        ins.append(pack_madd(first, *base))
        outs.append(pack_madd(nxt, [], [])[:4 * L + 1] + [eq])
    for xw, yw in seq:
        nxt, eq = madd(acc, xw, yw)
        ins.append(pack_madd(acc, xw, yw))
        outs.append(pack_madd(nxt, [], [])[:4 * L + 1] + [eq])
        acc = nxt
    return ins, outs
