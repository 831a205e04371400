"""Model of the differences folded into the products that compute them (csrc/fp30s.cuh: mul_sub, sqr_sub2; ec30s.cuh under
ARK_S30_FUSED_DIFF), beside tests/lazy30_model.py, whose operations stay the reference for every digit:

  mul_sub(a, b, s)  = a b / R' - s          must be  sub(mul(a, b), s)
  sqr_sub2(a, s, d) = a^2 / R' - s - 2 d    must be  sub(sqr(a), add_2b(s, d))

digit for digit.  Subtracting s R' from the double-width sum T touches columns 13..25 only, the quotient digits come from the low
13 columns, so (T - s R' + m p) / R' is the integer u - s; the high columns emit its balanced digits, which are unique.

`columns` runs the schedule of the header column by column with every partial sum checked against the signed 64-bit accumulator
and the final carry against its 32-bit word; `column_bounds` is the worst case of every column from the digit limits of the
operand classes and the real digits of p (lazy30_model.column_bounds with the new terms)."""
from fractions import Fraction

import lazy30_diet_model as D
import lazy30_model as M

W, L, HALF = M.W, M.L, M.HALF


def mul_sub(a, b, s):
    return M.balanced(M.val(M.mul(a, b)) - M.val(s))


def sqr_sub2(a, s, d):
    return M.balanced(M.val(M.sqr(a)) - M.val(s) - 2 * M.val(d))


def columns(a, b, s, d=None, square=False):
    """mul_sub (square = False; d = None) or sqr_sub2 (square = True; b unused) as fp30s.cuh schedules it: high column k takes
    - s[k - 13] (- 2 d[k - 13]) before its digit is cut, digit 12 leaves the final carry.  -> digits (Overflow if a partial sum
    leaves the signed 64-bit accumulator or the top digit its word)"""
    lim = 1 << 63
    m, r, t = [0] * L, [0] * L, 0

    def acc(t, v):
        t += v
        if not -lim <= t < lim:
            raise M.Overflow(t)
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
        for i in range(lo, (k - 1 if k < L else L - 1) + 1):
            t = acc(t, m[i] * M.PD[k - i])
        if k < L:
            m[k] = M.balanced(((t % (1 << 32)) * M.consts()["INV"]) % (1 << W), 1, top_free=False)[0]
            t = acc(t, m[k] * M.PD[0])
            assert t % (1 << W) == 0
        else:
            t = acc(t, -s[k - L])
            if d is not None:
                t = acc(t, -2 * d[k - L])
            r[k - L] = M.balanced(t % (1 << W), 1, top_free=False)[0]
            t = acc(t, HALF)
        t >>= W
    if not -(1 << 31) <= t < (1 << 31):
        raise M.Overflow(t)
    t -= s[L - 1] + (2 * d[L - 1] if d is not None else 0)
    if not -(1 << 31) <= t < (1 << 31):
        raise M.Overflow(t)
    r[L - 1] = t
    return r


def column_bounds(ops, s, d=None, square=False):
    """ops: digit-limit vectors of the product's operands (a, b) or (a,) for a square; s, d: digit limits of what is subtracted.
    The sum of the magnitudes of every term of every column -> 25 column bounds and the bound of the top digit (Overflow if a
    column reaches 2^63 or the top digit 2^31)"""
    out, carry = [], 0
    for k in range(2 * L - 1):
        lo, hi = (0, k) if k < L else (k - L + 1, L - 1)
        t = carry
        if square:
            a = ops[0]
            t += sum(a[i] * 2 * a[k - i] for i in range(lo, hi + 1) if 2 * i < k) + (a[k // 2] ** 2 if k % 2 == 0 else 0)
        else:
            t += sum(ops[0][i] * ops[1][k - i] for i in range(lo, hi + 1))
        t += sum(HALF * abs(M.PD[k - i]) for i in range(lo, (k if k < L else L - 1) + 1))
        if k >= L:
            t += s[k - L] + (2 * d[k - L] if d is not None else 0) + HALF
        if t >= 1 << 63:
            raise M.Overflow("column %d: 2^%.3f" % (k, __import__("math").log2(t)))
        out.append(t)
        carry = (t >> W) + 1
    top = carry + s[L - 1] + (2 * d[L - 1] if d is not None else 0)
    if top >= 1 << 31:
        raise M.Overflow("top digit")
    return out, top


def fused_products(b=None):
    """the three fused products of the mixed addition with the digit limits of their operands, from the value chain of
    lazy30_model: (name, square?, product operands, s, d)"""
    b = b or M.madd_value_chain()
    c = M.digit_class
    return [
        ("pd = x2 zz - x1", False, [D.U_CLASS, c(M.INV_Z)], c(M.INV_X), None),
        ("rd = y2 zzz - y1", False, [D.U_CLASS, c(M.INV_Z)], c(M.INV_Y), None),
        ("x3 = rd^2 - ppp - 2 q", True, [c(b["rd"])], c(b["ppp"]), c(b["q"])),
    ]


# ---- rows for the raw-digit hook ops (csrc/s30test_api.hpp: MUL_SUB, SQR_SUB2, after lazy30_diet_model.OPS) -------------------------
OPS = dict(mul_sub=10, sqr_sub2=11)


def edge_rows():
    """every digit at +-2^29 with the top digits at the limits of their classes in the mixed addition, the signs chosen so that the
    product terms of a column and what is subtracted all agree (both ways round), alternating digits, an unsigned gathered operand
    at its limit -> {op: rows of three digit vectors}"""
    b = M.madd_value_chain()
    top = lambda v: M.top_digit_bound(Fraction(v))
    full = lambda sign, t: [sign * HALF] * (L - 1) + [sign * t]
    alt = lambda sign, t: [sign * (HALF if i & 1 else -HALF) for i in range(L - 1)] + [sign * t]
    u = [(1 << W) - 1] * (L - 1) + [(1 << 27) - 1]
    ms, sq = [], []
    for sa in (1, -1):
        for sb in (1, -1):
            for ss in (1, -1):                          # ss = -sa sb: every term of a high column has one sign
                ms.append([full(sa, top(M.INV_Z)), full(sb, top(M.INV_Z)), full(ss, top(M.INV_X))])
                ms.append([alt(sa, top(M.INV_Z)), alt(sb, top(M.INV_Z)), full(ss, top(M.INV_X))])
        for ss in (1, -1):
            ms.append([u, full(sa, top(M.INV_Z)), full(ss, top(M.INV_X))])
            ms.append([u, alt(sa, top(M.INV_Z)), alt(ss, top(M.INV_Y))])
            for sd in (1, -1):                          # ss = sd = -1: a square's terms are positive, so are - s and - 2 d
                sq.append([full(sa, top(b["rd"])), full(ss, top(b["ppp"])), full(sd, top(b["q"]))])
                sq.append([alt(sa, top(b["rd"])), full(ss, top(b["ppp"])), full(sd, top(b["q"]))])
                sq.append([full(sa, top(b["rd"])), alt(ss, top(b["ppp"])), alt(sd, top(b["q"]))])
    zero = [0] * L
    one = [1] + [0] * (L - 1)
    ms += [[zero, zero, zero], [zero, one, full(1, 0)], [one, M.neg(one), full(-1, 0)], [M.balanced(M.P_INT - 1), M.balanced(1 - M.P_INT), M.balanced(2 * M.P_INT)]]
    sq += [[zero, zero, zero], [zero, full(1, 0), full(1, 0)], [one, full(-1, 0), full(-1, 0)], [M.balanced(M.P_INT - 1), M.balanced(-2 * M.P_INT), M.balanced(2 * M.P_INT)]]
    return dict(mul_sub=ms, sqr_sub2=sq)


def op_rows(op, rng, nrand=64):
    """the edge rows and `nrand` random rows (normalised operands of a few p; every fourth product with an unsigned gathered operand)"""
    rows = list(edge_rows()[op])
    rnd = M.random_digits(rng, 3 * nrand, 2)
    for i in range(nrand):
        row = rnd[3 * i:3 * i + 3]
        if op == "mul_sub" and i % 4 == 0:
            row[0] = D.from_canonical_u(M.to_words(int.from_bytes(rng.bytes(48), "little") % M.P_INT))
        rows.append(row)
    return rows


def apply(op, row):
    return mul_sub(*row) if op == "mul_sub" else sqr_sub2(*row)


def unfused(op, row):
    """the chain the fused operation replaces, from lazy30_model's own operations"""
    if op == "mul_sub":
        return M.sub(M.mul(row[0], row[1]), row[2])
    return M.sub(M.sqr(row[0]), M.add_2b(row[1], row[2]))


def pack_rows(rows):
    import numpy as np
    a = np.zeros((len(rows), len(rows[0]) * L), dtype=np.int64)
    for t, row in enumerate(rows):
        for j, d in enumerate(row):
            a[t, j * L:(j + 1) * L] = d
    return (a & 0xffffffff).astype(np.uint32).view(np.int32)


# ---- rows for the mixed addition (op 7 of lazy30_model.OPS) beyond lazy30_model.madd_rows -------------------------------------------
def reload(acc):
    """a stored bucket brought back (s30_from_bucket): canonical words, the signed repack, one product with the residue 1"""
    one = M.consts()["ONE"]
    return tuple(M.mul(M.from_canonical_shl(M.to_canonical(c)), one) for c in acc[:4]) + (acc[4],)


def madd_extra_rows(points):
    """points: [(x words, y words)] affine, canonical.  A RELOADED accumulator meeting another point, its own point and its own
    point's inverse; accumulators at the limits of the invariant (|x| < 2.02, |y| < 0.61, |zz|, |zzz| < 1 in units of p, both
    signs -- field values only, the addition is arithmetic) meeting a point.  -> (input rows, expected rows) as madd_rows"""
    neg_y = lambda yw: M.to_words(M.P_INT - M.from_words(yw))
    zero = [0] * L
    first, _ = M.madd((zero, zero, zero, zero, 1), *points[0])
    two, _ = M.madd(first, *points[1])
    accs = [(reload(two), points[4]), (reload(first), points[0]), (reload(first), (points[0][0], neg_y(points[0][1])))]
    lim = lambda v, sign: M.balanced(sign * int(Fraction(v) * M.P_INT - 1))
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                accs.append(((lim(M.INV_X, sx), lim(M.INV_Y, sy), lim(M.INV_Z, sz), lim(M.INV_Z, -sz), 0), points[3]))
    ins, outs = [], []
    for acc, (xw, yw) in accs:
        nxt, eq = M.madd(acc, xw, yw)
        ins.append(M.pack_madd(acc, xw, yw))
        outs.append(M.pack_madd(nxt, [], [])[:4 * L + 1] + [eq])
    return ins, outs
