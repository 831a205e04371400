"""Model of the FULL addition on 13 signed 30-bit digits (csrc/ec30s.cuh: xyzz_add_s, xyzz_dbl_s, s30_operands_of), beside
tests/lazy30_model.py, whose operations stay the reference for every digit.

Both operands of a full addition are sums, not gathered bases, so the bounds of the mixed addition do not carry over; they are
restated here from the same accumulator invariant

    |x| < 2.02,  |y| < 0.61,  |zz|, |zzz| < 1        (units of p)

with the operand b at the widest class it can have: a stored point's coordinates, unsigned digits of a value in [0, 64 p)
(lazy30_diet_model.U_CLASS) -- another accumulator (inside the invariant, normalised) is narrower in value and in every digit.

  * `add` and `double` are the addition and its doubling digit for digit, their products run column by column (an overflow of the
    64-bit accumulator would show);
  * `add_value_chain` the value bounds, exact rationals, from the invariant through one addition and back into it;
  * `add_products` every product with the digit limits of its operands, for lazy30_model.column_bounds and
    lazy30_fused_model.column_bounds; `dbl_value_chain` and `dbl_products` the same for the doubling.
"""
from fractions import Fraction

import lazy30_diet_model as D
import lazy30_fused_model as FM
import lazy30_model as M

W, L, HALF = M.W, M.L, M.HALF
INV_X, INV_Y, INV_Z, BASE = M.INV_X, M.INV_Y, M.INV_Z, M.BASE


# ---- the addition, digit for digit --------------------------------------------------------------------------------------------
def operands_of(words4):
    """s30_operands_of: four coordinates in canonical words -> unsigned digits; infinity is zz = 0"""
    x, y, zz, zzz = (D.from_canonical_u(w) for w in words4)
    return (x, y, zz, zzz, 0 if any(words4[2]) else 1)


def double(acc):
    """xyzz_dbl_s: dbl-2008-s-1 (a = 0) on the digits of an accumulator that is not at infinity"""
    x1, y1, zz1, zzz1, _ = acc
    u = M.sweep([2 * d for d in y1])
    v = M.columns(u, None, square=True)
    w, s = M.columns(u, v), M.columns(x1, v)
    xx = M.columns(x1, None, square=True)
    m = M.add_2b(xx, xx)
    x3 = FM.columns(m, None, [0] * L, s, square=True)
    t = M.sub(s, x3)
    return (x3, M.columns(m, t, M.neg(w), y1), M.columns(v, zz1), M.columns(w, zzz1), 0)


def field_double(a):
    """dbl-2008-s-1 on residues mod p"""
    p = M.P_INT
    x1, y1, zz1, zzz1 = a
    u = 2 * y1 % p
    v = u * u % p
    w, s, m = u * v % p, x1 * v % p, 3 * x1 * x1 % p
    x3 = (m * m - 2 * s) % p
    return (x3, (m * (s - x3) - w * y1) % p, v * zz1 % p, w * zzz1 % p)


def add(acc, b, doubling=double):
    """xyzz_add_s on accumulators (x, y, zz, zzz, inf).  `doubling`: what equal points do (xyzz_dbl_s on the accumulator)"""
    x1, y1, zz1, zzz1, inf1 = acc
    x2, y2, zz2, zzz2, inf2 = b
    one = M.consts()["ONE"]
    if inf2:
        return acc
    if inf1:
        return (M.columns(x2, one), M.columns(y2, one), M.columns(zz2, one), M.columns(zzz2, one), 0)
    u1, s1 = M.columns(x1, zz2), M.columns(y1, zzz2)
    pd, rd = FM.columns(x2, zz1, u1), FM.columns(y2, zzz1, s1)
    pp = M.sqr(pd)
    if not any(pp):
        if not any(M.sqr(rd)):
            return doubling(acc)
        return (x1, y1, zz1, zzz1, 1)
    ppp, q = M.columns(pd, pp), M.columns(u1, pp)
    x3 = FM.columns(rd, None, ppp, q, square=True)
    t = M.sub(q, x3)
    y3 = M.columns(rd, t, M.neg(s1), ppp)
    return (x3, y3, M.columns(M.columns(zz1, zz2), pp), M.columns(M.columns(zzz1, zzz2), ppp), 0)


def field_add(a, b):
    """add-2008-s on residues mod p (a, b: (x, y, zz, zzz) integers, neither at infinity, different x) -> (x, y, zz, zzz)"""
    p = M.P_INT
    x1, y1, zz1, zzz1 = a
    x2, y2, zz2, zzz2 = b
    u1, u2, s1, s2 = x1 * zz2 % p, x2 * zz1 % p, y1 * zzz2 % p, y2 * zzz1 % p
    pd, rd = (u2 - u1) % p, (s2 - s1) % p
    pp = pd * pd % p
    ppp, q = pd * pp % p, u1 * pp % p
    x3 = (rd * rd - ppp - 2 * q) % p
    return (x3, (rd * (q - x3) - s1 * ppp) % p, zz1 * zz2 * pp % p, zzz1 * zzz2 * ppp % p)


def residue(d):
    """the field element a digit vector holds: value / R' mod p"""
    return M.val(d) * pow(1 << M.RBITS, -1, M.P_INT) % M.P_INT


# ---- worst cases -----------------------------------------------------------------------------------------------------------------
def add_value_chain(x=INV_X, y=INV_Y, z=INV_Z, b=BASE):
    """value bounds of every intermediate of one full addition: accumulator at the invariant, every coordinate of b at `b`"""
    v = {}
    v["u1"] = M.prod_bound((x, b))
    v["s1"] = M.prod_bound((y, b))
    v["u2"] = M.prod_bound((b, z))
    v["s2"] = M.prod_bound((b, z))
    v["pd"] = v["u2"] + v["u1"]
    v["rd"] = v["s2"] + v["s1"]
    v["pp"] = M.prod_bound((v["pd"], v["pd"]))
    v["rr"] = M.prod_bound((v["rd"], v["rd"]))
    v["ppp"] = M.prod_bound((v["pd"], v["pp"]))
    v["q"] = M.prod_bound((v["u1"], v["pp"]))
    v["x3"] = v["rr"] + v["ppp"] + 2 * v["q"]
    v["t"] = v["q"] + v["x3"]
    v["y3"] = M.prod_bound((v["rd"], v["t"]), (v["s1"], v["ppp"]))
    v["zz12"] = M.prod_bound((z, b))
    v["zz3"] = M.prod_bound((v["zz12"], v["pp"]))
    v["zzz3"] = M.prod_bound((v["zz12"], v["ppp"]))
    v["copy"] = M.prod_bound((b, 1))          # an empty accumulator takes b through one product with the residue 1 (< p)
    return v


def add_products(v=None, x=INV_X, y=INV_Y, z=INV_Z, b_class=None):
    """every product of the full addition: (name, kind, product operands, s, d) with kind 'mul', 'sqr', 'sop2', 'mul_sub' or
    'sqr_sub2'; digit limits per operand.  b_class: the digit limits of b's coordinates (default: the unsigned stored class)"""
    v = v or add_value_chain(x, y, z)
    c = M.digit_class
    u = b_class or D.U_CLASS
    return [
        ("copy: b * 1", "mul", [u, c(1)], None, None),
        ("u1 = x1 zz2", "mul", [c(x), u], None, None),
        ("s1 = y1 zzz2", "mul", [c(y), u], None, None),
        ("pd = x2 zz1 - u1", "mul_sub", [u, c(z)], c(v["u1"]), None),
        ("rd = y2 zzz1 - s1", "mul_sub", [u, c(z)], c(v["s1"]), None),
        ("pp = pd^2", "sqr", [c(v["pd"])], None, None),
        ("rr = rd^2", "sqr", [c(v["rd"])], None, None),
        ("ppp = pd pp", "mul", [c(v["pd"]), c(v["pp"])], None, None),
        ("q = u1 pp", "mul", [c(v["u1"]), c(v["pp"])], None, None),
        ("x3 = rd^2 - ppp - 2 q", "sqr_sub2", [c(v["rd"])], c(v["ppp"]), c(v["q"])),
        ("y3 = rd t - s1 ppp", "sop2", [c(v["rd"]), c(v["t"]), c(v["s1"]), c(v["ppp"])], None, None),
        ("zz12 = zz1 zz2", "mul", [c(z), u], None, None),
        ("zz3 = zz12 pp", "mul", [c(v["zz12"]), c(v["pp"])], None, None),
        ("zzz3 = zzz12 ppp", "mul", [c(v["zz12"]), c(v["ppp"])], None, None),
    ]


def dbl_value_chain(x=INV_X, y=INV_Y, z=INV_Z):
    """value bounds of the doubling of an accumulator at the invariant"""
    v = {}
    v["u"] = 2 * y
    v["v"] = M.prod_bound((v["u"], v["u"]))
    v["w"] = M.prod_bound((v["u"], v["v"]))
    v["s"] = M.prod_bound((x, v["v"]))
    v["xx"] = M.prod_bound((x, x))
    v["m"] = 3 * v["xx"]
    v["x3"] = M.prod_bound((v["m"], v["m"])) + 2 * v["s"]
    v["t"] = v["s"] + v["x3"]
    v["y3"] = M.prod_bound((v["m"], v["t"]), (v["w"], y))
    v["zz3"] = M.prod_bound((v["v"], z))
    v["zzz3"] = M.prod_bound((v["w"], z))
    return v


def dbl_products(v=None, x=INV_X, y=INV_Y, z=INV_Z):
    """every product of the doubling, as add_products lists them"""
    v = v or dbl_value_chain(x, y, z)
    c = M.digit_class
    return [
        ("v = u^2", "sqr", [c(v["u"])], None, None),
        ("w = u v", "mul", [c(v["u"]), c(v["v"])], None, None),
        ("s = x1 v", "mul", [c(x), c(v["v"])], None, None),
        ("xx = x1^2", "sqr", [c(x)], None, None),
        ("x3 = m^2 - 2 s", "sqr_sub2", [c(v["m"])], [0] * L, c(v["s"])),
        ("y3 = m t - w y1", "sop2", [c(v["m"]), c(v["t"]), c(v["w"]), c(y)], None, None),
        ("zz3 = v zz1", "mul", [c(v["v"]), c(z)], None, None),
        ("zzz3 = w zzz1", "mul", [c(v["w"]), c(z)], None, None),
    ]


def column_maxima(products):
    """{name: (largest column bound, bound of the top digit or None)} -- Overflow if a column reaches 2^63"""
    out = {}
    for name, kind, ops, s, d in products:
        if kind in ("mul", "sop2"):
            out[name] = (max(M.column_bounds(ops)), None)
        elif kind == "sqr":
            out[name] = (max(M.column_bounds(ops, square=True)), None)
        else:
            cols, top = FM.column_bounds(ops, s, d, square=kind == "sqr_sub2")
            out[name] = (max(cols), top)
    return out


# ---- rows for the raw-digit hook ops (csrc/s30test_api.hpp: ADD_FULL, ADD_FULL_ACC, after lazy30_fused_model.OPS) ---------------------
OPS = dict(add_full=12, add_full_acc=13)
ADD_IN, ADD_OUT = 8 * L, 4 * L


def pack_points(a4, b4):
    """two stored points (4 x 12 canonical 32-bit words each) -> one input row of 8 slots"""
    row = []
    for w in list(a4) + list(b4):
        row += [int(t) for t in w] + [0] * (L - M.N32)
    return row
