"""Model of the UNSIGNED gathered coordinate of the accumulate kernel's mixed addition (csrc/fp30s.cuh: from_canonical_u;
ec30s.cuh: s30_from_affine), beside tests/lazy30_model.py, whose operations stay the reference for every digit: the repack
(digits in [0, 2^30), top digit below 2^27, no carry chain), its operand class (`U_CLASS`) for lazy30_model.column_bounds, and
the mixed addition with the gathered operands in that form, every product run column by column (lazy30_model.columns) so that
an overflow of the signed 64-bit accumulator would show."""
import lazy30_model as M

W, L, HALF = M.W, M.L, M.HALF
MASK = (1 << W) - 1

# the gathered class: what from_canonical_u can leave (digits < 2^30, top digit < 2^27), rounded up
U_CLASS = [1 << W] * (L - 1) + [(1 << 27) + 1]


def from_canonical_u(w):
    x = M.from_words(w) << M.SH
    return [(x >> (W * i)) & MASK for i in range(L - 1)] + [x >> (W * (L - 1))]


def madd(acc, x2w, y2w, sign=0):
    """the kernel's entry to the mixed addition (LazySK::madd): the digit's sign on the canonical y, the unsigned repack, the
    addition with U2, S2 and the first point's products run through the column schedule.  -> what lazy30_model.madd returns"""
    x, y, zz, zzz, inf = acc
    if sign:
        y2w = M.to_words((M.P_INT - M.from_words(y2w)) % M.P_INT)
    x2, y2 = from_canonical_u(x2w), from_canonical_u(y2w)
    one = M.consts()["ONE"]
    if inf:
        return (M.columns(x2, one), M.columns(y2, one), list(one), list(one), 0), 0
    u2, s2 = M.columns(x2, zz), M.columns(y2, zzz)
    pd, rd = M.sub(u2, x), M.sub(s2, y)
    pp = M.sqr(pd)
    if not any(pp):
        if not any(M.sqr(rd)):
            return (x, y, zz, zzz, 0), 1
        return (x, y, zz, zzz, 1), 0
    ppp, q = M.mul(pd, pp), M.mul(x, pp)
    x3 = M.sub(M.sqr(rd), M.add_2b(ppp, q))
    t = M.sub(q, x3)
    return (x3, M.sop2(rd, t, M.neg(y), ppp), M.mul(zz, pp), M.mul(zzz, ppp), 0), 0


def curve_points(n):
    """G, 2 G, ... n G of BLS12-381 G1 (y^2 = x^3 + 4) as (x words, y words), canonical Montgomery form (radix 2^384)"""
    p = M.P_INT
    gx = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
    gy = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
    out, x, y = [], gx, gy
    for _ in range(n):
        assert (y * y - x * x * x - 4) % p == 0
        out.append((M.to_words((x << 384) % p), M.to_words((y << 384) % p)))
        lam = (3 * x * x * pow(2 * y, -1, p) if (x, y) == (gx, gy) else (y - gy) * pow(x - gx, -1, p)) % p
        x3 = (lam * lam - x - gx) % p
        x, y = x3, (lam * (x - x3) - y) % p
    return out


# ---- raw-digit hook ops added after lazy30_model.OPS (csrc/s30test_api.hpp) ------------------------------------------------------
OPS = dict(from_canonical_u=8, madd_entry=9)
MADD_IN = M.MADD_IN + 1     # lazy30_model.pack_madd's row, then 1 for a negative digit
