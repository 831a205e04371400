"""Planted points and the Python-integer model for the base-set check (ark_hip_sw_check*, csrc/pointcheck.cuh), built on
tests/pyref.py: independent of the library and of the oracle's arithmetic.

    planted(cname)                      the planted points of a curve, by class (counts asserted)
    model_status(cname, row, checks, method)   the status byte the library must give for one point's limbs

Classes (status under checks = 3):
    valid          chain points [3 + 5 i] G and the identity (0, 0)                                       -> 0
    not_reduced    a valid point with p added to one Fp component's integer where it still fits the limbs, and a
                   component of all-ones limbs; over Fp2 each component separately                          -> 1
    off_curve      a valid point with one limb of y changed, and (x, y) swapped                           -> 2
    off_subgroup   random curve points Q (random x until x^3 + b is a square) and [r]Q                      -> 3
                   (BN254 G1 has cofactor one: every curve point passes, -> 0)
    small_order    points whose order is so small that the ladder's accumulator meets +-P in the middle:
                   order 3 (0, +-sqrt b) on BLS12-381 G1 and BLS12-377 G1 (b is a square there and on none of the
                   other three), order 2 (p - 1, 0) on BLS12-377 G1, order 11 [(h / 121) r] Q on BLS12-381 G1,
                   order 13 [(h2 / 169) r] Q on BLS12-381 G2                                                -> 3
                   BLS12-377 G2 has no prime factor of its cofactor below 200 000 and gets no small-order case; it
                   shares the kernel template with BLS12-381 G2.
"""
import collections
import functools

import numpy as np

import point_fixtures as PF
import pyref as P

BLS12_381_X = -0xd201000000010000
COFACTOR_ONE = ("BN254_G1",)
Planted = collections.namedtuple("Planted", "name cls row")
CLASS_STATUS = {"valid": 0, "not_reduced": 1, "off_curve": 2, "off_subgroup": 3, "small_order": 3}
# points per class and curve: nothing may be dropped
COUNTS = {
    "BN254_G1": {"valid": 7, "not_reduced": 4, "off_curve": 4, "off_subgroup": 6, "small_order": 0},
    "BLS12_381_G1": {"valid": 7, "not_reduced": 4, "off_curve": 4, "off_subgroup": 6, "small_order": 4},
    "BLS12_377_G1": {"valid": 7, "not_reduced": 4, "off_curve": 4, "off_subgroup": 6, "small_order": 3},
    "BLS12_377_G2": {"valid": 7, "not_reduced": 8, "off_curve": 4, "off_subgroup": 6, "small_order": 0},
    "BLS12_381_G2": {"valid": 7, "not_reduced": 8, "off_curve": 4, "off_subgroup": 6, "small_order": 2},
}


# ---- square roots ---------------------------------------------------------------------------------------------------
def sqrt_fp(a, p):
    """a square root of a mod p, or None (Tonelli-Shanks)"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    s, q = P.two_adicity(p)
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        t, r = t * c % p, r * b % p
    return r


def sqrt_fp2(a, p, beta):
    """a square root of a = (a0, a1) in Fp[u] / (u^2 - beta), or None (norm method)"""
    a0, a1 = a[0] % p, a[1] % p
    if a1 == 0:
        r = sqrt_fp(a0, p)
        if r is not None:
            return (r, 0)
        r = sqrt_fp(a0 * pow(beta, -1, p) % p, p)      # a0 = beta r^2 = (r u)^2
        return None if r is None else (0, r)
    n = sqrt_fp((a0 * a0 - beta * a1 * a1) % p, p)
    if n is None:
        return None
    half = pow(2, -1, p)
    for nn in (n, p - n):
        x0 = sqrt_fp((a0 + nn) * half % p, p)
        if x0:
            return (x0, a1 * pow(2 * x0, -1, p) % p)
    return None


def sqrt_f(cv, a):
    return sqrt_fp(a, cv.p) if cv.F.beta is None else sqrt_fp2(a, cv.p, cv.F.beta)


# ---- the unreduced ladder (pyref.Curve.mul reduces the scalar mod r) -------------------------------------------------
def ladder(cv, pt, k, meets=None):
    """[k] pt for any integer k >= 0 by left-to-right double-and-add on pyref's exact affine addition.  meets (a list):
    gets one entry per addition in which the accumulator had pt's x coordinate (it was +-pt)."""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = cv.add(acc, acc)
        if bit == "1":
            if meets is not None and acc is not None and pt is not None and acc[0] == pt[0]:
                meets.append(acc[1] == pt[1])
            acc = cv.add(acc, pt)
    return acc


@functools.lru_cache(maxsize=None)
def endo_beta():
    """the cube root of unity of BLS12-381 Fq with (beta x, y) = -[x^2](x, y) on the subgroup, read from the generated header
    (tools/gen_constants.py derives it and asserts the relation on the generator; test_check_bases_host.py asserts it again)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "algebra_amd", "csrc", "check_consts.hpp")).read()
    body = txt[txt.index("struct CHECK_BLS12_381_G1"):]
    limbs = re.search(r"ENDO_BETA\[12\] = \{([^}]*)\}", body).group(1)
    v = 0
    for i, w in enumerate(limbs.split(",")):
        v |= int(w.strip().rstrip("u"), 16) << (32 * i)
    p = P.MODULI["BLS12_381_FQ"][0]
    return v * pow(P.R_of(p), -1, p) % p


# ---- the model ---------------------------------------------------------------------------------------------------------
def _components(cv, row):
    n = P.nlimbs(cv.p)
    row = np.asarray(row, dtype=np.uint64).reshape(-1)
    assert row.size == 2 * cv.fw
    return [P.from_limbs(row[i * n:(i + 1) * n]) for i in range(2 * cv.fw // n)]


@functools.lru_cache(maxsize=None)
def _facts(cname, key):
    """(reduced, point, on_curve, [r]P == O, phi(P) == -[x^2]P or None) of one point's limbs"""
    cv = PF.curve(cname)
    row = np.frombuffer(key, dtype=np.uint64)
    if any(c >= cv.p for c in _components(cv, row)):
        return (False, None, None, None, None)
    pt = cv.dec(row)
    on = cv.on_curve(pt)
    if pt is None:
        return (True, None, True, True, True)
    in_r = ladder(cv, pt, cv.r) is None
    in_e = None
    if cname == "BLS12_381_G1":
        x2 = BLS12_381_X ** 2
        lhs = (endo_beta() * pt[0] % cv.p, pt[1])
        in_e = lhs == cv.neg(ladder(cv, pt, x2))
    return (True, pt, on, in_r, in_e)


def model_status(cname, row, checks, method=1):
    """the status byte for one point (2 * fe_words u64 limbs): 1 under every mask for a coordinate that is no field element;
    2 if bit 0 of checks is set and the point is off the curve; 3 if bit 1 is set and the subgroup test fails"""
    assert checks in (1, 2, 3) and method in (1, 2)
    assert method == 1 or cname == "BLS12_381_G1"
    reduced, pt, on, in_r, in_e = _facts(cname, np.ascontiguousarray(row, dtype=np.uint64).tobytes())
    if not reduced:
        return 1
    if (checks & 1) and not on:
        return 2
    if (checks & 2) and pt is not None and cname not in COFACTOR_ONE:
        if not (in_r if method == 1 else in_e):
            return 3
    return 0


def model(cname, rows, checks, method=1):
    """(status bytes, [first_bad, n1, n2, n3]) for an array of points"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 2 * PF.curve(cname).fw)
    st = np.array([model_status(cname, r, checks, method) for r in rows], dtype=np.uint8)
    bad = np.nonzero(st)[0]
    return st, [int(bad[0]) if bad.size else len(rows)] + [int((st == k).sum()) for k in (1, 2, 3)]


# ---- the planted points --------------------------------------------------------------------------------------------------
def _random_curve_point(cv, rng):
    F = cv.F
    while True:
        rnd = lambda: int.from_bytes(rng.bytes(56), "little") % cv.p     # noqa: E731
        x = rnd() if F.beta is None else (rnd(), rnd())
        y = sqrt_f(cv, F.add(F.mul(F.mul(x, x), x), cv.b))
        if y is not None and y != F.zero():
            assert cv.on_curve((x, y))
            return (x, y)


def _with_component(cv, row, k, value):
    """the limbs of `row` with Fp component k (x.c0, [x.c1,] y.c0, [y.c1]) replaced by the integer `value`"""
    n = P.nlimbs(cv.p)
    out = np.array(row, dtype=np.uint64)
    out[k * n:(k + 1) * n] = P.to_limbs(value, n)
    return out


def _cofactor_multiple(cv, cname, rng, h, q):
    """a point of order exactly q: [(h / q^2) r] Q for random curve points Q until it is not the identity"""
    assert h % (q * q) == 0
    while True:
        Q = _random_curve_point(cv, rng)
        assert ladder(cv, Q, h * cv.r) is None, "h r kills every curve point"
        T = ladder(cv, Q, (h // (q * q)) * cv.r)
        if T is not None and ladder(cv, T, q) is None:
            return T


@functools.lru_cache(maxsize=None)
def planted(cname):
    cv = PF.curve(cname)
    F, p = cv.F, cv.p
    n = P.nlimbs(p)
    ncomp = 2 * cv.fw // n
    rng = np.random.default_rng(0xC4EC + P.CURVE_ORDER.index(cname))
    out = []
    chain = PF.affine_chain(cname, 6)
    for i, pt in enumerate(chain):
        out.append(Planted("chain%d" % i, "valid", cv.enc(pt)))
    out.append(Planted("identity", "valid", cv.enc(None)))
    # not reduced: + p on one component (it still fits the limbs), all-ones limbs in one component
    base = cv.enc(chain[1])
    comps = _components(cv, base)
    for k in range(ncomp):
        assert comps[k] + p < 1 << (64 * n)
        out.append(Planted("plus_p_%d" % k, "not_reduced", _with_component(cv, base, k, comps[k] + p)))
    for k in range(ncomp):
        out.append(Planted("ones_%d" % k, "not_reduced", _with_component(cv, cv.enc(chain[2 + k % 2]), k, (1 << (64 * n)) - 1)))
    # off the curve
    for i in (0, 4):
        row = cv.enc(chain[i])
        row[cv.fw + (i % n)] ^= np.uint64(1 << (7 * i))
        out.append(Planted("y_limb_%d" % i, "off_curve", row))
        x, y = chain[i]
        out.append(Planted("swapped_%d" % i, "off_curve", cv.enc((y, x))))
    # on the curve, outside the subgroup (BN254 G1: cofactor one, these pass)
    for i in range(3):
        Q = _random_curve_point(cv, rng)
        rQ = ladder(cv, Q, cv.r)
        if cname in COFACTOR_ONE:
            assert rQ is None
            Q2 = _random_curve_point(cv, rng)
            out.append(Planted("random%d" % i, "off_subgroup", cv.enc(Q)))
            out.append(Planted("random%db" % i, "off_subgroup", cv.enc(Q2)))
        else:
            assert rQ is not None and ladder(cv, rQ, cv.r) is not None
            out.append(Planted("random%d" % i, "off_subgroup", cv.enc(Q)))
            out.append(Planted("r_random%d" % i, "off_subgroup", cv.enc(rQ)))
    # small order
    small = []
    x = BLS12_381_X
    if cname in ("BLS12_381_G1", "BLS12_377_G1"):
        sb = sqrt_fp(cv.b, p)
        assert sb is not None
        for y in (sb, p - sb):
            small.append(("order3_%s" % ("a" if y == sb else "b"), (0, y), 3, True))
    else:
        assert sqrt_f(cv, cv.b) is None      # b is a square on neither of the other three
    if cname == "BLS12_377_G1":
        small.append(("order2", (p - 1, 0), 2, False))
    if cname == "BLS12_381_G1":
        assert cv.r == x ** 4 - x ** 2 + 1 and (x - 1) ** 2 % 3 == 0
        T = _cofactor_multiple(cv, cname, rng, (x - 1) ** 2 // 3, 11)
        small += [("order11", T, 11, True), ("order11_neg", cv.neg(T), 11, True)]
    if cname == "BLS12_381_G2":
        assert cv.r == x ** 4 - x ** 2 + 1
        h2num = x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13
        assert h2num % 9 == 0
        T = _cofactor_multiple(cv, cname, rng, h2num // 9, 13)
        small += [("order13", T, 13, True), ("order13_neg", cv.neg(T), 13, True)]
    for name, pt, order, must_meet in small:
        assert cv.on_curve(pt) and ladder(cv, pt, order) is None
        assert all(ladder(cv, pt, d) is not None for d in range(1, order))
        meets = []
        assert ladder(cv, pt, cv.r, meets) is not None      # r is prime to the order
        if must_meet:
            assert len(meets) > 0, "%s no longer makes the ladder's accumulator meet +-P" % name
        out.append(Planted(name, "small_order", cv.enc(pt)))
    counts = collections.Counter(q.cls for q in out)
    assert dict((k, counts.get(k, 0)) for k in COUNTS[cname]) == COUNTS[cname], (cname, counts)
    assert len(set(q.row.tobytes() for q in out)) == len(out)
    for q in out:     # the class is what the model says under the full mask
        want = 0 if (cname in COFACTOR_ONE and q.cls == "off_subgroup") else CLASS_STATUS[q.cls]
        assert model_status(cname, q.row, 3) == want, (cname, q.name)
    return tuple(out)


def planted_rows(cname):
    return np.stack([q.row for q in planted(cname)])


def ladder_meets(cname, name):
    """how often the ladder over r adds with the accumulator at +-P for the planted point `name`"""
    cv = PF.curve(cname)
    q = [q for q in planted(cname) if q.name == name][0]
    meets = []
    ladder(cv, cv.dec(q.row), cv.r, meets)
    return len(meets)


PLANT_AT = (0, 1, 63, 64, 65, 127, 128, 255, 256)


@functools.lru_cache(maxsize=None)
def _chain_rows(cname, n):
    """n valid points [7 + 11 i] G as limbs.  They pass every stage BY CONSTRUCTION: [r]G = O (asserted here with the
    unreduced ladder), so [r]([k]G) = [k]([r]G) = O; each is checked against the curve equation.  That spares the model
    one Python ladder per filler point."""
    cv = PF.curve(cname)
    assert ladder(cv, PF.generator(cname), cv.r) is None
    chain = PF.affine_chain(cname, max(n, 1), 7, 11)[:n]
    assert all(cv.on_curve(pt) for pt in chain)
    rows = np.stack([cv.enc(pt) for pt in chain]) if n else np.zeros((0, 2 * cv.fw), dtype=np.uint64)
    rows.setflags(write=False)
    return rows


def bad_rows(cname, checks=3):
    """the planted rows whose status under `checks` is not 0, in planted order"""
    return np.stack([q.row for q in planted(cname) if model_status(cname, q.row, checks)])


def plant(cname, n, rows_to_plant, where=None):
    """n points: valid chain points everywhere, the given rows at `where` (default: PLANT_AT and n - 1, where they exist),
    cycling through them.  Returns (rows, the indices planted at)."""
    rows = _chain_rows(cname, n).copy()
    if where is None:
        where = PLANT_AT + (n - 1,)
    where = sorted(set(int(i) for i in where if 0 <= i < n)) if len(rows_to_plant) else []
    for k, i in enumerate(where):
        rows[i] = rows_to_plant[k % len(rows_to_plant)]
    return rows, where


def expected(cname, rows, where, checks, method=1):
    """(status bytes, [first_bad, n1, n2, n3]) of an array made by plant(): 0 for the chain points, the model at `where`"""
    st = np.zeros(len(rows), dtype=np.uint8)
    for i in where:
        st[i] = model_status(cname, rows[i], checks, method)
    bad = np.nonzero(st)[0]
    return st, [int(bad[0]) if bad.size else len(rows)] + [int((st == k).sum()) for k in (1, 2, 3)]
