"""The Python-integer model of the compressed-point codec (ark_hip_sw_decompress* / ark_hip_sw_compress*, csrc/pointcodec.cuh) and
its planted encodings, built on tests/pyref.py and the square roots of tests/check_fixtures.py: independent of the library.

    encode(cname, pt)                 the canonical E bytes of a point (None = identity)
    decode(cname, data, validate)     (status, point or None) of one encoding
    planted(cname)                    the planted encodings of a curve, by class (counts asserted)

The encodings (E bytes; "larger" = y > -y on canonical residues: integers for Fp; for Fp2 c1 first, then c0 --
ff/src/fields/models/quadratic_extension.rs:443-453 -- i.e. the deciding component is above (p - 1) / 2):
  arkworks form, BN254 G1 (32), BLS12-377 G1 (48), BLS12-377 G2 (96)      ec/src/models/short_weierstrass/mod.rs:125-193,
      serialize/src/flags.rs (serialization_flags.rs:55-80), ff/src/fields/models/fp/mod.rs:606-627, quadratic_extension.rs:719-727
    x little-endian (Fp2: c0 48 bytes without flag bits, then c1); bit 7 of the last byte = larger, bit 6 = infinity; both: refused.
    After the two bits are cleared every component must be < p -- also with the infinity bit, because x is read before the flags
    are looked at; with the infinity bit the result is the identity whatever x is.  y = 0: either value of bit 7 is accepted.
  zcash form, BLS12-381 G1 (48), G2 (96)             curves/bls12_381/src/curves/util.rs:16-36, 103-137, 174-209, g1.rs:97-147, g2.rs:124-140
    x big-endian (Fp2: c1 then c0); byte 0: bit 7 = compressed (must be set), bit 6 = infinity, bit 5 = larger.  Larger with
    infinity: refused.  Infinity: every other bit of the E bytes zero.  Every component < p after the three bits are cleared.
Status = the first failing stage, in this order: 1 flags refused / malformed, 2 a component is not a field element, 3 x^3 + b has
no square root, 4 [r]P != O (with validate only); a point with a non-zero status is the identity (0, 0).

The branch "x^3 + b has c1 = 0" of the Fp2 square root is not reached by a planted encoding (no such x is cheaply found on either
G2 curve); it is covered through the square-root hook (sqrt_inputs below) only.
"""
import collections
import functools

import numpy as np

import check_fixtures as CF
import point_fixtures as PF
import pyref as P

FORMS = {"BN254_G1": (32, False), "BLS12_381_G1": (48, True), "BLS12_377_G1": (48, False), "BLS12_377_G2": (96, False),
         "BLS12_381_G2": (96, True)}
Planted = collections.namedtuple("Planted", "name cls data")
# class -> status with validation (BN254 G1 has cofactor one: off_subgroup gives 0 there) / without
CLASS_STATUS = {"valid": (0, 0), "identity": (0, 0), "bad_flags": (1, 1), "inf_with_x": (0, 0), "not_reduced": (2, 2),
                "y_zero": (4, 0), "no_root": (3, 3), "off_subgroup": (4, 0)}
COUNTS = {
    "BN254_G1": {"valid": 6, "identity": 1, "bad_flags": 2, "inf_with_x": 2, "not_reduced": 4, "y_zero": 0, "no_root": 4, "off_subgroup": 6},
    "BLS12_381_G1": {"valid": 6, "identity": 1, "bad_flags": 6, "inf_with_x": 0, "not_reduced": 3, "y_zero": 0, "no_root": 4, "off_subgroup": 10},
    "BLS12_377_G1": {"valid": 6, "identity": 1, "bad_flags": 2, "inf_with_x": 2, "not_reduced": 5, "y_zero": 2, "no_root": 4, "off_subgroup": 8},
    "BLS12_377_G2": {"valid": 6, "identity": 1, "bad_flags": 2, "inf_with_x": 2, "not_reduced": 10, "y_zero": 0, "no_root": 4, "off_subgroup": 6},
    "BLS12_381_G2": {"valid": 6, "identity": 1, "bad_flags": 6, "inf_with_x": 0, "not_reduced": 4, "y_zero": 0, "no_root": 4, "off_subgroup": 8},
}


def size(cname):
    return FORMS[cname][0]


def _comps(cv, v):
    return [v] if cv.F.beta is None else [v[0], v[1]]


def is_larger(cv, y):
    """y > -y in the reference's order"""
    c = y if cv.F.beta is None else (y[1] if y[1] else y[0])
    return c > (cv.p - 1) // 2


def _pack(cname, comps, flags):
    """component integers (c0[, c1]) and the flag bits (already at their place in the top byte) -> E bytes"""
    e, zc = FORMS[cname]
    w = e // len(comps)
    if zc:
        out = bytearray(b"".join(c.to_bytes(w, "big") for c in reversed(comps)))
        out[0] |= flags
    else:
        out = bytearray(b"".join(c.to_bytes(w, "little") for c in comps))
        out[-1] |= flags
    return bytes(out)


def encode(cname, pt):
    cv = PF.curve(cname)
    zc = FORMS[cname][1]
    n = 1 if cv.F.beta is None else 2
    if pt is None:
        return _pack(cname, [0] * n, 0xC0 if zc else 0x40)
    flags = (0x80 if zc else 0) | ((0x20 if zc else 0x80) if is_larger(cv, pt[1]) else 0)
    return _pack(cname, _comps(cv, pt[0]), flags)


@functools.lru_cache(maxsize=None)
def _decode(cname, data):
    """(status without validation, point, in the subgroup?)"""
    cv = PF.curve(cname)
    e, zc = FORMS[cname]
    assert len(data) == e
    n = 1 if cv.F.beta is None else 2
    w = e // n
    raw = bytearray(data)
    if zc:
        top = raw[0]
        raw[0] &= 0x1F
        compressed, infinity, larger = bool(top & 0x80), bool(top & 0x40), bool(top & 0x20)
        comps = [int.from_bytes(raw[i * w:(i + 1) * w], "big") for i in range(n)][::-1]
        if not compressed or (infinity and (larger or any(raw))):
            return (1, None, True)
    else:
        top = raw[-1]
        raw[-1] &= 0x3F
        larger, infinity = bool(top & 0x80), bool(top & 0x40)
        comps = [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(n)]
        if larger and infinity:
            return (1, None, True)
    if any(c >= cv.p for c in comps):
        return (2, None, True)
    if infinity:
        return (0, None, True)
    F = cv.F
    x = comps[0] if n == 1 else (comps[0], comps[1])
    y = CF.sqrt_f(cv, F.add(F.mul(F.mul(x, x), x), cv.b))
    if y is None:
        return (3, None, True)
    if is_larger(cv, y) != larger:
        y = F.neg(y)
    pt = (x, y)
    assert cv.on_curve(pt)
    in_r = cname in CF.COFACTOR_ONE or CF.ladder(cv, pt, cv.r) is None
    return (0, pt, in_r)


def decode(cname, data, validate=True):
    st, pt, in_r = _decode(cname, bytes(data))
    if st == 0 and validate and not in_r:
        return (4, None)
    return (st, pt)


def status(cname, data, validate=True):
    return decode(cname, data, validate)[0]


def model(cname, rows, validate=True):
    """(points [n, 2 fe_words] u64, status bytes, [first_bad, n1, n2, n3, n4]) of an array of encodings"""
    cv = PF.curve(cname)
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, size(cname))
    dec = [decode(cname, r.tobytes(), validate) for r in rows]
    st = np.array([d[0] for d in dec], dtype=np.uint8)
    pts = np.stack([cv.enc(d[1]) for d in dec]) if len(dec) else np.zeros((0, 2 * cv.fw), dtype=np.uint64)
    return pts, st, summary(st)


def summary(st):
    bad = np.nonzero(st)[0]
    return [int(bad[0]) if bad.size else len(st)] + [int((st == k).sum()) for k in (1, 2, 3, 4)]


# ---- the planted encodings ---------------------------------------------------------------------------------------------------
def _no_root_xs(cv, rng, count):
    F = cv.F
    out = []
    while len(out) < count:
        rnd = lambda: int.from_bytes(rng.bytes(56), "little") % cv.p     # noqa: E731
        x = rnd() if F.beta is None else (rnd(), rnd())
        if CF.sqrt_f(cv, F.add(F.mul(F.mul(x, x), x), cv.b)) is None:
            out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def planted(cname):
    cv = PF.curve(cname)
    p = cv.p
    e, zc = FORMS[cname]
    ncomp = 1 if cv.F.beta is None else 2
    w = e // ncomp
    rng = np.random.default_rng(0xC0DEC + P.CURVE_ORDER.index(cname))
    out = []
    chain = PF.affine_chain(cname, 6)
    flags_seen = set()
    for i, pt in enumerate(chain):
        out.append(Planted("chain%d" % i, "valid", encode(cname, pt)))
        flags_seen.add(is_larger(cv, pt[1]))
    assert flags_seen == {False, True}, "the chain no longer has both values of the larger bit"
    out.append(Planted("identity", "identity", encode(cname, None)))
    x1 = _comps(cv, chain[1][0])
    if not zc:
        out.append(Planted("both_flags", "bad_flags", _pack(cname, x1, 0xC0)))
        out.append(Planted("both_flags_zero_x", "bad_flags", _pack(cname, [0] * ncomp, 0xC0)))
        out.append(Planted("inf_with_x", "inf_with_x", _pack(cname, x1, 0x40)))
        out.append(Planted("inf_with_pm1", "inf_with_x", _pack(cname, [p - 1] * ncomp, 0x40)))
        for k in range(ncomp):                     # infinity with x >= p: x is read first
            c = list(x1)
            c[k] = p + k
            out.append(Planted("inf_x_ge_p_%d" % k, "not_reduced", _pack(cname, c, 0x40)))
    else:
        out.append(Planted("no_compressed_bit", "bad_flags", _pack(cname, x1, 0x20 if is_larger(cv, chain[1][1]) else 0)))
        out.append(Planted("no_compressed_bit_inf", "bad_flags", _pack(cname, [0] * ncomp, 0x40)))
        out.append(Planted("larger_with_infinity", "bad_flags", _pack(cname, [0] * ncomp, 0xE0)))
        first = bytearray(_pack(cname, [0] * ncomp, 0xC0))
        first[0] |= 0x01
        last = bytearray(_pack(cname, [0] * ncomp, 0xC0))
        last[-1] |= 0x01
        mid = bytearray(_pack(cname, [0] * ncomp, 0xC0))
        mid[e // 2] |= 0x80
        out.append(Planted("inf_first_byte_bit", "bad_flags", bytes(first)))
        out.append(Planted("inf_last_byte_bit", "bad_flags", bytes(last)))
        out.append(Planted("inf_middle_bit", "bad_flags", bytes(mid)))
    # not a field element: p, p + 1, all ones under the flag mask -- each component separately
    keep = 5 if zc else 6                          # bits of the top byte that belong to the number
    for k in range(ncomp):
        for name, v in (("p", p), ("p_plus_1", p + 1), ("ones", (1 << (8 * w)) - 1)):
            if ncomp == 2 and name == "p_plus_1":
                continue
            c = list(x1)
            c[k] = v
            flagged = (k == ncomp - 1)             # the component whose top byte carries the flags
            if flagged:
                c[k] &= (1 << (8 * (w - 1) + keep)) - 1
            data = bytearray(_pack(cname, c, 0))
            if zc:
                data[0] |= 0x80
            out.append(Planted("%s_%d" % (name, k), "not_reduced", bytes(data)))
    if cname in ("BLS12_377_G1", "BLS12_377_G2"):  # junk in bits 377 .. 381 of a component
        for k in range(ncomp):
            c = list(x1)
            c[k] |= 1 << (377 + 2 * k)
            out.append(Planted("junk_bit_%d" % k, "not_reduced", _pack(cname, c, 0)))
        if ncomp == 2:                             # bits 382 / 383 of c0 are no flags
            for bit in (382, 383):
                c = list(x1)
                c[0] |= 1 << bit
                out.append(Planted("c0_bit_%d" % bit, "not_reduced", _pack(cname, c, 0)))
    if cname == "BLS12_377_G1":                    # y = 0: the point (p - 1, 0) of order 2, either flag
        assert cv.on_curve((p - 1, 0))
        out.append(Planted("y_zero", "y_zero", _pack(cname, [p - 1], 0)))
        out.append(Planted("y_zero_larger", "y_zero", _pack(cname, [p - 1], 0x80)))
    for i, x in enumerate(_no_root_xs(cv, rng, 4)):
        fl = ((0x80 | (0x20 if i % 2 else 0)) if zc else (0x80 if i % 2 else 0))
        out.append(Planted("no_root%d" % i, "no_root", _pack(cname, _comps(cv, x), fl)))
    for q in CF.planted(cname):
        if q.cls in ("off_subgroup", "small_order"):
            pt = cv.dec(q.row)
            if pt[1] == cv.F.zero():
                continue                           # (p - 1, 0): the y_zero class
            out.append(Planted(q.name, "off_subgroup", encode(cname, pt)))
    counts = collections.Counter(q.cls for q in out)
    assert dict((k, counts.get(k, 0)) for k in COUNTS[cname]) == COUNTS[cname], (cname, dict(counts))
    assert len(set(q.data for q in out)) == len(out)
    for q in out:
        want_v, want_n = CLASS_STATUS[q.cls]
        if cname in CF.COFACTOR_ONE and q.cls == "off_subgroup":
            want_v = 0
        assert status(cname, q.data, True) == want_v and status(cname, q.data, False) == want_n, (cname, q.name)
    return tuple(out)


def planted_rows(cname):
    return np.stack([np.frombuffer(q.data, dtype=np.uint8) for q in planted(cname)])


def bad_rows(cname, validate=True):
    return np.stack([np.frombuffer(q.data, dtype=np.uint8) for q in planted(cname) if status(cname, q.data, validate)])


@functools.lru_cache(maxsize=None)
def _chain(cname, n):
    """(encodings, points) of the n valid points [7 + 11 i] G of check_fixtures: they decode to themselves with status 0 by
    construction ([r]G = O is asserted there; encode() is the canonical form)"""
    cv = PF.curve(cname)
    pts = CF._chain_rows(cname, n)
    enc = np.stack([np.frombuffer(encode(cname, cv.dec(r)), dtype=np.uint8) for r in pts]) if n else np.zeros((0, size(cname)), dtype=np.uint8)
    enc.setflags(write=False)
    return enc, pts


def plant(cname, n, rows_to_plant, where=None):
    """n encodings: valid chain points everywhere, the given rows at `where` (default: check_fixtures.PLANT_AT and n - 1), cycling.
    Returns (encodings, the indices planted at)."""
    rows = _chain(cname, n)[0].copy()
    if where is None:
        where = CF.PLANT_AT + (n - 1,)
    where = sorted(set(int(i) for i in where if 0 <= i < n)) if len(rows_to_plant) else []
    for k, i in enumerate(where):
        rows[i] = rows_to_plant[k % len(rows_to_plant)]
    return rows, where


def expected(cname, rows, where, validate=True):
    """(points, status bytes, [first_bad, n1..n4]) of an array made by plant(): the chain points themselves, the model at `where`"""
    cv = PF.curve(cname)
    pts = _chain(cname, len(rows))[1].copy()
    st = np.zeros(len(rows), dtype=np.uint8)
    for i in where:
        s, pt = decode(cname, rows[i].tobytes(), validate)
        st[i] = s
        pts[i] = cv.enc(pt)
    return pts, st, summary(st)


# ---- inputs of the square-root hook ----------------------------------------------------------------------------------------------
def smaller_root(cv, a):
    """(the root r of a with r <= -r, 1) or (zero, 0)"""
    r = CF.sqrt_f(cv, a)
    if r is None:
        return cv.F.zero(), 0
    assert cv.F.mul(r, r) == a
    return (cv.F.neg(r) if is_larger(cv, r) else r), 1


def codec_root_of_unity():
    """the 2^46-th root of unity of BLS12-377 Fq from the generated header (Montgomery form there)"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "algebra_amd", "csrc", "codec_consts.hpp")).read()
    body = txt[txt.index("struct SQRT_BLS12_377_FQ"):]
    limbs = re.search(r"ROOT\[12\] = \{([^}]*)\}", body).group(1)
    v = 0
    for i, wd in enumerate(limbs.split(",")):
        v |= int(wd.strip().rstrip("u"), 16) << (32 * i)
    p = P.MODULI["BLS12_377_FQ"][0]
    return v * pow(P.R_of(p), -1, p) % p


@functools.lru_cache(maxsize=None)
def sqrt_inputs(cname):
    """[(name, element)]: 0, 1, p - 1, known non-residues, squares of random elements; over BLS12-377 Fq one input for each order 2^k
    of a^((p-1)/2^46), k = 0 .. 46 (k = 46: a non-residue); over Fp2 the three c1 = 0 cases, a non-residue norm and both signs of
    the delta branch"""
    cv = PF.curve(cname)
    p, F = cv.p, cv.F
    rng = np.random.default_rng(0x5017 + P.CURVE_ORDER.index(cname))
    rnd = lambda: 1 + int.from_bytes(rng.bytes(56), "little") % (p - 1)     # noqa: E731
    g = dict((v[0], v[1]) for v in P.MODULI.values())[p]                       # the multiplicative generator: a non-residue
    assert pow(g, (p - 1) // 2, p) == p - 1
    out = []
    if F.beta is None:
        out += [("zero", 0), ("one", 1), ("p_minus_1", p - 1), ("generator", g), ("generator_cubed", pow(g, 3, p))]
        for i in range(6):
            u = rnd()
            out.append(("square%d" % i, u * u % p))
            out.append(("nonresidue%d" % i, u * u * g % p))
        if cname == "BLS12_377_G1":
            s, q = P.two_adicity(p)
            assert s == 46
            omega = codec_root_of_unity()
            assert pow(omega, 1 << 45, p) == p - 1
            for k in range(s + 1):
                u = rnd()
                a = pow(omega, 1 << (s - k), p) * pow(u, 1 << s, p) % p if k else pow(u, 1 << s, p)
                t = pow(a, q, p)
                assert pow(t, 1 << k, p) == 1 and (k == 0 or pow(t, 1 << (k - 1), p) != 1)     # a^q has order exactly 2^k
                out.append(("order_2^%d" % k, a))
    else:
        beta = F.beta % p
        nonres = g if pow(g, (p - 1) // 2, p) == p - 1 else None
        out += [("zero", (0, 0)), ("one", (1, 0)), ("minus_one", (p - 1, 0)), ("u", (0, 1))]
        for i in range(3):
            u = rnd()
            out.append(("c1_zero_residue%d" % i, (u * u % p, 0)))               # root (u, 0)
            out.append(("c1_zero_nonresidue%d" % i, (u * u * nonres % p, 0)))   # root (0, s) with beta s^2 = c0
            out.append(("c1_zero_beta_square%d" % i, (beta * u * u % p, 0)))    # (u u)^2 exactly
        plus = minus = nonorm = 0
        while min(plus, minus) < 3 or nonorm < 3:
            a = (rnd(), rnd())
            norm = (a[0] * a[0] - beta * a[1] * a[1]) % p
            alpha = CF.sqrt_fp(norm, p)
            if alpha is None:
                if nonorm < 3:
                    out.append(("norm_nonresidue%d" % nonorm, a))
                nonorm += 1
                continue
            # which sign of alpha makes (c0 + alpha) / 2 a square depends on the root the implementation takes: give both
            for al in (alpha, p - alpha):
                d = (a[0] + al) * pow(2, -1, p) % p
                if CF.sqrt_fp(d, p) is not None:
                    if al == alpha and plus < 3:
                        out.append(("delta_first%d" % plus, a))
                        plus += 1
                    elif al != alpha and minus < 3:
                        out.append(("delta_second%d" % minus, a))
                        minus += 1
        for i in range(3):
            u = (rnd(), rnd())
            out.append(("square%d" % i, F.mul(u, u)))
    return tuple(out)
