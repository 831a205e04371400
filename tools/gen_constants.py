#!/usr/bin/env python3
"""Derive every field / curve constant used by the oracle and by the HIP kernels from the
decimal literals the reference declares, and emit them as C headers.

Sources (reference file:line, all under /root/reference/curves):
  bls12_381/src/fields/fq.rs:4-5, fr.rs:4-5      bn254/src/fields/fq.rs:4-5, fr.rs:4-5
  bls12_377/src/fields/fq.rs:4-5, fr.rs:24-25    bls12_377/src/fields/fq2.rs:12-13 (NONRESIDUE=-5)
  bls12_381/src/curves/g1.rs:43-46,199-205       bls12_381/src/curves/g2.rs:58-59,229-241
  bn254/src/curves/g1.rs:21,29-32,92-96          bls12_377/src/curves/g1.rs:42-43,217-223
  bls12_377/src/curves/g2.rs:47-58,135-152
Derivations follow ff/src/fields/models/fp/montgomery_backend.rs:21-60 (R, R2, INV) and
ff-macros/src/montgomery/mod.rs:40-52 (TWO_ADIC_ROOT_OF_UNITY = generator^((p-1)/2^s)).

Outputs:  oracle/constants.h  (64-bit limbs, C)      algebra_amd/csrc/params.hpp (32-bit limbs, C++)
          algebra_amd/csrc/curve_consts.hpp (subgroup generators, host side; the signed 30-bit constants of csrc/fp30s.cuh)
          algebra_amd/csrc/check_consts.hpp (what the base-set check needs: COEFF_B, the subgroup order r and, for
          BLS12-381 G1, the endomorphism constant beta and x^2 -- csrc/pointcheck.cuh)
          algebra_amd/csrc/codec_consts.hpp (what the compressed-point codec needs: square-root exponents, (p-1)/2,
          1/2, the 2^46-th root of unity of BLS12-377 Fq, 1/beta of the two Fp2 -- csrc/pointcodec.cuh)
This script is the single place the decimal literals live; tests/test_constants.py re-derives
them independently and checks both headers.
"""
import os, sys

FIELDS = [
    # name, modulus, multiplicative generator
    ("BN254_FQ", 21888242871839275222246405745257275088696311157297823662689037894645226208583, 3),
    ("BN254_FR", 21888242871839275222246405745257275088548364400416034343698204186575808495617, 5),
    ("BLS12_381_FQ", 4002409555221667393417789825735904156556882819939007885332058136124031650490837864442687629129015664037894272559787, 2),
    ("BLS12_381_FR", 52435875175126190479447740508185965837690552500527637822603658699938581184513, 7),
    ("BLS12_377_FQ", 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177, 15),
    ("BLS12_377_FR", 8444461749428370424248824938781546531375899335154063827935233455917409239041, 22),
]

# curve: name, base field, scalar field, ext degree, beta (Fp2 nonresidue, as small signed int), b coefficient (tuple), generator (x, y) tuples
CURVES = [
    ("BN254_G1", "BN254_FQ", "BN254_FR", 1, 0, (3,), ((1,), (2,))),
    ("BLS12_381_G1", "BLS12_381_FQ", "BLS12_381_FR", 1, 0, (4,),
     ((3685416753713387016781088315183077757961620795782546409894578378688607592378376318836054947676345821548104185464507,),
      (1339506544944476473020471379941921221584933875938349620426543736416511423956333506472724655353366534992391756441569,))),
    ("BLS12_377_G1", "BLS12_377_FQ", "BLS12_377_FR", 1, 0, (1,),
     ((81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695,),
      (241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030,))),
    ("BLS12_377_G2", "BLS12_377_FQ", "BLS12_377_FR", 2, -5,
     (0, 155198655607781456406391640216936120121836107652948796323930557600032281009004493664981332883744016074664192874906),
     ((233578398248691099356572568220835526895379068987715365179118596935057653620464273615301663571204657964920925606294,
       140913150380207355837477652521042157274541796891053068589147167627541651775299824604154852141315666357241556069118),
      (63160294768292073209381361943935198908131692476676907196754037919244929611450776219210369229519898517858833747423,
       149157405641012693445398062341192467754805999074082136895788947234480009303640899064710353187729182149407503257491))),
    ("BLS12_381_G2", "BLS12_381_FQ", "BLS12_381_FR", 2, -1, (4, 4),
     ((352701069587466618187139116011060144890029952792775240219908644239793785735715026873347600343865175952761926303160,
       3059144344244213709971259814753781636986470325476647558659373206291635324768958432433509563104347017837885763365758),
      (1985150602287291935568054521177171638300868978215655730859378665066344726373823718423869104263333984641494340347905,
       927553665492332455747201965776037880757740193453592970025027978793976877002675564980949289727957565575433344219582))),
]


def field_consts(p, g):
    n64 = (p.bit_length() + 63) // 64
    R = (1 << (64 * n64)) % p
    R2 = R * R % p
    inv64 = (-pow(p, -1, 1 << 64)) % (1 << 64)
    s = 0
    t = p - 1
    while t % 2 == 0:
        t //= 2
        s += 1
    root = pow(g, t, p)  # 2^s-th primitive root of unity
    return dict(n64=n64, bits=p.bit_length(), R=R, R2=R2, inv64=inv64, two_adicity=s, root=root, gen=g)


def limbs(x, n, w):
    return [(x >> (w * i)) & ((1 << w) - 1) for i in range(n)]


def signed_digits(x, n, w):
    """x >= 0 as n digits of w bits in [-2^(w-1), 2^(w-1)); the top digit takes what is left"""
    out = []
    for _ in range(n - 1):
        d = x & ((1 << w) - 1)
        if d >= 1 << (w - 1):
            d -= 1 << w
        out.append(d)
        x = (x - d) >> w
    out.append(x)
    return out


# fields that get the signed 30-bit form of fp30s.cuh (S30_<field> in curve_consts.hpp), and the multiple of p that makes
# an accumulator coordinate (|v| < 2.2 p, ec30s.cuh) positive on its way out
S30_FIELDS = ["BLS12_381_FQ"]
S30_OUT_K = 4


def c_arr(x, n, w):
    fmt = "0x%016xULL" if w == 64 else ("0x%08xu" if w == 32 else "0x%07xu")
    return "{" + ", ".join(fmt % v for v in limbs(x, n, w)) + "}"


# ---- the base-set check (csrc/pointcheck.cuh) ----
BLS12_381_X = -0xd201000000010000          # curves/bls12_381/src/curves/mod.rs: X = 0xd201000000010000, X_IS_NEGATIVE
BN254_U = 4965661367192848881              # curves/bn254/src/curves/mod.rs: X


def _aff_add(P, Q, p):
    """textbook affine addition on y^2 = x^3 + b over Fp (None: the identity)"""
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return (x3, (lam * (x1 - x3) - y1) % p)


def _aff_mul(P, k, p):
    acc = None
    for bit in bin(k)[2:]:
        acc = _aff_add(acc, acc, p)
        if bit == "1":
            acc = _aff_add(acc, P, p)
    return acc


def endo_beta_bls12_381():
    """The cube root of unity beta in Fq with (beta x, y) = -[x^2](x, y) on the subgroup of BLS12-381 G1 (Scott, eprint
    2021/1130 section 6; curves/bls12_381/src/curves/g1.rs:69-85), derived and ASSERTED on the generator."""
    p = dict((n, q) for n, q, _ in FIELDS)["BLS12_381_FQ"]
    r = dict((n, q) for n, q, _ in FIELDS)["BLS12_381_FR"]
    x = BLS12_381_X
    assert r == x ** 4 - x ** 2 + 1
    G = [(c[6][0][0], c[6][1][0]) for c in CURVES if c[0] == "BLS12_381_G1"][0]
    assert (G[1] * G[1] - G[0] ** 3 - 4) % p == 0 and _aff_mul(G, r, p) is None
    w = pow(2, (p - 1) // 3, p)
    assert w != 1 and pow(w, 3, p) == 1
    T = _aff_mul(G, x * x, p)
    want = (T[0], (-T[1]) % p)
    hits = [b for b in (w, w * w % p) if (b * G[0] % p, G[1]) == want]
    assert len(hits) == 1, "exactly one non-trivial cube root of unity satisfies phi(G) = -[x^2]G"
    return hits[0], x * x


def check_consts_header(fc):
    fp = dict((n, q) for n, q, _ in FIELDS)
    beta, x2 = endo_beta_bls12_381()
    assert x2.bit_length() == 128
    # BN254 G1 has cofactor one: #E(Fq) = q + 1 - t with t = 6u^2 + 1 is r itself (curves/bn254/src/curves/g1.rs:59)
    assert fp["BN254_FQ"] + 1 - (6 * BN254_U ** 2 + 1) == fp["BN254_FR"]
    h = []
    h.append("// GENERATED by tools/gen_constants.py -- do not edit.")
    h.append("// Per curve, what the base-set check (pointcheck.cuh) needs: COEFF_B (Montgomery form, one row per Fp component), the")
    h.append("// subgroup order r as a plain integer (32-bit limbs) and whether the cofactor is one; for BLS12-381 G1 also x^2 and the")
    h.append("// cube root of unity beta with (beta x, y) = -[x^2](x, y) on the subgroup (asserted on the generator at generation time).")
    h.append("#pragma once\n#include <stdint.h>\nnamespace arkhip {")
    for name, bf, sf, deg, _, b, _ in CURVES:
        f = fc[bf]
        p, n = f["p"], f["n64"] * 2
        r = fp[sf]
        endo = name == "BLS12_381_G1"
        h.append("struct CHECK_%s {" % name)
        h.append("  static constexpr bool COFACTOR_ONE = %s;" % ("true" if name == "BN254_G1" else "false"))
        h.append("  static constexpr int R_BITS = %d;           // popcount %d" % (r.bit_length(), bin(r).count("1")))
        h.append("  static constexpr uint32_t R[8] = %s;" % c_arr(r, 8, 32))
        h.append("  static constexpr uint32_t B[%d][%d] = {%s};" % (deg, n, ", ".join(c_arr(c * f["R"] % p, n, 32) for c in b)))
        h.append("  static constexpr bool HAS_ENDO = %s;" % ("true" if endo else "false"))
        if endo:
            h.append("  static constexpr int X2_BITS = %d;          // popcount %d" % (x2.bit_length(), bin(x2).count("1")))
            h.append("  static constexpr uint32_t X2[8] = %s;" % c_arr(x2, 8, 32))
            h.append("  static constexpr uint32_t ENDO_BETA[%d] = %s;" % (n, c_arr(beta * f["R"] % p, n, 32)))
        h.append("};")
    h.append("} // namespace arkhip")
    return "\n".join(h) + "\n"

# ---- the compressed-point codec (csrc/pointcodec.cuh) ----
# curve -> (bytes per point, zcash form?)   arkworks: short_weierstrass/mod.rs:125-193; zcash: bls12_381/src/curves/util.rs
CODEC_FORMS = {"BN254_G1": (32, False), "BLS12_381_G1": (48, True), "BLS12_377_G1": (48, False), "BLS12_377_G2": (96, False),
               "BLS12_381_G2": (96, True)}


def sqrt_plan(p, g):
    """How csrc/pointcodec.cuh takes a square root in Fp, and what it costs in Fp products.
    p = 3 mod 4: w = a^((p-3)/4), root = w a, accepted iff root^2 = a (then 1/root = w).
    otherwise (BLS12-377 Fq, p - 1 = 2^s q): Tonelli-Shanks with fixed trip counts (RFC 9380 appendix I.4):
    z = a^((q-1)/2), then s - 1 rounds of (i - 2 squarings, 3 products), i = s .. 2, accepted iff root^2 = a."""
    if p % 4 == 3:
        e = (p - 3) // 4
        count = (e.bit_length() - 1) + (bin(e).count("1") - 1) + 2
        return dict(p3mod4=True, e=e, s=1, products=count)
    s, q = 0, p - 1
    while q % 2 == 0:
        q //= 2
        s += 1
    e = (q - 1) // 2
    count = (e.bit_length() - 1) + (bin(e).count("1") - 1) + 3 + sum(i - 2 for i in range(2, s + 1)) + 3 * (s - 1) + 1
    root = pow(g, q, p)
    assert pow(root, 1 << (s - 1), p) == p - 1
    return dict(p3mod4=False, e=e, s=s, products=count, root=root)


def codec_consts_header(fc):
    h = []
    h.append("// GENERATED by tools/gen_constants.py -- do not edit.")
    h.append("// What the compressed-point codec (pointcodec.cuh) needs.  Per base field: the square-root exponent E as a plain integer")
    h.append("// ((p-3)/4 where p = 3 mod 4; (q-1)/2 with p - 1 = 2^S q otherwise), (p-1)/2 as a plain integer (y > -y iff the deciding")
    h.append("// component is above it), p - 2 as a plain integer (the inversion exponent), 1/2 and the 2^S-th root of unity in Montgomery")
    h.append("// form (-1 where S = 1), and the Fp products of one square root.")
    h.append("// Per curve: bytes per point, which form, and for BLS12-377 G2 1/beta of the quadratic extension (Montgomery form).")
    h.append("#pragma once\n#include <stdint.h>\nnamespace arkhip {")
    for name in ("BN254_FQ", "BLS12_381_FQ", "BLS12_377_FQ"):
        f = fc[name]
        p, n = f["p"], f["n64"] * 2
        plan = sqrt_plan(p, f["gen"])
        m = lambda x: x * f["R"] % p
        h.append("struct SQRT_%s {" % name)
        h.append("  static constexpr bool P3MOD4 = %s;" % ("true" if plan["p3mod4"] else "false"))
        h.append("  static constexpr int S = %d;                // two-adicity used by the root (1: none needed)" % plan["s"])
        h.append("  static constexpr int E_BITS = %d;           // popcount %d" % (plan["e"].bit_length(), bin(plan["e"]).count("1")))
        h.append("  static constexpr int PRODUCTS = %d;        // Fp products of one square root, acceptance test included" % plan["products"])
        h.append("  static constexpr uint32_t E[%d] = %s;" % (n, c_arr(plan["e"], n, 32)))
        h.append("  static constexpr uint32_t HALF_P[%d] = %s;" % (n, c_arr((p - 1) // 2, n, 32)))
        h.append("  static constexpr uint32_t PM2[%d] = %s;" % (n, c_arr(p - 2, n, 32)))
        h.append("  static constexpr uint32_t TWO_INV[%d] = %s;" % (n, c_arr(m(pow(2, -1, p)), n, 32)))
        h.append("  static constexpr uint32_t ROOT[%d] = %s;" % (n, c_arr(m(plan.get("root", p - 1)), n, 32)))
        h.append("};")
    for name, bf, sf, deg, beta, b, _ in CURVES:
        f = fc[bf]
        p, n = f["p"], f["n64"] * 2
        e, zc = CODEC_FORMS[name]
        assert e == deg * f["n64"] * 8 and 8 * f["n64"] * 8 - f["bits"] >= (3 if zc else 2)
        h.append("struct CODEC_%s {" % name)
        h.append("  static constexpr int E = %d;" % e)
        h.append("  static constexpr bool ZCASH = %s;" % ("true" if zc else "false"))
        if deg == 2:
            assert pow(beta % p, (p - 1) // 2, p) == p - 1
        if deg == 2 and not (p % 4 == 3 and beta == -1):     # beta = -1 with p = 3 mod 4: the root of -a comes for free
            h.append("  static constexpr uint32_t INV_BETA[%d] = %s;" % (n, c_arr(pow(beta, -1, p) * f["R"] % p, n, 32)))
        h.append("};")
    h.append("} // namespace arkhip")
    return "\n".join(h) + "\n"


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fc = {name: dict(p=p, **field_consts(p, g)) for name, p, g in FIELDS}

    # ---------------- oracle/constants.h ----------------
    o = []
    o.append("/* GENERATED by tools/gen_constants.py -- do not edit. TEST INFRASTRUCTURE (oracle). */")
    o.append("#ifndef ARK_ORACLE_CONSTANTS_H\n#define ARK_ORACLE_CONSTANTS_H\n#include <stdint.h>")
    o.append("typedef struct { const char* name; int n; int bits; int two_adicity; uint64_t inv;")
    o.append("  uint64_t p[6], r[6], r2[6], gen[6], root[6]; } ark_field_consts;")
    o.append("static const ark_field_consts ARK_FIELDS[%d] = {" % len(FIELDS))
    for name, p, g in FIELDS:
        f = fc[name]
        n = f["n64"]
        m = lambda x: x * f["R"] % p
        o.append('  {"%s", %d, %d, %d, 0x%016xULL,' % (name, n, f["bits"], f["two_adicity"], f["inv64"]))
        o.append("   %s, %s, %s,\n   %s, %s}," % (c_arr(p, 6, 64), c_arr(f["R"], 6, 64), c_arr(f["R2"], 6, 64),
                                                   c_arr(m(g), 6, 64), c_arr(m(f["root"]), 6, 64)))
    o.append("};")
    o.append("enum { " + ", ".join("ARK_F_%s=%d" % (n, i) for i, (n, _, _) in enumerate(FIELDS)) + " };")
    o.append("typedef struct { const char* name; int base_field, scalar_field, ext_degree, beta_abs;")
    o.append("  uint64_t b[12], gx[12], gy[12]; } ark_curve_consts; /* Montgomery form, c0 then c1 */")
    o.append("static const ark_curve_consts ARK_CURVES[%d] = {" % len(CURVES))
    fidx = {n: i for i, (n, _, _) in enumerate(FIELDS)}
    for name, bf, sf, deg, beta, b, (gx, gy) in CURVES:
        f = fc[bf]
        p = f["p"]
        n = f["n64"]
        def ext(t):
            out = []
            for c in t:
                out += limbs(c * f["R"] % p, n, 64)
            out += [0] * (12 - len(out))
            return "{" + ", ".join("0x%016xULL" % v for v in out) + "}"
        o.append('  {"%s", %d, %d, %d, %d,\n   %s,\n   %s,\n   %s},' % (name, fidx[bf], fidx[sf], deg, abs(beta), ext(b), ext(gx), ext(gy)))
    o.append("};")
    o.append("enum { " + ", ".join("ARK_C_%s=%d" % (c[0], i) for i, c in enumerate(CURVES)) + " };")
    o.append("#endif")
    open(os.path.join(root, "oracle", "constants.h"), "w").write("\n".join(o) + "\n")

    # ---------------- algebra_amd/csrc/params.hpp ----------------
    d = []
    d.append("// GENERATED by tools/gen_constants.py -- do not edit.")
    d.append("// Field parameters as 32-bit little-endian limbs for the gfx950 kernels.")
    d.append("// (memory layout of an element is identical to the reference's [u64; N] little-endian limbs,")
    d.append("//  ff/src/biginteger/mod.rs:34, so a u64[N] buffer is read as u32[2N] with no conversion)")
    d.append("#pragma once\n#include <stdint.h>\nnamespace arkhip {")
    for i, (name, p, g) in enumerate(FIELDS):
        f = fc[name]
        n = f["n64"] * 2
        m = lambda x: x * f["R"] % p
        inv32 = f["inv64"] & 0xffffffff
        d.append("struct %s {" % name)
        d.append("  static constexpr int ID = %d;" % i)
        d.append("  static constexpr int N = %d;           // 32-bit limbs" % n)
        d.append("  static constexpr int BITS = %d;" % f["bits"])
        d.append("  static constexpr int TWO_ADICITY = %d;" % f["two_adicity"])
        d.append("  static constexpr uint32_t INV = 0x%08xu;   // -p^-1 mod 2^32" % inv32)
        for nm, val in (("P", p), ("R", f["R"]), ("R2", f["R2"]), ("GEN", m(g)), ("ROOT", m(f["root"]))):
            d.append("  static constexpr uint32_t %s[%d] = %s;" % (nm, n, c_arr(val, n, 32)))
        # carry-free form (fp28.cuh): LZ_L limbs of LZ_W bits, Montgomery radix 2^(LZ_W*LZ_L); a whole column of a
        # product-scanning multiplication (2 LZ_L products of 2 LZ_W bits) must fit 64 bits: 14 x 28 bits for the
        # 384-bit fields, 9 x 29 bits for the 254/255-bit ones.  k*p tables for borrow-free subtraction / zero tests
        lw = 28 if n > 8 else 29
        lz = 14 if n > 8 else 9
        assert lw * lz >= 32 * n and 2 * lz * (1 << (2 * lw)) < (1 << 64)
        d.append("  static constexpr int LZ_W = %d;           // bits per limb of the carry-free form" % lw)
        d.append("  static constexpr int LZ_L = %d;           // its limbs" % lz)
        d.append("  static constexpr uint32_t LZ_INV = 0x%07xu;   // -p^-1 mod 2^LZ_W" % (f["inv64"] & ((1 << lw) - 1)))
        d.append("  static constexpr uint32_t LZ_CIN[%d] = %s;   // 2^(LZ_W*LZ_L) mod p  (raw residue, 32-bit limbs)" % (n, c_arr(pow(2, lw * lz, p), n, 32)))
        rows = ", ".join(c_arr(k * p, lz, lw) for k in range(9))
        d.append("  static constexpr uint32_t LZ_KP[9][%d] = {%s};   // k*p, k = 0..8, LZ_W-bit limbs" % (lz, rows))
        d.append("  static constexpr int LZ_RP = %d;          // floor(2^(LZ_W*LZ_L) / p): a product of A p and B p comes out below (A B / LZ_RP + 1) p" % ((1 << (lw * lz)) // p))
        d.append("};")
    d.append("} // namespace arkhip")
    open(os.path.join(root, "algebra_amd", "csrc", "params.hpp"), "w").write("\n".join(d) + "\n")

    # ---------------- algebra_amd/csrc/curve_consts.hpp (host-side: subgroup generators) ----------------
    h = []
    h.append("// GENERATED by tools/gen_constants.py -- do not edit.")
    h.append("// Prime-order subgroup generators (affine x|y, Montgomery form, 64-bit limbs, Fp2 as c0|c1) from")
    h.append("// curves/bn254/src/curves/g1.rs:92-96, bls12_381 g1.rs:199-205 / g2.rs:229-241, bls12_377 g1.rs:217-223 / g2.rs:135-152.")
    h.append("#pragma once\n#include <stdint.h>\nnamespace arkhip {")
    for name, bf, sf, deg, beta, b, (gx, gy) in CURVES:
        f = fc[bf]
        p = f["p"]
        n = f["n64"]
        words = []
        for t in (gx, gy):
            for c in t:
                words += limbs(c * f["R"] % p, n, 64)
        h.append("static const uint64_t GEN_%s[%d] = {%s};" % (name, len(words), ", ".join("0x%016xULL" % v for v in words)))
    # signed 30-bit form of the accumulate kernel (fp30s.cuh): 13 digits in [-2^29, 2^29), Montgomery radix 2^390
    for name in S30_FIELDS:
        p = fc[name]["p"]
        sw, sl = 30, 13
        assert sw * sl >= 32 * fc[name]["n64"] * 2 and p >> (sw * (sl - 1)) < 1 << (sw - 1)
        sd = lambda x: "{" + ", ".join("%d" % v for v in signed_digits(x, sl, sw)) + "}"
        h.append("struct S30_%s {" % name)
        h.append("  static constexpr int W = %d, L = %d;" % (sw, sl))
        h.append("  static constexpr int32_t P[%d] = %s;   // p, signed digits" % (sl, sd(p)))
        h.append("  static constexpr uint32_t INV = 0x%08xu;   // -p^-1 mod 2^W" % (fc[name]["inv64"] & ((1 << sw) - 1)))
        h.append("  static constexpr int32_t ONE[%d] = %s;   // 2^(W L) mod p, signed digits: the residue 1" % (sl, sd(pow(2, sw * sl, p))))
        h.append("  static constexpr int OUT_K = %d;           // OUT_K p is added to a signed residue on its way to the canonical form" % S30_OUT_K)
        h.append("  static constexpr int32_t OUT_KP[%d] = %s;   // OUT_K p, signed digits" % (sl, sd(S30_OUT_K * p)))
        h.append("};")
    h.append("} // namespace arkhip")
    open(os.path.join(root, "algebra_amd", "csrc", "curve_consts.hpp"), "w").write("\n".join(h) + "\n")
    open(os.path.join(root, "algebra_amd", "csrc", "check_consts.hpp"), "w").write(check_consts_header(fc))
    open(os.path.join(root, "algebra_amd", "csrc", "codec_consts.hpp"), "w").write(codec_consts_header(fc))
    print("wrote oracle/constants.h, algebra_amd/csrc/params.hpp, curve_consts.hpp, check_consts.hpp and codec_consts.hpp")


if __name__ == "__main__":
    main()
