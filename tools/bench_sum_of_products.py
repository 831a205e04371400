"""Times the gate expression on device vectors (ark_hip_fr_sum_of_products_device) over BLS12-381 Fr at
n = 2^20, 2^22, 2^24 rows on periodic random columns:

  nine_term   q_M a b + q_L a + q_R b + q_O c + q_C + alpha (z N - z(wX) D) + alpha^2 L_1 (z - 1): nine terms over twelve
              columns, rotation 4 on z (a coset of blow-up 4), in ONE call -- against the composed route a caller had before
              the entry: eight ark_hip_fr_mul_device, two ark_hip_memcpy_d2d for the rotated copy of z, one
              ark_hip_fr_lincomb_device over eight tables and one ark_hip_fr_axpy_device, with eight temporaries;
  mul         the single product a b in one call -- against ark_hip_fr_mul_device, the streaming Montgomery-product rate the
              chip has demonstrated;
  pow8        a^8 (one read, one write, seven products per row): the product rate of this kernel when memory is out of the way;
  rotate      the rotated copy -- against the two ark_hip_memcpy_d2d that did it before;

and, as the neighbouring profiles do, one device copy and the d2h + h2d round trip of one vector through pinned memory.  The
composed results are compared bitwise with the new ones over the whole vector before anything is timed, and sampled rows with
Python big integers.  Next to the times: the vector passes (vectors read + vectors written, and launches) of both routes, the
bytes per row, and which of the two bounds -- the bytes at the copy's rate, the products at pow8's rate -- is the larger one
for the nine-term expression.

Timing: as tools/bench_prefix_scan.py -- the wall clock around `reps` queued calls bracketed by ark_hip_synchronize(), after
warm-up calls -- repeated ROUNDS times with the variants interleaved; the JSON keeps the median and the spread (max - min) of
the rounds.
The windows hold 200 / 50 / 20 calls at 2^20 / 2^22 / 2^24, tens of milliseconds each: with the 20 / 10 / 5 of the
neighbouring tools a single stall decides a round's figure at 2^20.

    python tools/bench_sum_of_products.py [--out profiles/sum_of_products.json] [--logs 20,22,24]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import algebra_amd as A  # noqa: E402
from algebra_amd import curves as cv  # noqa: E402
from algebra_amd._lib import check, lib  # noqa: E402
from tools.bench_poly_ops import limbs, periodic, rows  # noqa: E402
from tools.bench_prefix_scan import rounds, ROUNDS  # noqa: E402
from tools.bench_csr import summarise  # noqa: E402

FIELD = "BLS12_381_FR"
FID = cv.field_id(FIELD)
P = cv.SCALAR_MODULUS[FIELD]
R = (1 << 256) % P
RINV = pow(R, -1, P)
L_BLOCK = (1 << 16) - 1
NAMES = ["qM", "a", "b", "qL", "qR", "qO", "c", "qC", "z", "N", "D", "L1"]
STEP = 4


def mul(x, y):
    return x * y * RINV % P


def nine_terms(alpha):
    ix = {nm: k for k, nm in enumerate(NAMES)}
    a2 = mul(alpha, alpha)
    return [(None, [("qM", 0), ("a", 0), ("b", 0)]), (None, [("qL", 0), ("a", 0)]), (None, [("qR", 0), ("b", 0)]),
            (None, [("qO", 0), ("c", 0)]), (None, [("qC", 0)]), (alpha, [("z", 0), ("N", 0)]), (P - alpha, [("z", STEP), ("D", 0)]),
            (a2, [("L1", 0), ("z", 0)]), (P - a2, [("L1", 0)])], ix


def want_row(blocks, terms, n, i):
    acc = 0
    for coeff, factors in terms:
        pr = R if coeff is None else coeff
        for nm, rot in factors:
            pr = mul(pr, blocks[nm][((i + rot) % n) % L_BLOCK])
        acc += pr
    return acc % P


def composed(L, n, v, tmp, alpha, out):
    """the nine-term expression through the entries of the parent commit; tmp: eight vectors"""
    p1, p2, p3, p4, p5, p6, p7, zrot = tmp
    m = L.ark_hip_fr_mul_device
    check(m(FID, v["a"].ptr, v["b"].ptr, p1.ptr, n), "mul")
    check(m(FID, v["qM"].ptr, p1.ptr, p1.ptr, n), "mul")
    check(m(FID, v["qL"].ptr, v["a"].ptr, p2.ptr, n), "mul")
    check(m(FID, v["qR"].ptr, v["b"].ptr, p3.ptr, n), "mul")
    check(m(FID, v["qO"].ptr, v["c"].ptr, p4.ptr, n), "mul")
    check(m(FID, v["z"].ptr, v["N"].ptr, p5.ptr, n), "mul")
    check(L.ark_hip_memcpy_d2d(zrot.ptr, C.c_void_p(v["z"].ptr.value + STEP * 32), (n - STEP) * 32), "d2d")
    check(L.ark_hip_memcpy_d2d(C.c_void_p(zrot.ptr.value + (n - STEP) * 32), v["z"].ptr, STEP * 32), "d2d")
    check(m(FID, zrot.ptr, v["D"].ptr, p6.ptr, n), "mul")
    check(m(FID, v["L1"].ptr, v["z"].ptr, p7.ptr, n), "mul")
    a2 = mul(alpha, alpha)
    tabs = (C.c_void_p * 8)(*[t.ptr.value for t in (p1, p2, p3, p4, v["qC"], p5, p6, p7)])
    coeffs = limbs([R, R, R, R, R, alpha, P - alpha, a2])
    check(L.ark_hip_fr_lincomb_device(FID, tabs, 8, coeffs.ctypes.data_as(C.c_void_p), None, out.ptr, n), "lincomb")
    k = limbs([P - a2])
    check(L.ark_hip_fr_axpy_device(FID, out.ptr, k.ctypes.data_as(C.c_void_p), v["L1"].ptr, out.ptr, n), "axpy")


# vectors read + vectors written, and launches, of the two routes
COMPOSED_PASSES = {"launches": 12, "vector_reads": 8 * 2 + 1 + 8 + 2, "vector_writes": 8 + 1 + 1 + 1}
ONE_CALL_PASSES = {"launches": 1, "factor_reads": 17, "distinct_vector_reads": 13, "vector_writes": 1, "products_per_row": 12}


def same(x, y):
    return np.array_equal(x.to_host(), y.to_host())


def run(log_n, rng):
    L = lib()
    n = 1 << log_n
    reps = 200 if log_n <= 20 else 50 if log_n <= 22 else 20      # a timed window of tens of milliseconds: one stall does not decide a round
    blocks = {nm: [int.from_bytes(rng.bytes(40), "little") % P for _ in range(L_BLOCK)] for nm in NAMES}
    v = {nm: periodic(blocks[nm], n) for nm in NAMES}
    alpha = int.from_bytes(rng.bytes(40), "little") % (P - 1) + 1
    terms, ix = nine_terms(alpha)
    res = {"n": n, "reps": reps, "rounds": ROUNDS, "plan": dict(zip(("blocks", "rows_per_lane"), A.sum_of_products_plan(n)))}

    expr = A.SumOfProducts(FIELD, n)
    for coeff, factors in terms:
        expr.add_product([(v[nm], rot) for nm, rot in factors], None if coeff is None else limbs([coeff])[0])
    assert len(expr.columns) == 12 and len(expr.products) == 9
    out, ref = A.DeviceVec(FIELD, n, _zero=False), A.DeviceVec(FIELD, n, _zero=False)
    tmp = [A.DeviceVec(FIELD, n, _zero=False) for _ in range(8)]
    prod = A.SumOfProducts(FIELD, n).add_product([v["a"], v["b"]])
    pow8 = A.SumOfProducts(FIELD, n).add_product([v["a"]] * 8)
    rot = A.SumOfProducts(FIELD, n).add_product([(v["z"], STEP)])

    def two_copies():
        check(L.ark_hip_memcpy_d2d(ref.ptr, C.c_void_p(v["z"].ptr.value + STEP * 32), (n - STEP) * 32), "d2d")
        check(L.ark_hip_memcpy_d2d(C.c_void_p(ref.ptr.value + (n - STEP) * 32), v["z"].ptr, STEP * 32), "d2d")

    # every result first, checked over the whole vector against the route it replaces and at sampled rows; then the clock
    sample = sorted({0, 1, n - STEP - 1, n - STEP, n - 2, n - 1, n // 2} | {int(i) for i in rng.integers(0, n, size=25)})
    expr.evaluate(out)
    composed(L, n, v, tmp, alpha, ref)
    assert same(out, ref), "the nine-term expression differs from the composed route"
    assert np.array_equal(rows(out, sample), limbs([want_row(blocks, terms, n, i) for i in sample])), "nine_term"
    prod.evaluate(out)
    check(L.ark_hip_fr_mul_device(FID, v["a"].ptr, v["b"].ptr, ref.ptr, n), "mul")
    assert same(out, ref), "a b differs from ark_hip_fr_mul_device"
    rot.evaluate(out)
    two_copies()
    assert same(out, ref), "rotate differs from the two copies"
    pow8.evaluate(out)
    assert np.array_equal(rows(out, sample), limbs([want_row(blocks, [(None, [("a", 0)] * 8)], n, i) for i in sample])), "pow8"
    res["checked"] = "whole vectors bitwise against the composed route / fr_mul / two copies; %d sampled rows against big integers" % len(sample)

    t = rounds({
        "nine_term": lambda: expr.evaluate(out),
        "nine_term_composed": lambda: composed(L, n, v, tmp, alpha, ref),
        "mul": lambda: prod.evaluate(out),
        "fr_mul": lambda: check(L.ark_hip_fr_mul_device(FID, v["a"].ptr, v["b"].ptr, ref.ptr, n), "mul"),
        "pow8": lambda: pow8.evaluate(out),
        "rotate": lambda: rot.evaluate(out),
        "rotate_two_d2d": two_copies,
        "d2d": lambda: check(L.ark_hip_memcpy_d2d(ref.ptr, v["z"].ptr, n * 32), "d2d"),
    }, reps, warm=max(2, reps // 10))
    pin = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pin)), "host_alloc")

    def round_trip():
        check(L.ark_hip_memcpy_d2h(pin, v["z"].ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(ref.ptr, pin, n * 32), "h2d")
    t.update(rounds({"d2h_h2d": round_trip}, 5, warm=1))
    check(L.ark_hip_host_free(pin), "host_free")
    summarise(res, t)

    def beats(new, old):
        return bool(res[old + "_ms"] - res[new + "_ms"] > res[old + "_spread_ms"] + res[new + "_spread_ms"])
    res["composed_over_nine_term"] = round(res["nine_term_composed_ms"] / res["nine_term_ms"], 2)
    res["nine_term_beats_composed_beyond_spread"] = beats("nine_term", "nine_term_composed")
    res["nine_term_beats_d2h_h2d_beyond_spread"] = beats("nine_term", "d2h_h2d")
    res["mul_over_fr_mul"] = round(res["mul_ms"] / res["fr_mul_ms"], 3)
    res["rotate_over_two_d2d"] = round(res["rotate_ms"] / res["rotate_two_d2d_ms"], 3)
    res["rotate_beats_two_d2d_beyond_spread"] = beats("rotate", "rotate_two_d2d")
    # the two bounds of the nine-term call: 13 distinct vectors read + 1 written at the copy's rate (a copy moves two vectors);
    # 12 products per row at the rate pow8 shows (7 products per row, two vectors moved)
    gb = n * 32 / 1e6
    res["GB_per_s"] = {"d2d": round(2 * gb / res["d2d_ms"], 1), "fr_mul": round(3 * gb / res["fr_mul_ms"], 1), "mul": round(3 * gb / res["mul_ms"], 1),
                       "rotate": round(2 * gb / res["rotate_ms"], 1), "nine_term_distinct": round(14 * gb / res["nine_term_ms"], 1),
                       "nine_term_all_factor_reads": round(18 * gb / res["nine_term_ms"], 1)}
    res["products_per_ns"] = {"fr_mul": round(n / res["fr_mul_ms"] / 1e6, 2), "mul": round(n / res["mul_ms"] / 1e6, 2),
                              "pow8": round(7 * n / res["pow8_ms"] / 1e6, 2), "nine_term": round(12 * n / res["nine_term_ms"] / 1e6, 2)}
    per_vector, per_product = res["d2d_ms"] / 2, res["pow8_ms"] / 7      # ms per vector moved, ms per product and row

    def bounds(vectors, products):
        b = {"bytes_at_d2d_rate": round(vectors * per_vector, 4), "products_at_pow8_rate": round(products * per_product, 4)}
        return b, "vector ALU" if b["products_at_pow8_rate"] > b["bytes_at_d2d_rate"] else "HBM"
    res["nine_term_bounds_ms"], res["nine_term_bound_by"] = bounds(14, 12)
    res["mul_bounds_ms"], res["mul_bound_by"] = bounds(3, 1)
    res["pow8_bounds_ms"] = {"bytes_at_d2d_rate": round(2 * per_vector, 4)}   # far above it: pow8 is bound by its products
    for x in list(v.values()) + tmp + [out, ref]:
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_of_products.json"))
    ap.add_argument("--logs", default="20,22,24")
    args = ap.parse_args()
    rng = np.random.default_rng(25)
    out = {"field": FIELD, "date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; median and "
                     "spread (max - min) of `rounds` interleaved rounds",
           "expression": "qM a b + qL a + qR b + qO c + qC + alpha (z N - z(rot 4) D) + alpha^2 L1 (z - 1): 9 terms, 12 columns",
           "passes": {"one_call": ONE_CALL_PASSES, "composed": COMPOSED_PASSES,
                      "composed_route": "8 fr_mul + 2 memcpy_d2d (rotated z) + 1 fr_lincomb over 8 tables + 1 fr_axpy, 8 temporaries"},
           "sizes": []}
    for lg in (int(x) for x in args.logs.split(",")):
        r = run(lg, rng)
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    out["accepted"] = bool(all(s["nine_term_beats_composed_beyond_spread"] for s in out["sizes"]))
    out["not_measured"] = ["BN254 Fr and BLS12-377 Fr timings", "device times from a kernel trace (all figures are host-observed)",
                           "an operand-preload variant of the kernel (DESIGN.md section 25)", "the Rust mirror (source only, not compiled)"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
