"""Times the products of a device-resident CSR matrix (ark_hip_fr_csr_mul_device: y = M x and y = M^T x) over BLS12-381 Fr on
synthetic R1CS-like matrices built here from a fixed seed -- square with 2^20, 2^22 and 2^24 rows, 1 to 4 nonzeros per row
(2.5 on average), column 0 present in a quarter of the rows (so row 0 of M^T is a long row of rows / 4 entries), 90 % of the
values +1 or -1 -- plus one degenerate matrix of a single row with 2^24 nonzeros, and ark_hip_fr_csr_create with and without
the transpose (one-time cost per circuit: recorded once, not gated).  Yardsticks measured in the same run:

  (a) ark_hip_memcpy_d2d of one vector;
  (b) ark_hip_memcpy_d2h of x plus ark_hip_memcpy_h2d of y through pinned host memory: the floor of the host route, the host
      multiplication itself not counted;
  (c) ark_hip_fr_inner_product_device over as many elements as the single-row matrix has nonzeros: the same products and sums
      with both operands streamed instead of one gathered.

Every timed result is checked against Python big integers at 32 sampled rows (row 0 of M^T, the long one, among them).  The
vectors are a random block of L = 2^16 - 1 elements repeated, so x[j] = block[j mod L] is known without a download.

Timing: as tools/bench_prefix_scan.py -- the wall clock around `reps` queued calls bracketed by ark_hip_synchronize(), after
warm-up calls -- repeated ROUNDS times with the variants interleaved; the JSON keeps the median and the spread (max - min) of
the rounds.

    python tools/bench_csr.py [--out profiles/csr_mul.json] [--logs 20,22,24] [--single-log 24]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import algebra_amd as A  # noqa: E402
from algebra_amd import curves as cv  # noqa: E402
from algebra_amd._lib import check, lib  # noqa: E402
from tools.bench_poly_ops import limbs, periodic, rows  # noqa: E402
from tools.bench_prefix_scan import rounds, ROUNDS  # noqa: E402

FIELD = "BLS12_381_FR"
P = cv.SCALAR_MODULUS[FIELD]
R = (1 << 256) % P
RINV = pow(R, -1, P)
L_BLOCK = (1 << 16) - 1
POOL = 4096          # distinct "other" coefficients


def rand_block(rng):
    return [int.from_bytes(rng.bytes(40), "little") % P for _ in range(L_BLOCK)]


def r1cs_like(n, rng):
    """(row_ptr, col_idx, value index per nonzero, value table as integers): n x n"""
    lens = rng.choice(np.array([1, 2, 3, 4], dtype=np.int64), size=n, p=[0.2, 0.3, 0.3, 0.2])
    row_ptr = np.zeros(n + 1, dtype=np.uint32)
    row_ptr[1:] = np.cumsum(lens)
    nnz = int(row_ptr[-1])
    col_idx = rng.integers(1, n, size=nnz, dtype=np.uint32)
    col_idx[row_ptr[:-1][::4]] = 0                                   # the constant column, in every fourth row
    table = [R % P, (P - R) % P] + [int.from_bytes(rng.bytes(40), "little") % P for _ in range(POOL)]
    kind = rng.random(nnz)
    vidx = np.where(kind < 0.45, 0, np.where(kind < 0.9, 1, 2 + rng.integers(0, POOL, size=nnz))).astype(np.int32)
    return row_ptr, col_idx, vidx, table


def want_rows(row_ptr, col_idx, vidx, table, block, sample):
    """stored (M x)[r] for r in sample with x[j] = block[j mod L], by big integers"""
    out = []
    for r in sample:
        a, b = int(row_ptr[r]), int(row_ptr[r + 1])
        cs, vs = col_idx[a:b].astype(np.int64) % L_BLOCK, vidx[a:b]
        out.append(sum(table[int(v)] * block[int(c)] for v, c in zip(vs, cs)) * RINV % P)
    return limbs(out)


def want_cols(n_rows, row_ptr, col_idx, vidx, table, block, sample):
    """stored (M^T u)[c] for c in sample with u[i] = block[i mod L]"""
    out = []
    for c in sample:
        js = np.nonzero(col_idx == np.uint32(c))[0]
        rs = (np.searchsorted(row_ptr, js, side="right") - 1) % L_BLOCK
        out.append(sum(table[int(v)] * block[int(r)] for v, r in zip(vidx[js], rs)) * RINV % P)
    return limbs(out)


def yardsticks(n, x, out, reps):
    L = lib()
    pin = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pin)), "host_alloc")

    def round_trip():
        check(L.ark_hip_memcpy_d2h(pin, x.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(out.ptr, pin, n * 32), "h2d")
    t = rounds({"d2d": lambda: check(L.ark_hip_memcpy_d2d(out.ptr, x.ptr, n * 32), "d2d")}, reps)
    t.update(rounds({"d2h_h2d": round_trip}, max(2, reps // 4), warm=1))
    check(L.ark_hip_host_free(pin), "host_free")
    return t


def summarise(res, t):
    for k, v in t.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = round(max(v) - min(v), 4)


def beats(res, name, yard="d2h_h2d"):
    gain = res[yard + "_ms"] - res[name + "_ms"]
    return bool(gain > res[yard + "_spread_ms"] + res[name + "_spread_ms"])


def run_square(log_n, rng):
    n = 1 << log_n
    reps = 20 if log_n <= 20 else 10 if log_n <= 22 else 5
    row_ptr, col_idx, vidx, table = r1cs_like(n, rng)
    nnz = int(row_ptr[-1])
    vals = limbs(table)[vidx]
    bx, bu = rand_block(rng), rand_block(rng)
    x, u = periodic(bx, n), periodic(bu, n)
    t0 = time.perf_counter()
    plain = A.CsrMatrix(FIELD, n, n, row_ptr, col_idx, vals)
    t1 = time.perf_counter()
    plain.free()
    t2 = time.perf_counter()
    m = A.CsrMatrix(FIELD, n, n, row_ptr, col_idx, vals, transpose=True)
    t3 = time.perf_counter()
    del vals
    plan = A.csr_plan(n, row_ptr)
    t_ptr = np.zeros(n + 1, dtype=np.uint32)
    t_ptr[1:] = np.cumsum(np.bincount(col_idx, minlength=n))
    plan_t = A.csr_plan(n, t_ptr)
    res = {"rows": n, "cols": n, "nnz": nnz, "nnz_per_row": round(nnz / n, 3), "long_row_of_transpose": int(t_ptr[1]), "reps": reps,
           "rounds": ROUNDS, "checked_rows": 32, "create_ms": round((t1 - t0) * 1e3, 1), "create_with_transpose_ms": round((t3 - t2) * 1e3, 1),
           "plan": dict(zip(("tile", "max_rows", "blocks", "long_rows", "long_chunks"), plan)),
           "plan_transpose": dict(zip(("tile", "max_rows", "blocks", "long_rows", "long_chunks"), plan_t))}
    sample = {0, 1, 2, 3, 4, n // 2, n - 2, n - 1}
    while len(sample) < 32:
        sample.add(int(rng.integers(0, n)))
    sample = sorted(sample)
    y, yt = A.DeviceVec(FIELD, n, _zero=False), A.DeviceVec(FIELD, n, _zero=False)
    # every result first, checked; then the clock
    m.mul(x, out=y)
    assert np.array_equal(rows(y, sample), want_rows(row_ptr, col_idx, vidx, table, bx, sample)), "mul"
    m.mul_t(u, out=yt)
    assert np.array_equal(rows(yt, sample), want_cols(n, row_ptr, col_idx, vidx, table, bu, sample)), "mul_t"
    t = rounds({"mul": lambda: m.mul(x, out=y), "mul_t": lambda: m.mul_t(u, out=yt)}, reps)
    t.update(yardsticks(n, x, y, reps))
    summarise(res, t)
    res["mul_beats_d2h_h2d_beyond_spread"] = beats(res, "mul")
    res["mul_t_beats_d2h_h2d_beyond_spread"] = beats(res, "mul_t")
    res["mul_over_d2d"] = round(res["mul_ms"] / res["d2d_ms"], 2)
    res["mul_t_over_d2d"] = round(res["mul_t_ms"] / res["d2d_ms"], 2)
    res["ns_per_nonzero"] = {"mul": round(res["mul_ms"] * 1e6 / nnz, 3), "mul_t": round(res["mul_t_ms"] * 1e6 / nnz, 3)}
    for v in (x, u, y, yt, m):
        v.free()
    return res


def run_single_row(log_nnz, rng):
    """one row holding 2^log_nnz nonzeros over 2^log_nnz columns, columns random: every chunk gathers"""
    L = lib()
    n = 1 << log_nnz
    reps = 5
    row_ptr = np.array([0, n], dtype=np.uint32)
    col_idx = rng.integers(0, n, size=n, dtype=np.uint32)
    table = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(POOL)]
    vidx = rng.integers(0, POOL, size=n).astype(np.int32)
    vals = limbs(table)[vidx]
    bx = rand_block(rng)
    x = periodic(bx, n)
    m = A.CsrMatrix(FIELD, 1, n, row_ptr, col_idx, vals)
    dvals = A.DeviceVec.from_host(FIELD, vals)
    del vals
    y, out = A.DeviceVec(FIELD, 1, _zero=False), A.DeviceVec(FIELD, n, _zero=False)
    host = np.zeros(4, dtype=np.uint64)
    res = {"rows": 1, "cols": n, "nnz": n, "reps": reps, "rounds": ROUNDS,
           "plan": dict(zip(("tile", "max_rows", "blocks", "long_rows", "long_chunks"), A.csr_plan(1, row_ptr)))}
    m.mul(x, out=y)
    # the whole row against big integers: sum_v table[v] S_v with S_v the sum of x over the nonzeros that hold coefficient v,
    # added limb by limb (32-bit limbs, at most 2^24 terms: exact in a double)
    cj = col_idx.astype(np.int64) % L_BLOCK
    bl = limbs(bx).view(np.uint32).reshape(-1, 8)
    sums = [0] * POOL
    for k in range(8):
        s = np.bincount(vidx, weights=bl[cj, k].astype(np.float64), minlength=POOL)
        for v in range(POOL):
            sums[v] += int(s[v]) << (32 * k)
    want = sum(table[v] * sums[v] for v in range(POOL)) * RINV % P
    assert np.array_equal(y.to_host()[0], limbs([want])[0]), "the single row"
    t = rounds({"mul": lambda: m.mul(x, out=y),
                "inner_product": lambda: check(L.ark_hip_fr_inner_product_device(x.field, dvals.ptr, x.ptr, n, host.ctypes.data_as(C.c_void_p)), "inner")}, reps)
    t.update(yardsticks(n, x, out, reps))
    summarise(res, t)
    res["mul_beats_d2h_h2d_beyond_spread"] = beats(res, "mul")
    res["mul_over_inner_product"] = round(res["mul_ms"] / res["inner_product_ms"], 2)
    res["ns_per_nonzero"] = round(res["mul_ms"] * 1e6 / n, 3)
    res["note"] = "inner_product returns its value to the host (one 32-byte download and its wait inside every call); mul is asynchronous"
    for v in (x, y, out, dvals, m):
        v.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_mul.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--single-log", type=int, default=24)
    args = ap.parse_args()
    rng = np.random.default_rng(24)
    out = {"field": FIELD, "date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; median and "
                     "spread (max - min) of `rounds` interleaved rounds; create_*: one call each, wall clock, host work and uploads included",
           "sizes": []}
    for lg in (int(v) for v in args.logs.split(",")):
        r = run_square(lg, rng)
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    out["single_row"] = run_single_row(args.single_log, rng)
    print(json.dumps(out["single_row"]), flush=True)
    out["accepted"] = bool(all(s["mul_beats_d2h_h2d_beyond_spread"] and s["mul_t_beats_d2h_h2d_beyond_spread"] for s in out["sizes"])
                           and out["single_row"]["mul_beats_d2h_h2d_beyond_spread"])
    out["not_measured"] = ["BN254 Fr and BLS12-377 Fr timings", "device times from a kernel trace (all figures are host-observed)",
                           "the Rust mirror (source only, not compiled)", "a value dictionary for the +-1-heavy coefficients (priced in DESIGN.md section 24, not built)"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
