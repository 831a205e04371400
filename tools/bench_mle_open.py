"""Times the two multilinear-opening entries -- the eq table (ark_hip_mle_eq_table_device) and the
quotients of an opening (ark_hip_mle_quotients_device, with and without the value) -- at nu = 20, 22 and 24 over BLS12-381 Fr,
next to yardsticks measured in the same run:

  (a) ark_hip_memcpy_d2d of 2^nu elements: what moving n * 32 bytes in and out of HBM costs;
  (b) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d of 2^nu elements through pinned host memory: the transfer the host route cannot
      avoid -- a FLOOR for it, the host's own 2^nu products are not counted;
  (c) ark_hip_mle_evaluate_device on the same table: the quotients' reads without their writes;
  (d) nu chained launches of fix_variables with dim = 1: the reads of a quotient route that binds one variable per launch,
      without any of its quotient writes -- a floor for that route.

The one claim checked (the run fails otherwise): each new call is faster than (b) at every size.  The ratios to (a), (c) and
(d) and the achieved product rate are reported, not promised.

Every timed result is checked against Python big integers: the eq table at sampled indices against the product formula;
the value in full and sampled rows of every quotient segment on a table of four random base blocks of 2^12 elements laid
out by a random map (tools/bench_mle_ops.py), whose quotients below 12 variables are the blocks' own and whose 2^(nu-12)
rows above are walked in full.

Timing: wall clock around `reps` queued calls between two ark_hip_synchronize(), after warm-up.  The quotients with a value
and evaluate wait inside every call: HOST-OBSERVED LATENCY ("host_observed" in the JSON).

Every size runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_mle_open.py [--out profiles/mle_open.json] [--logs 20,22,24] [--limit 240]
    python tools/bench_mle_open.py --one 24          (one size in this process, its JSON line on stdout)
"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mle_ops import FIELD, LO, fold, ints, limbs, timed   # noqa: E402

PRODUCT_RATE_G = 124.0                                 # 256-bit Montgomery products per second the chip sustains


def eq_issues_per_output(nu, tile_log, widths, tiles):
    """vector multiplies a wave of mle_eq_kernel issues per output, masked lanes included (csrc/mle_open.cuh): 5 + 7 for a
    lane's own weights once per wave, then 8 per tile; summed over the launches of the plan"""
    total, m = 0, 0
    for w, gl in zip(widths, tiles):
        m += w
        waves = max((1 << m) >> (tile_log + gl), 1)
        total += waves * 64 * (12 + (8 << gl))
    return total / (1 << nu)


def quotient_issues_per_element(nu, tile_log, widths):
    """the same for mle_quot_kernel: 4 + 2 + 1 between a lane's registers, one per lane bit after that"""
    total, m = 0, nu
    for w in widths:
        per_lane = sum(8 >> (a + 1) for a in range(min(w, 3))) + max(w - 3, 0)
        total += max((1 << m) >> tile_log, 1) * 64 * per_lane
        m -= w
    return total / (1 << nu)


def quotients_model(table, point, p):
    f, qs = list(table), []
    for r in point:
        qs.append([(f[2 * b + 1] - f[2 * b]) % p for b in range(len(f) // 2)])
        f = [(f[2 * b] + r * qs[-1][b]) % p for b in range(len(f) // 2)]
    return f[0], qs


def run(nu):
    import algebra_amd as A
    from algebra_amd import curves as cv
    from algebra_amd._lib import check, lib
    L = lib()
    P = cv.SCALAR_MODULUS[FIELD]
    R = (1 << 256) % P
    rng = np.random.default_rng(200 + nu)
    n = 1 << nu
    reps = 20 if nu <= 20 else 10 if nu <= 22 else 5
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % P   # noqa: E731
    base = [[rnd() for _ in range(1 << LO)] for _ in range(4)]
    cmap = rng.integers(0, 4, size=n >> LO)
    a = limbs([x for blk in base for x in blk]).reshape(4, 1 << LO, 4)[cmap].reshape(-1, 4)
    point = [rnd() for _ in range(nu)]
    pointM = limbs([x * R % P for x in point])
    scale = rnd()
    scaleM = limbs([scale * R % P])[0]
    m = A.DenseMultilinearExtension.from_evaluations(FIELD, nu, a)
    tab = m.evaluations
    tile_log, eq_widths, eq_tiles = A.mle_eq_plan(nu)
    _, q_widths, q_tiles = A.mle_quotients_plan(nu)
    res = {"num_vars": nu, "n": n, "reps": reps, "tile_log": tile_log, "eq_widths": eq_widths, "eq_tiles_per_wave_log": eq_tiles,
           "quotient_widths": q_widths, "quotient_tiles_per_wave_log": q_tiles}

    def rows(ptr, idx):
        out = np.zeros((len(idx), 4), dtype=np.uint64)
        for k, i in enumerate(idx):
            check(L.ark_hip_memcpy_d2h(out[k].ctypes.data_as(C.c_void_p), C.c_void_p(ptr.value + int(i) * 32), 32), "d2h")
        return out

    # yardsticks
    other = A.DeviceVec(FIELD, n, _zero=False)
    res["d2d_ms"] = timed(lambda: check(L.ark_hip_memcpy_d2d(other.ptr, tab.ptr, n * 32), "d2d"), reps)
    pinned = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")

    def round_trip():
        check(L.ark_hip_memcpy_d2h(pinned, tab.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(other.ptr, pinned, n * 32), "h2d")
    res["d2h_h2d_ms"] = timed(round_trip, max(3, reps // 2), warm=1)
    check(L.ark_hip_host_free(pinned), "host_free")
    res["evaluate_ms"] = timed(lambda: m.evaluate(pointM), reps)
    bufs = [A.DeviceVec(FIELD, n // 2, _zero=False), A.DeviceVec(FIELD, n // 4, _zero=False)]

    def one_by_one():
        src = tab
        for d in range(nu):
            dst = bufs[d % 2]
            check(L.ark_hip_mle_fix_variables_device(tab.field, src.ptr, nu - d, pointM[d].ctypes.data_as(C.c_void_p), 1, dst.ptr), "fix 1")
            src = dst
    res["fold_as_dim1_launches_ms"] = timed(one_by_one, reps)
    for v in bufs:
        v.free()

    # the eq table
    pt_p, sc_p = pointM.ctypes.data_as(C.c_void_p), scaleM.ctypes.data_as(C.c_void_p)
    res["eq_ms"] = timed(lambda: check(L.ark_hip_mle_eq_table_device(tab.field, pt_p, nu, sc_p, other.ptr), "eq"), reps)
    T = 1 << tile_log
    sample = sorted({0, 1, 63, 64, T - 1, T, n // 2, n // 2 + T - 1, n - T, n - 2, n - 1} | {int(v) for v in rng.integers(0, n, size=245)})

    def eq_at(i):
        w = scale
        for j, r in enumerate(point):
            w = w * (r if (i >> j) & 1 else 1 - r) % P
        return w * R % P
    assert np.array_equal(rows(other.ptr, sample), limbs([eq_at(i) for i in sample])), "eq table"
    res["eq_issues_per_output"] = round(eq_issues_per_output(nu, tile_log, eq_widths, eq_tiles), 4)

    # the quotients: the model -- the blocks' own quotients below LO variables, the rows above walked in full
    per_block = [quotients_model(blk, point[:LO], P) for blk in base]
    value, high = quotients_model([per_block[q][0] for q in cmap], point[LO:], P)
    quot = A.DeviceVec(FIELD, n - 1, _zero=False)
    out = np.zeros(4, dtype=np.uint64)
    ev_p, out_p = tab.ptr, out.ctypes.data_as(C.c_void_p)
    res["quotients_ms"] = timed(lambda: check(L.ark_hip_mle_quotients_device(tab.field, ev_p, nu, pt_p, quot.ptr, out_p), "quotients"), reps)
    assert np.array_equal(out, limbs([value])[0]) and np.array_equal(out, m.evaluate(pointM)), "the value"

    def check_segments(tag):
        for i in range(nu):
            off, ln = n - (n >> i), n >> (i + 1)
            idx = sorted({0, ln - 1, ln // 2} | {int(v) for v in rng.integers(0, ln, size=13)})
            if i < LO:
                per = 1 << (LO - 1 - i)
                want = [per_block[cmap[b // per]][1][i][b % per] for b in idx]
            else:
                want = [high[i - LO][b] for b in idx]
            assert np.array_equal(rows(quot.ptr, [off + b for b in idx]), limbs(want)), (tag, "segment", i)
    check_segments("with the value")
    check(L.ark_hip_memset_device(quot.ptr, 0, (n - 1) * 32), "memset")
    res["quotients_async_ms"] = timed(lambda: check(L.ark_hip_mle_quotients_device(tab.field, ev_p, nu, pt_p, quot.ptr, None), "quotients"), reps)
    check_segments("asynchronous")
    res["quotient_issues_per_element"] = round(quotient_issues_per_element(nu, tile_log, q_widths), 4)
    assert np.array_equal(rows(tab.ptr, sample), a[sample]), "input changed"

    per_byte = res["d2d_ms"] / (2 * n * 32)
    moved = {"eq": 1, "quotients": 2, "quotients_async": 2, "evaluate": 1}     # tables of n elements read or written
    res["host_observed"] = ["quotients", "evaluate"]
    res["times_d2d_per_byte"] = {k: round(res[k + "_ms"] / (f * n * 32) / per_byte, 2) for k, f in moved.items()}
    res["faster_than_d2h_h2d"] = {k: bool(res[k + "_ms"] < res["d2h_h2d_ms"]) for k in ("eq", "quotients", "quotients_async")}
    res["d2h_h2d_over"] = {k: round(res["d2h_h2d_ms"] / res[k + "_ms"], 1) for k in ("eq", "quotients", "quotients_async")}
    res["quotients_vs_evaluate"] = round(res["quotients_ms"] / res["evaluate_ms"], 2)
    res["quotients_async_vs_fold_as_dim1_launches"] = round(res["quotients_async_ms"] / res["fold_as_dim1_launches_ms"], 2)
    res["eq_products_G_per_s"] = round(res["eq_issues_per_output"] * n / (res["eq_ms"] * 1e-3) / 1e9, 1)
    res["quotients_async_products_G_per_s"] = round(res["quotient_issues_per_element"] * n / (res["quotients_async_ms"] * 1e-3) / 1e9, 1)
    res["product_rate_of_section_4_G_per_s"] = PRODUCT_RATE_G
    assert all(res["faster_than_d2h_h2d"].values()), ("a new call is slower than the transfer it replaces", res)
    for v in (quot, other):
        v.free()
    m.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_open.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up",
           "claim": "eq, quotients and quotients_async are each faster than d2h_h2d at every size (asserted by the tool)",
           "sizes": []}
    for lg in (int(x) for x in args.logs.split(",")):
        # a fresh process per size, under its own time limit; a failure ends the run: nothing more is started on the GPU
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(lg)],
                               capture_output=True, text=True)
        line = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")]
        if child.returncode != 0 or not line:
            print(child.stdout + child.stderr)
            print("size 2^%d failed with status %d: stopping" % (lg, child.returncode))
            return 1
        r = json.loads(line[-1][len("RESULT "):])
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
