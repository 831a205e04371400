"""Times the dense-multilinear-extension entries (evaluate, fix_variables with dim = 1 and dim = nu / 2, relabel with low and
with high windows, a + k x) at nu = 20, 22 and 24 over BLS12-381 Fr, next to three yardsticks measured in the same run:

  (a) ark_hip_memcpy_d2d of the table: what moving n * 32 bytes in and out of HBM costs;
  (b) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d of the table through pinned host memory: the only route there was before
      these entries (download, host arithmetic -- not even counted --, upload);
  (c) DeviceVec.evaluate (ark_hip_poly_evaluate_device) at the same length: the existing kernel with the same traffic.

Also timed: nu launches of fix_variables with dim = 1 chained (what a kernel that binds one variable per launch costs),
against the one evaluate call.

Every timed result is checked against Python big integers: the table is four random base blocks of 2^12 elements, block h
of the table being base block c[h] for a random map c, so that binding up to 12 low variables has 4 * 2^12 steps of big-integer
work whatever nu is, and what is left (2^(nu - 12) values) is folded in full.  Folded tables are compared element for
element, relabel and axpy at sampled indices.

Timing: the library runs on a stream of its own and exposes no events, so a call is timed by the wall clock around `reps`
queued calls bracketed by ark_hip_synchronize(), after warm-up calls.  evaluate returns a value to the host and waits inside
every call: its rows are HOST-OBSERVED LATENCY ("host_observed" in the JSON); the kernels' own times come from a kernel
trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/bench_mle_ops.py --one 24).

Every size runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_mle_ops.py [--out profiles/mle_ops.json] [--logs 20,22,24] [--limit 240]
    python tools/bench_mle_ops.py --one 24          (one size in this process, its JSON line on stdout)
"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD = "BLS12_381_FR"
LO = 12                                                # variables inside a base block


def limbs(xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def fold(table, point, p):
    """dense.rs:224-257 on integers"""
    t = list(table)
    for r in point:
        t = [(t[2 * b] + r * (t[2 * b + 1] - t[2 * b])) % p for b in range(len(t) // 2)]
    return t


def swap_bits(x, a, b, n):
    d = ((x >> a) ^ (x >> b)) & ((1 << n) - 1)
    return x ^ ((d << a) | (d << b))


def issues_per_element(nu, tile_log, widths, tiles):
    """vector multiplies a wave issues per element of the table, masked lanes included, from the structure of mle_fold_kernel
    (csrc/mle.cuh) and the library's own plan (ark_hip_mle_fold_plan / _fold_tiles): a launch that binds w bits gives a wave
    2^gl tiles of 2^tile_log elements, 2^(tile_log - 6) per lane and tile (a wave has 2^6 lanes); the bits above the lane's
    are bound between registers (every product useful), then one step per lane bit with half the lane's streams as
    products while it holds more than one"""
    lane_log = 6
    per_lane = 1 << (tile_log - lane_log)
    total, m = 0.0, nu
    for w, gl in zip(widths, tiles):
        na = max(w - lane_log, 0)
        per_wave = (per_lane - (per_lane >> na)) << gl
        s = (per_lane >> na) << gl
        for _ in range(w - na):
            per_wave += max(s // 2, 1)
            s = max(s // 2, 1)
        waves = max((1 << m) >> (tile_log + gl), 1)
        total += per_wave * waves * 64
        m -= w
    return total / (1 << nu)


def timed(fn, reps, warm=2):
    from algebra_amd._lib import check, lib
    L = lib()
    for _ in range(warm):
        fn()
    check(L.ark_hip_synchronize(), "sync")
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    check(L.ark_hip_synchronize(), "sync")
    return (time.perf_counter() - t0) * 1e3 / reps


def run(nu):
    import algebra_amd as A
    from algebra_amd import curves as cv
    from algebra_amd._lib import check, lib
    L = lib()
    P = cv.SCALAR_MODULUS[FIELD]
    R = (1 << 256) % P
    RINV = pow(R, -1, P)
    rng = np.random.default_rng(100 + nu)
    n = 1 << nu
    reps = 20 if nu <= 20 else 10 if nu <= 22 else 5
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % P   # noqa: E731
    base = [[rnd() for _ in range(1 << LO)] for _ in range(4)]
    cmap = rng.integers(0, 4, size=n >> LO)
    a = limbs([x for blk in base for x in blk]).reshape(4, 1 << LO, 4)[cmap].reshape(-1, 4)
    point = [rnd() for _ in range(nu)]
    pointM = limbs([x * R % P for x in point])
    m = A.DenseMultilinearExtension.from_evaluations(FIELD, nu, a)
    tab = m.evaluations
    tile_log, widths = A.mle_fold_plan(nu, nu)
    res = {"num_vars": nu, "n": n, "reps": reps, "tile_log": tile_log, "evaluate_widths": widths,
           "evaluate_tiles_per_wave_log": A.mle_fold_tiles(nu, nu)}

    def rows(v, idx):
        out = np.zeros((len(idx), 4), dtype=np.uint64)
        for k, i in enumerate(idx):
            check(L.ark_hip_memcpy_d2h(out[k].ctypes.data_as(C.c_void_p), C.c_void_p(v.ptr.value + int(i) * 32), 32), "d2h")
        return out

    sample = sorted({0, 1, 511, 512, 513, n // 2, n - 2, n - 1} | {int(v) for v in rng.integers(0, n, size=24)})

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
    res["poly_evaluate_ms"] = timed(lambda: tab.evaluate(pointM[0]), reps)

    # the model: every base block folded over the low variables, what is left folded in full
    def folded(dim):                                   # dim <= LO: element for element
        fb = limbs([x for blk in base for x in fold(blk, point[:dim], P)]).reshape(4, 1 << (LO - dim), 4)
        return fb[cmap].reshape(-1, 4)
    low = [fold(blk, point[:LO], P)[0] for blk in base]
    value = limbs([fold([low[q] for q in cmap], point[LO:], P)[0]])[0]

    # evaluate
    res["evaluate_ms"] = timed(lambda: m.evaluate(pointM), reps)
    assert np.array_equal(m.evaluate(pointM), value), "evaluate"
    res["evaluate_issues_per_element"] = round(issues_per_element(nu, tile_log, widths, A.mle_fold_tiles(nu, nu)), 3)

    # fix_variables, dim = 1 and dim = nu / 2
    for label, dim in (("fix_1", 1), ("fix_half", nu // 2)):
        out = A.DeviceVec(FIELD, n >> dim, _zero=False)
        pt = pointM[:dim]
        res[label + "_ms"] = timed(lambda: check(L.ark_hip_mle_fix_variables_device(
            tab.field, tab.ptr, nu, pt.ctypes.data_as(C.c_void_p), dim, out.ptr), "fix_variables"), reps)
        assert dim <= LO and np.array_equal(out.to_host(), folded(dim)), label
        res[label + "_dim"] = dim
        res[label + "_issues_per_element"] = round(issues_per_element(nu, tile_log, A.mle_fold_plan(nu, dim)[1], A.mle_fold_tiles(nu, dim)), 3)
        out.free()

    # nu launches that bind one variable each, chained through two buffers: the kernel this change does not build
    bufs = [A.DeviceVec(FIELD, n // 2, _zero=False), A.DeviceVec(FIELD, n // 4, _zero=False)]

    def one_by_one():
        src = tab
        for d in range(nu):
            dst = bufs[d % 2]
            check(L.ark_hip_mle_fix_variables_device(tab.field, src.ptr, nu - d, pointM[d].ctypes.data_as(C.c_void_p), 1, dst.ptr), "fix 1")
            src = dst
    res["evaluate_as_dim1_launches_ms"] = timed(one_by_one, reps)
    assert np.array_equal(rows(bufs[(nu - 1) % 2], [0])[0], value), "one variable per launch"
    for v in bufs:
        v.free()

    # relabel: low windows (inside a wave's 2 KiB) and high windows (whole strides apart), out of place and in place
    for label, (wa, wb, k) in (("relabel_low", (0, 3, 3)), ("relabel_high", (nu - 8, nu - 4, 4))):
        res[label + "_ms"] = timed(lambda: check(L.ark_hip_mle_relabel_device(tab.field, tab.ptr, nu, wa, wb, k, other.ptr), "relabel"), reps)
        assert np.array_equal(rows(other, sample), a[[swap_bits(i, wa, wb, k) for i in sample]]), label
        work = tab.clone()
        res[label + "_in_place_ms"] = timed(lambda: check(L.ark_hip_mle_relabel_device(tab.field, work.ptr, nu, wa, wb, k, work.ptr), "relabel"),
                                            2 * (reps // 2), warm=2)     # an even number of exchanges: the table itself again
        assert np.array_equal(rows(work, sample), a[sample]), label + " in place"
        work.free()

    # axpy
    kk = rnd()
    kM = limbs([kk * R % P])[0]
    x = A.DeviceVec(FIELD, n, _zero=False)
    check(L.ark_hip_mle_relabel_device(tab.field, tab.ptr, nu, 0, nu - 2, 2, x.ptr), "relabel")   # a second table
    res["axpy_ms"] = timed(lambda: check(L.ark_hip_fr_axpy_device(tab.field, tab.ptr, kM.ctypes.data_as(C.c_void_p), x.ptr, other.ptr, n), "axpy"), reps)
    am = ints(a[sample])
    xm = ints(a[[swap_bits(i, 0, nu - 2, 2) for i in sample]])
    assert np.array_equal(rows(other, sample), limbs([(u + kk * v) % P for u, v in zip(am, xm)])), "axpy"

    moved = {"evaluate": 1, "poly_evaluate": 1, "fix_1": 1.5, "fix_half": 1, "relabel_low": 2, "relabel_high": 2,
             "relabel_low_in_place": 2, "relabel_high_in_place": 2, "axpy": 3}
    per_byte = res["d2d_ms"] / (2 * n * 32)
    res["host_observed"] = ["evaluate", "poly_evaluate"]
    res["times_d2d_per_byte"] = {k: round(res[k + "_ms"] / (f * n * 32) / per_byte, 2) for k, f in moved.items()}
    res["faster_than_d2h_h2d"] = {k: bool(res[k + "_ms"] < res["d2h_h2d_ms"]) for k in moved}
    res["evaluate_vs_poly_evaluate"] = round(res["evaluate_ms"] / res["poly_evaluate_ms"], 3)
    res["dim1_launches_vs_evaluate"] = round(res["evaluate_as_dim1_launches_ms"] / res["evaluate_ms"], 2)
    for v in (x, other):
        v.free()
    m.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_ops.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up",
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
