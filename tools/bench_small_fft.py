"""Times the transforms and pointwise kernels over the one-word fields (Goldilocks, BabyBear, KoalaBear: ark_hip_sfp_*) on device-
resident data: one transform at 2^16, 2^20 and 2^24, a batch of 64 x 2^20, the 4x low-degree extension of 64 x 2^18 (batched
inverse at 2^18, then batched forward of 2^18 coefficients on the coset of 2^20), and mul and inverse at 2^24 -- next to three
yardsticks measured in the same run:

  (a) ark_hip_memcpy_d2d of the same bytes: what reading and writing them once costs;
  (b) ark_hip_fft_in_place_device over BLS12-381 Fr at the same lengths (the transform this library had before);
  (c) the upload + download of the vector through pinned host memory.

Each transform is reported as a multiple of (passes x the copy time of its bytes) and per element against the Fr transform of the
same length; `faster_per_element_than_fr_beyond_spread` is the one condition.

Every timed entry is checked first: the transforms on an input with 258 non-zero coefficients, whose values at 8 sampled domain
elements are a short sum of big-integer powers (the kernels' work does not depend on the data), and by inverse(forward(x)) == x on a
dense random vector; mul and inverse against Python integers at 64 sampled indices.

Timing: the wall clock around `reps` queued calls between two ark_hip_synchronize(), after warm-up calls, repeated ROUNDS times with
the variants interleaved, so the chip is busy before and while the clock runs; the JSON keeps the median and the spread (max - min).

    python tools/bench_small_fft.py [--out profiles/small_fft.json] [--logs 16,20,24] [--quick]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import algebra_amd as A  # noqa: E402
from algebra_amd._lib import check, lib  # noqa: E402
import smallfp_ref as R  # noqa: E402

ROUNDS = 5
FR = "BLS12_381_FR"


def rounds(variants, reps, warm=2):
    L = lib()
    out = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warm):
            fn()
    check(L.ark_hip_synchronize(), "sync")
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            check(L.ark_hip_synchronize(), "sync")
            out[name].append((time.perf_counter() - t0) * 1e3 / reps)
    return {k: (round(statistics.median(v), 5), round(max(v) - min(v), 5)) for k, v in out.items()}


def dt(f):
    return np.uint64 if f.bytes == 8 else np.uint32


def check_transform(f, log_n, rng):
    """forward coset transform of a sparse input at 8 sampled outputs against big integers; inverse(forward(dense)) == dense"""
    n = 1 << log_n
    m = f.get_coset(f.domain_new(n), f.gen)
    d = A.SmallRadix2EvaluationDomain.new(f.name, n).get_coset(f.gen)
    support = sorted({0, n - 1} | {int(i) for i in rng.integers(0, n, size=256)})
    vals = {i: int(rng.integers(1, f.p, dtype=np.uint64)) for i in support}
    x = np.zeros(n, dtype=dt(f))
    for i, v in vals.items():
        x[i] = v
    v = A.SmallDeviceVec.from_host(f.name, x)
    d.fft_batch_in_place(v.ptr, 1)
    got = v.to_host()
    for j in [0, n - 1] + [int(i) for i in rng.integers(0, n, size=6)]:
        pt = f.from_mont(f.domain_element(m, j))
        want = sum(f.from_mont(c) * pow(pt, i, f.p) for i, c in vals.items()) % f.p
        assert int(got[j]) == f.to_mont(want), (f.name, log_n, j)
    dense = rng.integers(0, f.p, size=n, dtype=np.uint64).astype(dt(f))
    w = A.SmallDeviceVec.from_host(f.name, dense)
    d.fft_batch_in_place(w.ptr, 1)
    assert not np.array_equal(w.to_host(), dense)
    d.fft_batch_in_place(w.ptr, 1, inverse=True)
    assert np.array_equal(w.to_host(), dense), (f.name, log_n, "inverse(forward(x)) != x")
    v.free()
    w.free()


def fr_transform_ms(log_n, reps):
    n = 1 << log_n
    L = lib()
    d = A.Radix2EvaluationDomain.new(FR, n)
    p = C.c_void_p()
    check(L.ark_hip_malloc(n * 32, C.byref(p)), "malloc")
    check(L.ark_hip_memset_device(p, 0, n * 32), "memset")
    one = np.zeros(4, dtype=np.uint64)
    one[0] = 1
    check(L.ark_hip_memcpy_h2d(p, one.ctypes.data_as(C.c_void_p), 32), "h2d")
    fid = d.field
    t = rounds({"fr": lambda: check(L.ark_hip_fft_in_place_device(fid, C.byref(d._s), p), "fr fft")}, reps)
    check(L.ark_hip_free(p), "free")
    return t["fr"]


def run_field(f, logs, quick, rng, fr_ms):
    L = lib()
    res = {"field": f.name, "word_bytes": f.bytes, "sizes": []}
    for log_n in logs:
        n = 1 << log_n
        reps = 200 if log_n <= 16 else 50 if log_n <= 20 else 10
        check_transform(f, log_n, rng)
        plain = A.SmallRadix2EvaluationDomain.new(f.name, n)
        coset = plain.get_coset(f.gen)
        v = A.SmallDeviceVec.from_host(f.name, rng.integers(0, f.p, size=n, dtype=np.uint64).astype(dt(f)))
        w = A.SmallDeviceVec(f.name, n)
        pin = C.c_void_p()
        check(L.ark_hip_host_alloc(n * f.bytes, C.byref(pin)), "host_alloc")

        def up_down():
            check(L.ark_hip_memcpy_h2d(w._p, pin, n * f.bytes), "h2d")
            check(L.ark_hip_memcpy_d2h(pin, w._p, n * f.bytes), "d2h")

        t = rounds({
            "d2d": lambda: check(L.ark_hip_memcpy_d2d(w._p, v._p, n * f.bytes), "d2d"),
            "fft": lambda: plain.fft_batch_in_place(v._p, 1),
            "ifft": lambda: plain.fft_batch_in_place(v._p, 1, inverse=True),
            "coset_fft": lambda: coset.fft_batch_in_place(v._p, 1),
            "coset_ifft": lambda: coset.fft_batch_in_place(v._p, 1, inverse=True),
        }, reps)
        t.update(rounds({"upload_download": up_down}, max(2, reps // 10), warm=1))
        check(L.ark_hip_host_free(pin), "host_free")
        passes = len(A.small_fft_plan(f.name, log_n)[3])
        row = {"log_n": log_n, "reps": reps, "rounds": ROUNDS, "passes": passes}
        for k, (med, spread) in t.items():
            row[k + "_ms"], row[k + "_spread_ms"] = med, spread
        row["fr_fft_ms"], row["fr_fft_spread_ms"] = fr_ms[log_n]
        # a pass reads and writes the vector once, as the copy does
        row["times_passes_x_copy"] = {k: round(row[k + "_ms"] / (passes * row["d2d_ms"]), 2) for k in ("fft", "ifft", "coset_fft", "coset_ifft")}
        row["fr_over_small_per_element"] = round(row["fr_fft_ms"] / row["fft_ms"], 2)
        row["faster_per_element_than_fr_beyond_spread"] = bool(row["fr_fft_ms"] - row["fft_ms"] > row["fr_fft_spread_ms"] + row["fft_spread_ms"])
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        v.free()
        w.free()

    # batches: 64 x 2^20, and the 4x low-degree extension of 64 x 2^18
    cols, blog, slog = (8, 14, 12) if quick else (64, 20, 18)
    bn = 1 << blog
    mat = A.SmallDeviceVec.from_host(f.name, rng.integers(0, f.p, size=cols * bn, dtype=np.uint64).astype(dt(f)))
    other = A.SmallDeviceVec(f.name, cols * bn)
    big = A.SmallRadix2EvaluationDomain.new(f.name, bn)
    small = A.SmallRadix2EvaluationDomain.new(f.name, 1 << slog)
    big_coset = big.get_coset(f.gen)
    # check the extension's first column at 4 points: interpolate a sparse polynomial's evaluations, extend, compare
    bm = f.get_coset(f.domain_new(bn), f.gen)
    coeffs = {int(i): int(rng.integers(1, f.p, dtype=np.uint64)) for i in rng.integers(0, 1 << slog, size=64)}
    poly = np.zeros(1 << slog, dtype=dt(f))
    for i, c in coeffs.items():
        poly[i] = c
    col0 = A.SmallDeviceVec.from_host(f.name, poly).evaluate_over_domain(small)
    check(L.ark_hip_memcpy_d2d(mat._p, col0._p, (1 << slog) * f.bytes), "d2d")
    small.fft_batch_in_place(mat._p, cols, stride=bn, inverse=True)
    big_coset.fft_batch_in_place(mat._p, cols, stride=bn, num_coeffs=1 << slog)
    ext = mat.to_host()[:bn]
    for j in [0, bn - 1] + [int(i) for i in rng.integers(0, bn, size=2)]:
        pt = f.from_mont(f.domain_element(bm, j))
        want = sum(f.from_mont(c) * pow(pt, i, f.p) for i, c in coeffs.items()) % f.p
        assert int(ext[j]) == f.to_mont(want), (f.name, "extension", j)

    def lde():
        small.fft_batch_in_place(mat._p, cols, stride=bn, inverse=True)
        big_coset.fft_batch_in_place(mat._p, cols, stride=bn, num_coeffs=1 << slog)

    t = rounds({
        "d2d": lambda: check(L.ark_hip_memcpy_d2d(other._p, mat._p, cols * bn * f.bytes), "d2d"),
        "batch_fft": lambda: big.fft_batch_in_place(mat._p, cols),
        "lde_4x": lde,
    }, 3 if not quick else 20)
    bp = len(A.small_fft_plan(f.name, blog)[3])
    sp = len(A.small_fft_plan(f.name, slog)[3])
    res["batch"] = {"columns": cols, "log_n": blog, "passes": bp, "lde_from_log": slog}
    for k, (med, spread) in t.items():
        res["batch"][k + "_ms"], res["batch"][k + "_spread_ms"] = med, spread
    res["batch"]["batch_fft_times_passes_x_copy"] = round(t["batch_fft"][0] / (bp * t["d2d"][0]), 2)
    # the extension: sp passes over a quarter of the bytes, then bp passes over all of them
    res["batch"]["lde_times_passes_x_copy"] = round(t["lde_4x"][0] / ((bp + sp / 4) * t["d2d"][0]), 2)
    res["batch"]["batch_fft_ms_per_column"] = round(t["batch_fft"][0] / cols, 5)
    print(json.dumps(res["batch"]), flush=True)
    mat.free()
    other.free()

    # pointwise at 2^24
    plog = 14 if quick else 24
    pn = 1 << plog
    ha = rng.integers(0, f.p, size=pn, dtype=np.uint64).astype(dt(f))
    hb = rng.integers(0, f.p, size=pn, dtype=np.uint64).astype(dt(f))
    ha[5] = 0
    a, b, r = A.SmallDeviceVec.from_host(f.name, ha), A.SmallDeviceVec.from_host(f.name, hb), A.SmallDeviceVec(f.name, pn)
    sample = [0, 5, pn - 1] + [int(i) for i in rng.integers(0, pn, size=61)]
    check(L.ark_hip_sfp_mul_device(f.sid, a._p, b._p, r._p, pn), "mul")
    got = r.to_host()
    assert all(int(got[i]) == f.mul(int(ha[i]), int(hb[i])) for i in sample), (f.name, "mul")
    check(L.ark_hip_sfp_inverse_device(f.sid, a._p, r._p, pn), "inverse")
    got = r.to_host()
    assert all(int(got[i]) == f.inv(int(ha[i])) for i in sample), (f.name, "inverse")
    t = rounds({
        "d2d": lambda: check(L.ark_hip_memcpy_d2d(r._p, a._p, pn * f.bytes), "d2d"),
        "mul": lambda: check(L.ark_hip_sfp_mul_device(f.sid, a._p, b._p, r._p, pn), "mul"),
        "inverse": lambda: check(L.ark_hip_sfp_inverse_device(f.sid, a._p, r._p, pn), "inverse"),
    }, 10)
    res["pointwise"] = {"log_n": plog}
    for k, (med, spread) in t.items():
        res["pointwise"][k + "_ms"], res["pointwise"][k + "_spread_ms"] = med, spread
    res["pointwise"]["mul_times_copy_per_byte"] = round(t["mul"][0] / 1.5 / t["d2d"][0], 2)   # three vectors move, the copy moves two
    res["pointwise"]["inverse_times_copy"] = round(t["inverse"][0] / t["d2d"][0], 2)
    print(json.dumps(res["pointwise"]), flush=True)
    for vec in (a, b, r):
        vec.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_fft.json"))
    ap.add_argument("--logs", default="16,20,24")
    ap.add_argument("--quick", action="store_true", help="small batches and vectors: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    logs = [int(x) for x in args.logs.split(",")]
    rng = np.random.default_rng(27)
    out = {"date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; median and spread "
                     "(max - min) of `rounds` interleaved rounds; device-resident data",
           "quick": bool(args.quick), "fields": []}
    fr_ms = {lg: fr_transform_ms(lg, 50 if lg <= 16 else 10 if lg <= 20 else 3) for lg in logs}
    out["fr_fft_ms"] = {str(k): v[0] for k, v in fr_ms.items()}
    print(json.dumps(out["fr_fft_ms"]), flush=True)
    for f in R.FIELDS.values():
        out["fields"].append(run_field(f, logs, args.quick, rng, fr_ms))
    out["accepted"] = all(s["faster_per_element_than_fr_beyond_spread"] for fld in out["fields"] for s in fld["sizes"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out, "accepted:", out["accepted"])


if __name__ == "__main__":
    main()
