"""Times the polynomial operations on device-resident vectors (evaluate, divide by x - z, divide by the vanishing polynomial,
Lagrange coefficients, inner product) at 2^20, 2^22 and 2^24 coefficients over BLS12-381 Fr, next to two yardsticks measured
in the same run:

  (a) ark_hip_memcpy_d2d of the same vector: what moving n * 32 bytes in and out of HBM costs;
  (b) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d of the vector through pinned host memory: the cheapest conceivable form of the
      only route there was before these entries (download, host arithmetic -- not even counted --, upload).

Every timed result is checked against Python big integers at sampled indices.  The vectors are a random block of L = 2^16 - 1
coefficients repeated (an odd period: it never lines up with a tile), which gives every suffix sum a closed form.

Timing: the library runs on a stream of its own and exposes no events, so -- like the other tools here -- a call is timed
by the wall clock around `reps` queued calls bracketed by ark_hip_synchronize(), after warm-up calls.  For the asynchronous
entries (divide without a remainder, vanishing, Lagrange, the d2d copy) that is the device time per call once the queue is
full.  The entries that return a value to the host (evaluate, inner product, divide with a remainder) wait inside every
call: their rows are HOST-OBSERVED LATENCY -- kernels plus one 32-byte download and its wait -- and are labelled so in the
JSON ("host_observed"); the kernels' own times come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats).
The vanishing division is timed at two ratios, m = n / 4 (a prover's) and m = n / 64, and once at 2^24 for m = 2^10, the
corner its m-lane parallelism is not made for.

    python tools/bench_poly_ops.py [--out profiles/poly_ops.json] [--logs 20,22,24]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import algebra_amd as A  # noqa: E402
from algebra_amd import curves as cv  # noqa: E402
from algebra_amd._lib import check, lib  # noqa: E402

FIELD = "BLS12_381_FR"
P = cv.SCALAR_MODULUS[FIELD]
R = (1 << 256) % P
RINV = pow(R, -1, P)
L_BLOCK = (1 << 16) - 1


def limbs(xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def one(x):
    return limbs([x])[0]


def periodic(block, n):
    """device vector of n elements: block repeated (doubling device-to-device copies)"""
    v = A.DeviceVec(FIELD, n, _zero=False)
    Lb = len(block)
    first = min(Lb, n)
    host = limbs(block[:first])
    check(lib().ark_hip_memcpy_h2d(v.ptr, host.ctypes.data_as(C.c_void_p), host.nbytes), "h2d")
    cur = first
    while cur < n:
        cnt = min(cur, n - cur)
        check(lib().ark_hip_memcpy_d2d(C.c_void_p(v.ptr.value + cur * 32), v.ptr, cnt * 32), "d2d")
        cur += cnt
    check(lib().ark_hip_synchronize(), "sync")
    return v


class Suffix:
    """S(i) = sum_{j >= i} p[j] z^(j - i) for p[j] = block[j mod L], j < n, in closed form (residues as integers, canonical z)"""

    def __init__(self, block, n, z):
        Lb = len(block)
        self.block, self.n, self.z, self.L = block, n, z, Lb
        self.K, self.rem = divmod(n, Lb)
        self.suf = [0] * (Lb + 1)                      # suf[e] = sum_{f >= e} block[f] z^(f - e)
        for e in range(Lb - 1, -1, -1):
            self.suf[e] = (block[e] + z * self.suf[e + 1]) % P
        self.pre = [0] * (Lb + 1)                      # pre[e] = sum_{f < e} block[f] z^f
        zp = 1
        for e in range(Lb):
            self.pre[e + 1] = (self.pre[e] + block[e] * zp) % P
            zp = zp * z % P
        self.zL = pow(z, Lb, P)

    def geo(self, f):                                  # sum_{t < f} z^(L t)
        if self.zL == 1:
            return f % P
        return (pow(self.zL, f, P) - 1) * pow(self.zL - 1, -1, P) % P

    def at(self, i):
        if i >= self.n:
            return 0
        k, e0 = divmod(i, self.L)
        if k == self.K:                                # inside the ragged last block
            return (self.pre[self.rem] - self.pre[e0]) * pow(pow(self.z, e0, P), -1, P) % P if self.z else (self.block[e0] if e0 < self.rem else 0)
        full = self.K - 1 - k
        rest = (self.suf[0] * self.geo(full) + pow(self.zL, full, P) * self.pre[self.rem]) % P
        return (self.suf[e0] + pow(self.z, self.L - e0, P) * rest) % P


def timed(fn, reps, warm=2):
    L = lib()
    for _ in range(warm):
        fn()
    check(L.ark_hip_synchronize(), "sync")
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    check(L.ark_hip_synchronize(), "sync")
    return (time.perf_counter() - t0) * 1e3 / reps


def rows(v, idx):
    """elements idx of a device vector (small downloads)"""
    out = np.zeros((len(idx), 4), dtype=np.uint64)
    for k, i in enumerate(idx):
        check(lib().ark_hip_memcpy_d2h(out[k].ctypes.data_as(C.c_void_p), C.c_void_p(v.ptr.value + int(i) * 32), 32), "d2h")
    return out


def run(log_n, rng):
    L = lib()
    n = 1 << log_n
    reps = 20 if log_n <= 20 else 10 if log_n <= 22 else 5
    block = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(L_BLOCK)]
    block2 = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(L_BLOCK)]
    z = int.from_bytes(rng.bytes(40), "little") % P
    tau = int.from_bytes(rng.bytes(40), "little") % P
    zM, tauM = one(z * R % P), one(tau * R % P)
    p, b = periodic(block, n), periodic(block2, n)
    sample = sorted({0, 1, 2047, 2048, 2049, n // 2, n - 3, n - 2} | {int(v) for v in rng.integers(0, n - 1, size=24)})
    res = {"n": n, "reps": reps, "checked_indices": len(sample)}
    S = Suffix(block, n, z)

    # yardsticks
    other = A.DeviceVec(FIELD, n, _zero=False)
    res["d2d_ms"] = timed(lambda: check(L.ark_hip_memcpy_d2d(other.ptr, p.ptr, n * 32), "d2d"), reps)
    pinned = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")

    def round_trip():
        check(L.ark_hip_memcpy_d2h(pinned, p.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(other.ptr, pinned, n * 32), "h2d")
    res["d2h_h2d_ms"] = timed(round_trip, max(3, reps // 2), warm=1)
    check(L.ark_hip_host_free(pinned), "host_free")

    # evaluate
    res["evaluate_ms"] = timed(lambda: p.evaluate(zM), reps)
    assert np.array_equal(p.evaluate(zM), one(S.at(0))), "evaluate"

    # divide by x - z: out of place with the remainder (waits), and the asynchronous in-place form of a prover
    q = A.DeviceVec(FIELD, n - 1, _zero=False)
    rem = np.zeros(4, dtype=np.uint64)

    def divide():
        check(L.ark_hip_poly_divide_linear_device(p.field, p.ptr, n, zM.ctypes.data_as(C.c_void_p), q.ptr, rem.ctypes.data_as(C.c_void_p)), "divide")
    res["divide_linear_ms"] = timed(divide, reps)
    assert np.array_equal(rem, one(S.at(0))), "remainder"
    assert np.array_equal(rows(q, sample), limbs([S.at(i + 1) for i in sample])), "quotient"
    res["divide_linear_async_ms"] = timed(lambda: check(L.ark_hip_poly_divide_linear_device(
        p.field, p.ptr, n, zM.ctypes.data_as(C.c_void_p), q.ptr, None), "divide"), reps)
    q.free()

    # divide by x^m - 1, m = n / 4
    m = n // 4
    vq, vr = A.DeviceVec(FIELD, n - m, _zero=False), A.DeviceVec(FIELD, m, _zero=False)
    res["vanishing_ms"] = timed(lambda: check(L.ark_hip_poly_divide_by_vanishing_device(p.field, m, p.ptr, n, vq.ptr, vr.ptr), "vanishing"), reps)
    qs = [j for j in sample if j < n - m]
    want_q = [sum(block[(j + i * m) % L_BLOCK] for i in range(1, (n - 1 - j) // m + 1)) % P for j in qs]
    assert np.array_equal(rows(vq, qs), limbs(want_q)), "vanishing quotient"
    rs = [j for j in sample if j < m]
    want_r = [sum(block[(j + i * m) % L_BLOCK] for i in range(0, (n - 1 - j) // m + 1)) % P for j in rs]
    assert np.array_equal(rows(vr, rs), limbs(want_r)), "vanishing remainder"
    vq.free()
    vr.free()
    for label, m2, r2 in [("vanishing_m64", n // 64, reps)] + ([("vanishing_m1024", 1 << 10, 1)] if log_n == 24 else []):
        vq, vr = A.DeviceVec(FIELD, n - m2, _zero=False), A.DeviceVec(FIELD, m2, _zero=False)
        res[label + "_ms"] = timed(lambda: check(L.ark_hip_poly_divide_by_vanishing_device(p.field, m2, p.ptr, n, vq.ptr, vr.ptr), "vanishing"),
                                   r2, warm=1)
        rs = [j for j in sample if j < m2]
        want_r = [sum(block[(j + i * m2) % L_BLOCK] for i in range(0, (n - 1 - j) // m2 + 1)) % P for j in rs]
        assert np.array_equal(rows(vr, rs), limbs(want_r)), label
        vq.free()
        vr.free()

    # Lagrange coefficients of the size-n domain at tau
    dom = A.Radix2EvaluationDomain.new(FIELD, n)
    lag = A.DeviceVec(FIELD, n, _zero=False)
    res["lagrange_ms"] = timed(lambda: check(L.ark_hip_domain_lagrange_coefficients_device(
        p.field, C.byref(dom._s), tauM.ctypes.data_as(C.c_void_p), lag.ptr), "lagrange"), reps)
    g = sum(int(v) << (64 * i) for i, v in enumerate(dom.group_gen())) * RINV % P
    zh = (pow(tau, n, P) - 1) % P
    want_l = [zh * pow(g, i, P) % P * pow(n * (tau - pow(g, i, P)) % P, -1, P) % P * R % P for i in sample]
    assert np.array_equal(rows(lag, sample), limbs(want_l)), "lagrange"
    lag.free()

    # inner product
    res["inner_product_ms"] = timed(lambda: p.inner_product(b), reps)
    K, rem_b = divmod(n, L_BLOCK)
    full = sum(x * y for x, y in zip(block, block2))
    part = sum(x * y for x, y in zip(block[:rem_b], block2[:rem_b]))
    assert np.array_equal(p.inner_product(b), one((K * full + part) * RINV % P)), "inner product"

    # per byte that must move, as a multiple of the device-to-device copy (which moves 2 n 32 bytes)
    per_byte = res["d2d_ms"] / (2 * n * 32)
    moved = {"evaluate": 1, "divide_linear": 3, "divide_linear_async": 3, "vanishing": 2, "vanishing_m64": 2, "lagrange": 1,
             "inner_product": 2}
    if "vanishing_m1024_ms" in res:
        moved["vanishing_m1024"] = 2
    res["host_observed"] = ["evaluate", "divide_linear", "inner_product"]
    res["times_d2d_per_byte"] = {k: round(res[k + "_ms"] / (f * n * 32) / per_byte, 2) for k, f in moved.items()}
    res["faster_than_d2h_h2d"] = {k: bool(res[k + "_ms"] < res["d2h_h2d_ms"]) for k in moved}
    for v in (p, b, other):
        v.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_ops.json"))
    ap.add_argument("--logs", default="20,22,24")
    args = ap.parse_args()
    rng = np.random.default_rng(11)
    out = {"field": FIELD, "date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up",
           "sizes": []}
    for lg in (int(x) for x in args.logs.split(",")):
        r = run(lg, rng)
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    out["accepted"] = all(all(s["faster_than_d2h_h2d"].values()) for s in out["sizes"])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
