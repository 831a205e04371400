"""Times the prefix scans on device-resident vectors (prefix product, prefix sum, the ratio accumulator) at 2^20, 2^22 and
2^24 elements over BLS12-381 Fr, synchronous (the total comes back to the host) and asynchronous (NULL for it), next to three
yardsticks measured in the same run:

  (a) ark_hip_memcpy_d2d of one vector: what moving n * 32 bytes in and out of HBM costs;
  (b) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d through pinned host memory of the vectors an entry takes and gives (one down
      and one up for the product and the sum, two down and one up for the ratio): the cheapest conceivable form of the only
      route there was before these entries (download, a serial host loop -- not even counted --, upload);
  (c) for the ratio only, the composed route these entries allow: two exclusive ark_hip_fr_prefix_product_device calls and
      one ark_hip_fr_div_device (one inversion per eight elements instead of one per tile, two temporaries of length n).

Every timed result is checked against Python big integers at 32 sampled indices.  The vectors are a random block of
L = 2^16 - 1 elements repeated (an odd period: it never lines up with a tile), which gives every prefix a closed form:
prefix(i) = total(block)^(i div L) (op) prefix_of_block(i mod L).

Timing: as tools/bench_poly_ops.py -- the wall clock around `reps` queued calls bracketed by ark_hip_synchronize(), after
warm-up calls -- repeated ROUNDS times with the variants interleaved; the JSON keeps the median and the spread (max - min) of
the rounds.  For the asynchronous forms that is the device time per call once the queue is full; the synchronous forms wait
inside every call and are HOST-OBSERVED LATENCY (kernels plus one 32-byte download and its wait).

    python tools/bench_prefix_scan.py [--out profiles/prefix_scan.json] [--logs 20,22,24]
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
from tools.bench_poly_ops import limbs, one, periodic, rows  # noqa: E402

FIELD = "BLS12_381_FR"
P = cv.SCALAR_MODULUS[FIELD]
R = (1 << 256) % P
RINV = pow(R, -1, P)
L_BLOCK = (1 << 16) - 1
ROUNDS = 5


class Periodic:
    """closed forms of the prefixes of v[j] = block[j mod L] (stored residues as integers; products on canonical values)"""

    def __init__(self, block):
        self.L = len(block)
        canon = [x * RINV % P for x in block]
        self.ppre, self.spre = [1] * (self.L + 1), [0] * (self.L + 1)      # of the first e elements of the block
        for e in range(self.L):
            self.ppre[e + 1] = self.ppre[e] * canon[e] % P
            self.spre[e + 1] = (self.spre[e] + block[e]) % P

    def product(self, count):
        """canonical product of the first `count` elements"""
        k, e = divmod(count, self.L)
        return pow(self.ppre[self.L], k, P) * self.ppre[e] % P

    def sum(self, count):
        """stored sum of the first `count` elements"""
        k, e = divmod(count, self.L)
        return (k * self.spre[self.L] + self.spre[e]) % P


def rounds(variants, reps, warm=2):
    """{name: [ms per call, one entry per round]} with the variants interleaved inside every round"""
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
    return out


def run(log_n, rng):
    L = lib()
    n = 1 << log_n
    reps = 20 if log_n <= 20 else 10 if log_n <= 22 else 5
    blk_a = [int.from_bytes(rng.bytes(40), "little") % (P - 1) + 1 for _ in range(L_BLOCK)]      # no zeros: a zero would make every check trivial
    blk_b = [int.from_bytes(rng.bytes(40), "little") % (P - 1) + 1 for _ in range(L_BLOCK)]
    a, b = periodic(blk_a, n), periodic(blk_b, n)
    pa, pb = Periodic(blk_a), Periodic(blk_b)
    sample = {0, 1, 2047, 2048, 2049, n // 2, n - 2, n - 1}
    while len(sample) < 32:
        sample.add(int(rng.integers(0, n)))
    sample = sorted(sample)
    fid = a.field
    out = A.DeviceVec(FIELD, n, _zero=False)
    t1, t2 = A.DeviceVec(FIELD, n, _zero=False), A.DeviceVec(FIELD, n, _zero=False)
    host = np.zeros(4, dtype=np.uint64)
    hp = host.ctypes.data_as(C.c_void_p)
    pin = [C.c_void_p() for _ in range(2)]
    for q in pin:
        check(L.ark_hip_host_alloc(n * 32, C.byref(q)), "host_alloc")

    def round_trip_1():
        check(L.ark_hip_memcpy_d2h(pin[0], a.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(out.ptr, pin[0], n * 32), "h2d")

    def round_trip_ratio():
        check(L.ark_hip_memcpy_d2h(pin[0], a.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_d2h(pin[1], b.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(out.ptr, pin[0], n * 32), "h2d")

    def composed():
        check(L.ark_hip_fr_prefix_product_device(fid, a.ptr, n, 1, t1.ptr, None), "product")
        check(L.ark_hip_fr_prefix_product_device(fid, b.ptr, n, 1, t2.ptr, None), "product")
        check(L.ark_hip_fr_div_device(fid, t1.ptr, t2.ptr, out.ptr, n), "div")

    want_ratio = limbs([pa.product(i) * pow(pb.product(i), -1, P) % P * R % P for i in sample])
    want_last = one(pa.product(n) * pow(pb.product(n), -1, P) % P * R % P)
    res = {"n": n, "reps": reps, "rounds": ROUNDS, "checked_indices": len(sample)}

    # every result first, checked; then the clock
    check(L.ark_hip_fr_prefix_product_device(fid, a.ptr, n, 0, out.ptr, hp), "product")
    assert np.array_equal(rows(out, sample), limbs([pa.product(i + 1) * R % P for i in sample])), "product"
    assert np.array_equal(host, one(pa.product(n) * R % P)), "product total"
    check(L.ark_hip_fr_prefix_product_device(fid, a.ptr, n, 1, out.ptr, None), "product")
    assert np.array_equal(rows(out, sample), limbs([pa.product(i) * R % P for i in sample])), "exclusive product (asynchronous)"
    check(L.ark_hip_fr_prefix_sum_device(fid, a.ptr, n, 0, out.ptr, hp), "sum")
    assert np.array_equal(rows(out, sample), limbs([pa.sum(i + 1) for i in sample])), "sum"
    assert np.array_equal(host, one(pa.sum(n))), "sum total"
    check(L.ark_hip_fr_prefix_sum_device(fid, a.ptr, n, 1, out.ptr, None), "sum")
    assert np.array_equal(rows(out, sample), limbs([pa.sum(i) for i in sample])), "exclusive sum (asynchronous)"
    check(L.ark_hip_fr_prefix_ratio_device(fid, a.ptr, b.ptr, n, out.ptr, hp), "ratio")
    assert np.array_equal(rows(out, sample), want_ratio), "ratio"
    assert np.array_equal(host, want_last), "ratio last"
    check(L.ark_hip_memset_device(out.ptr, 0, n * 32), "memset")
    check(L.ark_hip_fr_prefix_ratio_device(fid, a.ptr, b.ptr, n, out.ptr, None), "ratio")
    assert np.array_equal(rows(out, sample), want_ratio), "ratio (asynchronous)"
    check(L.ark_hip_memset_device(out.ptr, 0, n * 32), "memset")
    composed()
    assert np.array_equal(rows(out, sample), want_ratio), "the composed route"

    variants = {
        "d2d": lambda: check(L.ark_hip_memcpy_d2d(out.ptr, a.ptr, n * 32), "d2d"),
        "product": lambda: check(L.ark_hip_fr_prefix_product_device(fid, a.ptr, n, 0, out.ptr, hp), "product"),
        "product_async": lambda: check(L.ark_hip_fr_prefix_product_device(fid, a.ptr, n, 0, out.ptr, None), "product"),
        "sum": lambda: check(L.ark_hip_fr_prefix_sum_device(fid, a.ptr, n, 0, out.ptr, hp), "sum"),
        "sum_async": lambda: check(L.ark_hip_fr_prefix_sum_device(fid, a.ptr, n, 0, out.ptr, None), "sum"),
        "ratio": lambda: check(L.ark_hip_fr_prefix_ratio_device(fid, a.ptr, b.ptr, n, out.ptr, hp), "ratio"),
        "ratio_async": lambda: check(L.ark_hip_fr_prefix_ratio_device(fid, a.ptr, b.ptr, n, out.ptr, None), "ratio"),
        "ratio_composed": composed,
    }
    t = rounds(variants, reps)
    t.update(rounds({"d2h_h2d": round_trip_1, "d2h_h2d_ratio": round_trip_ratio}, max(2, reps // 4), warm=1))
    for k, v in t.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_spread_ms"] = round(max(v) - min(v), 4)
    for q in pin:
        check(L.ark_hip_host_free(q), "host_free")

    # per byte that must move, as a multiple of the device-to-device copy (which moves 2 n 32 bytes): the product and the sum
    # read the vector twice (totals, then the scan) and write it once, the ratio reads two vectors twice and writes one
    per_byte = res["d2d_ms"] / (2 * n * 32)
    moved = {"product": 3, "product_async": 3, "sum": 3, "sum_async": 3, "ratio": 5, "ratio_async": 5, "ratio_composed": 11}
    res["host_observed"] = ["product", "sum", "ratio"]
    res["times_d2d_per_byte"] = {k: round(res[k + "_ms"] / (f * n * 32) / per_byte, 2) for k, f in moved.items()}
    res["faster_than_d2h_h2d"] = {k: bool(res[k + "_ms"] < res["d2h_h2d_ratio_ms" if k.startswith("ratio") else "d2h_h2d_ms"])
                                  for k in moved if k != "ratio_composed"}
    gain = res["ratio_composed_ms"] - res["ratio_async_ms"]
    res["ratio_vs_composed"] = {"composed_over_ratio": round(res["ratio_composed_ms"] / res["ratio_async_ms"], 2),
                                "gain_ms": round(gain, 4),
                                "beats_composed_beyond_spread": bool(gain > res["ratio_composed_spread_ms"] + res["ratio_async_spread_ms"])}
    for v in (a, b, out, t1, t2):
        v.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_scan.json"))
    ap.add_argument("--logs", default="20,22,24")
    args = ap.parse_args()
    rng = np.random.default_rng(22)
    out = {"field": FIELD, "date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; median and "
                     "spread (max - min) of `rounds` interleaved rounds",
           "sizes": []}
    for lg in (int(x) for x in args.logs.split(",")):
        r = run(lg, rng)
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    out["accepted"] = all(all(s["faster_than_d2h_h2d"].values()) and s["ratio_vs_composed"]["beats_composed_beyond_spread"]
                          for s in out["sizes"])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
