"""Times the lookup by value (ark_hip_fr_lookup_device) over BLS12-381 Fr at n = 2^20, 2^22 and 2^24
witness cells against tables of 2^16 and 2^24 values, for section 20's three witness distributions -- uniform over the table,
the witness-like mix (half the cells over the first 256 table values, half uniform) and all cells equal -- next to yardsticks
measured in the same process:

  (a) the floor of the route a caller had: ark_hip_memcpy_d2h of the n values plus ark_hip_memcpy_h2d of n indices through
      pinned memory; the host's hashing is NOT counted;
  (b) ark_hip_fr_count_indices_device on the equivalent index array (the new call does strictly more: a build and a probe);
  (c) ark_hip_memcpy_d2d of the n values.

The call is timed as it ships (indices and counts, asynchronous) and its build phase alone: the same entry with n = 0 and
out_missing, which clears and fills the slots, launches no probe and waits for one word; the probe phase is the difference of
the two medians.  Everything is timed in ROUNDS interleaved rounds; the JSON keeps every round, the median and the spread
(max - min) so that a difference can be held against it.

With --variants DIR every libark_hip*.so in DIR (builds of csrc/field_unit.hip that differ in ARK_LOOKUP_ROUNDS, the rounds of
combining equal cells within a wave in front of the atomic) is loaded into ONE process beside the shipped library and times
the same device vectors at n = 2^24 in the same interleaved rounds, each library on its own context.

Every timed result is checked: the table's values are distinct by construction, so the expected indices are the drawn ones and
the expected counts are numpy's bincount of them; every index and every cell is compared, for every library.

Every size runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_lookup.py [--out profiles/lookup.json] [--logs 20,22,24] [--variants DIR] [--limit 420]
    python tools/bench_lookup.py --one 24                    (one n in this process, its JSON line on stdout)
    python tools/bench_lookup.py --variants DIR --vary 24    (the variants of DIR at one n in this process)
"""
import argparse
import ctypes as C
import datetime
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELD = "BLS12_381_FR"
ROUNDS = 3
TABLE_LOGS = (16, 24)
SETS = ("uniform", "witness_like_mix", "all_equal")


def spread(xs):
    return {"rounds_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4), "spread_ms": round(max(xs) - min(xs), 4)}


def timed(L, fn, reps, warm=2):
    """wall clock per call over `reps` queued calls between two synchronisations of library L's context"""
    for _ in range(warm):
        fn()
    assert L.ark_hip_synchronize() == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    assert L.ark_hip_synchronize() == 0
    return (time.perf_counter() - t0) * 1e3 / reps


def distinct_elements(count, seed):
    """`count` elements below 2^252 (below the modulus), distinct by construction: the second limb is the position"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(12)
    a[:, 1] = np.arange(count, dtype=np.uint64)
    return a


def index_sets(n, table_len, rng):
    return {"uniform": rng.integers(0, table_len, size=n, dtype=np.uint32),
            "witness_like_mix": np.where(rng.random(n) < 0.5, rng.integers(0, 256, size=n), rng.integers(0, table_len, size=n)).astype(np.uint32),
            "all_equal": np.full(n, table_len // 3, dtype=np.uint32)}


def bind(path):
    """another build of the library beside the shipped one: its own context, the same device memory"""
    from algebra_amd import _lib
    L = C.CDLL(path)
    for name in ("ark_hip_fr_lookup_device", "ark_hip_synchronize"):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SYMBOLS[name]
    return L


class Bench:
    def __init__(self, log_n):
        import algebra_amd as A
        from algebra_amd import curves as cv
        from algebra_amd._lib import check, lib
        self.A, self.L, self.check = A, lib(), check
        self.n = 1 << log_n
        self.P = cv.SCALAR_MODULUS[FIELD]
        self.R = (1 << 256) % self.P
        self.reps = 10 if log_n <= 20 else 5 if log_n <= 22 else 3
        self.d_idx, self.d_out_idx = C.c_void_p(), C.c_void_p()
        check(self.L.ark_hip_malloc(self.n * 4, C.byref(self.d_idx)), "malloc")
        check(self.L.ark_hip_malloc(self.n * 4, C.byref(self.d_out_idx)), "malloc")
        self.values = A.DeviceVec(FIELD, self.n, _zero=False)
        self.field = self.values.field

    def mont_counts(self, want):
        """the Montgomery elements of an array of counts, through its few distinct values"""
        uniq, inv = np.unique(want, return_inverse=True)
        el = np.frombuffer(b"".join((int(c) * self.R % self.P).to_bytes(32, "little") for c in uniq), dtype="<u8").reshape(-1, 4)
        return el.astype(np.uint64)[inv]

    def lookup(self, L, table, table_len, mult, n=None, missing=None):
        n = self.n if n is None else n
        rc = L.ark_hip_fr_lookup_device(self.field, table.ptr, table_len, self.values.ptr if n else None, n,
                                        self.d_out_idx if n else None, mult.ptr if n else None, missing)
        assert rc == 0, rc

    def upload(self, ta, idx):
        va = ta[idx]
        self.check(self.L.ark_hip_memcpy_h2d(self.values.ptr, va.ctypes.data_as(C.c_void_p), va.nbytes), "h2d")
        self.check(self.L.ark_hip_memcpy_h2d(self.d_idx, idx.ctypes.data_as(C.c_void_p), idx.nbytes), "h2d")
        self.check(self.L.ark_hip_synchronize(), "sync")   # another library's context may read them next

    def verify(self, L, table, table_len, mult, idx, tag):
        """one call of library L into poisoned outputs: every index and every count"""
        check, M = self.check, self.L
        check(M.ark_hip_memset_device(mult.ptr, 0xAB, table_len * 32), "memset")
        check(M.ark_hip_memset_device(self.d_out_idx, 0xAB, self.n * 4), "memset")
        check(M.ark_hip_synchronize(), "sync")
        missing = C.c_uint64(99)
        self.lookup(L, table, table_len, mult, missing=C.byref(missing))
        got = np.empty(self.n, dtype=np.uint32)
        check(M.ark_hip_memcpy_d2h(got.ctypes.data_as(C.c_void_p), self.d_out_idx, got.nbytes), "d2h")
        assert missing.value == 0 and np.array_equal(got, idx), (tag, "indices")
        want = np.bincount(idx, minlength=table_len)
        assert int(want.sum()) == self.n
        assert np.array_equal(mult.to_host(), self.mont_counts(want)), (tag, "counts")

    def free(self):
        self.check(self.L.ark_hip_free(self.d_idx), "free")
        self.check(self.L.ark_hip_free(self.d_out_idx), "free")
        self.values.free()


def run(log_n):
    B = Bench(log_n)
    A, L, check, n, reps = B.A, B.L, B.check, B.n, B.reps
    res = {"log_n": log_n, "n": n, "reps": reps, "rounds": ROUNDS, "tables": []}
    copy = A.DeviceVec(FIELD, n, _zero=False)
    pinned = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")

    def host_route():
        check(L.ark_hip_memcpy_d2h(pinned, B.values.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(B.d_idx, pinned, n * 4), "h2d")
    floors = {"d2h_values_h2d_indices": [], "d2d_values": []}
    rng = np.random.default_rng(2600 + log_n)
    for table_log in TABLE_LOGS:
        table_len = 1 << table_log
        ta = distinct_elements(table_len, 100 + table_log)
        table = A.DeviceVec.from_host(FIELD, ta)
        mult = A.DeviceVec(FIELD, table_len, _zero=False)
        sets = index_sets(n, table_len, rng)
        case = {"table_len": table_len, "plan": dict(zip(("capacity_log", "scratch_bytes"), A.lookup_plan(table_len)))}
        t = {(k, s): [] for k in ("lookup", "count_indices") for s in SETS}
        build = []
        miss = C.c_uint64()
        for _ in range(ROUNDS):                            # interleaved, so that drift hits all alike
            for name in SETS:
                B.upload(ta, sets[name])
                t["lookup", name].append(timed(L, lambda: B.lookup(L, table, table_len, mult), reps))
                t["count_indices", name].append(timed(L, lambda: check(L.ark_hip_fr_count_indices_device(B.field, B.d_idx, n, mult.ptr, table_len), "count"), reps))
            build.append(timed(L, lambda: B.lookup(L, table, table_len, mult, n=0, missing=C.byref(miss)), reps))
            floors["d2d_values"].append(timed(L, lambda: check(L.ark_hip_memcpy_d2d(copy.ptr, B.values.ptr, n * 32), "d2d"), reps))
            floors["d2h_values_h2d_indices"].append(timed(L, host_route, max(2, reps // 2), warm=1))
        for name in SETS:
            B.upload(ta, sets[name])
            B.verify(L, table, table_len, mult, sets[name], (log_n, table_log, name))
            case[name] = {"lookup": spread(t["lookup", name]), "count_indices": spread(t["count_indices", name])}
            a, b = case[name]["lookup"], case[name]["count_indices"]
            case[name]["lookup_over_count_indices"] = round(a["median_ms"] / b["median_ms"], 3)
            case[name]["lookup_faster_by_more_than_both_spreads"] = bool(b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"])
        case["build_alone_n0_waits"] = spread(build)
        for name in SETS:
            case[name]["probe_by_difference_ms"] = round(case[name]["lookup"]["median_ms"] - case["build_alone_n0_waits"]["median_ms"], 4)
        res["tables"].append(case)
        table.free()
        mult.free()
    res["floors"] = {k: spread(v) for k, v in floors.items()}
    check(L.ark_hip_host_free(pinned), "host_free")
    copy.free()
    B.free()
    return res


def vary(log_n, directory):
    """the shipped library and every build of `directory` in one process, interleaved"""
    B = Bench(log_n)
    A, n, reps = B.A, B.n, B.reps
    libs = {"shipped": B.L}
    for path in sorted(glob.glob(os.path.join(directory, "libark_hip*.so"))):
        libs[os.path.basename(path)] = bind(os.path.abspath(path))
    res = {"log_n": log_n, "n": n, "reps": reps, "rounds": ROUNDS, "tables": []}
    rng = np.random.default_rng(2700 + log_n)
    for table_log in TABLE_LOGS:
        table_len = 1 << table_log
        ta = distinct_elements(table_len, 100 + table_log)
        table = A.DeviceVec.from_host(FIELD, ta)
        mult = A.DeviceVec(FIELD, table_len, _zero=False)
        sets = index_sets(n, table_len, rng)
        t = {(k, s): [] for k in libs for s in SETS}
        for _ in range(ROUNDS):
            for name in SETS:
                B.upload(ta, sets[name])
                for k, L in libs.items():
                    t[k, name].append(timed(L, lambda: B.lookup(L, table, table_len, mult), reps))
        for name in SETS:
            B.upload(ta, sets[name])
            for k, L in libs.items():
                B.verify(L, table, table_len, mult, sets[name], (k, table_log, name))
        res["tables"].append({"table_len": table_len, "variants": {k: {s: spread(t[k, s]) for s in SETS} for k in libs}})
        table.free()
        mult.free()
    B.free()
    return res


def child(args, limit):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        print(out.stdout[-4000:] + out.stderr[-4000:])
        return None, out.returncode
    return json.loads(line[-1][len("RESULT "):]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--variants", default=None, help="a directory of libark_hip*.so builds that differ in ARK_LOOKUP_ROUNDS")
    ap.add_argument("--limit", type=int, default=420, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None)
    ap.add_argument("--vary", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    if args.vary is not None:
        print("RESULT " + json.dumps(vary(args.vary, args.variants)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up, in `rounds` "
                     "interleaved rounds; spread = max - min; the lookup writes indices and counts and is asynchronous; the build phase "
                     "alone is the entry with n = 0 and out_missing (it waits for one word)",
           "sizes": []}
    for lg in (int(x) for x in args.logs.split(",")):
        # a fresh process per size under its own time limit; a failure ends the run: nothing more is started on the GPU
        r, rc = child(["--one", str(lg)], args.limit)
        if r is None:
            print("n = 2^%d failed with status %d: stopping" % (lg, rc))
            return 1
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    if args.variants:
        v, rc = child(["--variants", args.variants, "--vary", "24"], args.limit)
        if v is None:
            print("the variants failed with status %d: stopping" % rc)
            return 1
        out["combine_rounds_variants"] = v
        print(json.dumps(v), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
