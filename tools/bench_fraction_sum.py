"""Times the fractional-sum entries over BLS12-381 Fr, next to the routes they replace and to yardsticks
measured in the same run:

  tree       ark_hip_mle_fraction_tree_device (asynchronous) with numerators and with ones, at nu = 20, 22 and 24, against
             (a) the route a caller had: per level three ark_hip_fr_mul_device, one ark_hip_fr_add_device and a temporary on
                 half-level views, into the same tree buffers (with ones the first level is one add and one product);
             (b) ark_hip_memcpy_d2d of the two input tables: the byte floor;
             (c) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d of the two tables through pinned memory: the floor of a host prover.
             With --variants DIR every libark_hip*.so in DIR (builds that differ in ARK_FRAC_TREE_W of csrc/fraction_sum.cuh:
             1, 2 or 3 levels per launch) times the same trees in a process of its own.
  counts     ark_hip_fr_count_indices_device at n = 2^24 into table_len = 2^16 and 2^24 for three index sets -- uniform, all
             equal, and a witness-like mix (half the indices uniform over the first 256 cells, as the small values of a range
             check, half uniform over the table) -- against ark_hip_memcpy_d2d of the index array.
  proof      FractionalSum.prove's steps, host-observed (every round waits for its evaluations, as in section 17), split into
             the trees, the eq tables, the sumcheck rounds of the layers of at least SMALL variables and the layers below.

The trees and their baseline are timed in ROUNDS interleaved rounds; the JSON keeps every round, the median, and the spread
(max - min) so that a difference can be held against it.

Every timed result is checked.  A table is a base block of 2^12 random elements repeated, with planted cells; the levels of
both trees are modelled on Python integers as a base block and the cells the planted ones reach (0 is not planted: a zero
denominator would hide every denominator above it), and walked in full below 2^12; sampled rows of every level are compared.
The counts are compared with numpy's bincount (every cell of 2^16, sampled cells and the sum of 2^24).  The proof is checked
by a verifier written out here and its last claims against evaluate on the device.

Every size runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_fraction_sum.py [--out profiles/fraction_sum.json] [--logs 20,22,24] [--variants DIR] [--limit 300]
    python tools/bench_fraction_sum.py --one 24          (one size in this process, its JSON line on stdout)
    python tools/bench_fraction_sum.py --tree 24         (the trees alone, for a variant named by ARK_HIP_LIB)
    python tools/bench_fraction_sum.py --counts 24       (the counts alone: n = 2^24)
"""
import argparse
import ctypes as C
import datetime
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mle_ops import FIELD, LO, ints, limbs, timed   # noqa: E402

SMALL = 12        # layers of fewer variables count as the launch-bound tail of the proof
ROUNDS = 3


def spread(xs):
    return {"rounds_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4), "spread_ms": round(max(xs) - min(xs), 4)}


class Periodic:
    """2^k values: base[i mod len(base)] except at the planted cells"""

    def __init__(self, k, base, cells):
        self.k, self.base, self.cells = k, base, cells

    def at(self, i):
        v = self.cells.get(i)
        return self.base[i % len(self.base)] if v is None else v


class Setup:
    """the two tables on the device and their trees on integers"""

    def __init__(self, nu):
        import algebra_amd as A
        from algebra_amd import curves as cv
        self.A, self.nu, self.n = A, nu, 1 << nu
        self.P = cv.SCALAR_MODULUS[FIELD]
        self.R = (1 << 256) % self.P
        rng = np.random.default_rng(400 + nu)
        self.rng = rng
        rnd = lambda: int.from_bytes(rng.bytes(40), "little") % self.P or 1   # noqa: E731
        self.rnd = rnd
        n = self.n
        self.tables = {}
        for name in ("num", "den"):
            base = [rnd() for _ in range(1 << LO)]                             # canonical values
            cells = {i: v for i, v in ((1, 1), (2, self.P - 1), (n - 1, rnd()), (n // 2, rnd()), (n // 2 - 1, rnd()),
                                       (n - 1 - (1 << LO), rnd()))}
            a = np.tile(limbs([x * self.R % self.P for x in base]), (n >> LO, 1))
            for i, v in cells.items():
                a[i] = limbs([v * self.R % self.P])[0]
            self.tables[name] = (Periodic(nu, base, cells), a, A.DenseMultilinearExtension.from_evaluations(FIELD, nu, a))
        self.num, self.den = self.tables["num"][2], self.tables["den"][2]

    def level_models(self, has_num):
        """[(k, N_k, D_k)] for k = nu - 1 .. 0 as Periodic tables on canonical integers"""
        P, nu = self.P, self.nu
        N = self.tables["num"][0] if has_num else Periodic(nu, [1] * (1 << LO), {})
        D = self.tables["den"][0]
        out = []
        for k in range(nu - 1, -1, -1):
            h = 1 << k

            def pair(i, N=N, D=D, h=h):
                n0, n1, d0, d1 = N.at(i), N.at(i + h), D.at(i), D.at(i + h)
                return (n0 * d1 + n1 * d0) % P, d0 * d1 % P
            if k >= LO:                                # a base element pairs with itself, a cell with what lies h away
                both = [((2 * a * b) % P, b * b % P) for a, b in zip(N.base, D.base)]
                cells = {o: pair(o) for o in {i % h for i in list(N.cells) + list(D.cells)}}
                N = Periodic(k, [x for x, _ in both], {o: v[0] for o, v in cells.items()})
                D = Periodic(k, [y for _, y in both], {o: v[1] for o, v in cells.items()})
            else:                                      # in full
                both = [pair(i) for i in range(h)]
                N, D = Periodic(k, [x for x, _ in both], {}), Periodic(k, [y for _, y in both], {})
            out.append((k, N, D))
        return out

    def check_trees(self, ntree_ptr, dtree_ptr, has_num, tag):
        from algebra_amd._lib import check, lib
        L, n, P, R = lib(), self.n, self.P, self.R

        def rows(ptr, idx):
            out = np.zeros((len(idx), 4), dtype=np.uint64)
            for q, i in enumerate(idx):
                check(L.ark_hip_memcpy_d2h(out[q].ctypes.data_as(C.c_void_p), C.c_void_p(ptr.value + int(i) * 32), 32), "d2h")
            return out
        root = None
        for k, N, D in self.level_models(has_num):
            size, off = 1 << k, n - (2 << k)
            idx = sorted({0, size - 1, size // 2} | set(N.cells) | {int(v) for v in self.rng.integers(0, size, size=12)})
            for ptr, T, what in ((ntree_ptr, N, "numerators"), (dtree_ptr, D, "denominators")):
                want = [T.at(i) for i in idx]
                assert np.array_equal(rows(ptr, [off + i for i in idx]), limbs([w * R % P for w in want])), (tag, what, "level", k)
            root = (N.at(0), D.at(0))
        return root


def tree_times(S, reps, with_baseline):
    from algebra_amd._lib import check, lib
    L, A, nu, n = lib(), S.A, S.nu, S.n
    num, den = S.num.evaluations, S.den.evaluations
    field = den.field
    ntree, dtree = A.DeviceVec(FIELD, n - 1, _zero=False), A.DeviceVec(FIELD, n - 1, _zero=False)
    tmp = A.DeviceVec(FIELD, n // 2, _zero=False)
    out = np.zeros((2, 4), dtype=np.uint64)
    out_p = out.ctypes.data_as(C.c_void_p)
    p = C.c_void_p

    def fused(has_num):
        check(L.ark_hip_mle_fraction_tree_device(field, num.ptr if has_num else None, den.ptr, nu, ntree.ptr, dtree.ptr, None), "tree")

    def pointwise(has_num):                                # the route a caller had: 3 products, 1 sum and a temporary per level
        nsrc, dsrc = (num.ptr.value if has_num else None), den.ptr.value
        for k in range(nu - 1, -1, -1):
            h, off = 1 << k, (n - (2 << k)) * 32
            nd, dd = ntree.ptr.value + off, dtree.ptr.value + off
            if nsrc is None:
                check(L.ark_hip_fr_add_device(field, p(dsrc), p(dsrc + 32 * h), p(nd), h), "add")
            else:
                check(L.ark_hip_fr_mul_device(field, p(nsrc), p(dsrc + 32 * h), p(tmp.ptr.value), h), "mul")
                check(L.ark_hip_fr_mul_device(field, p(nsrc + 32 * h), p(dsrc), p(nd), h), "mul")
                check(L.ark_hip_fr_add_device(field, p(nd), p(tmp.ptr.value), p(nd), h), "add")
            check(L.ark_hip_fr_mul_device(field, p(dsrc), p(dsrc + 32 * h), p(dd), h), "mul")
            nsrc, dsrc = nd, dd
    res = {}
    times = {(f, h): [] for f in ("fused", "pointwise") for h in (True, False)}
    for _ in range(ROUNDS):                                # interleaved, so that drift hits all alike
        for has_num in (True, False):
            times["fused", has_num].append(timed(lambda: fused(has_num), reps))
            if with_baseline:
                times["pointwise", has_num].append(timed(lambda: pointwise(has_num), reps))
    for has_num in (True, False):
        tag = "with_num" if has_num else "ones"
        for name, fn in (("pointwise", pointwise), ("fused", fused)):
            if name == "pointwise" and not with_baseline:
                continue
            for t in (ntree, dtree):
                check(L.ark_hip_memset_device(t.ptr, 0, (n - 1) * 32), "memset")
            fn(has_num)
            check(L.ark_hip_synchronize(), "sync")
            root = S.check_trees(ntree.ptr, dtree.ptr, has_num, (name, tag))
        res["tree_async_" + tag] = spread(times["fused", has_num])
        if with_baseline:
            res["tree_pointwise_launches_" + tag] = spread(times["pointwise", has_num])
        res["tree_with_root_%s_ms" % tag] = round(timed(lambda: check(L.ark_hip_mle_fraction_tree_device(
            field, num.ptr if has_num else None, den.ptr, nu, ntree.ptr, dtree.ptr, out_p), "tree"), reps), 4)
        assert np.array_equal(out, limbs([v * S.R % S.P for v in root])), "root"
    res["plan"] = dict(zip(("levels_per_run", "group_log_per_run"), A.mle_fraction_tree_plan(nu)))
    for v in (ntree, dtree, tmp):
        v.free()
    return res


def challenge_int(S, layer, rnd, values):
    tag = bytes([layer, 255 if rnd is None else 254 if rnd == "lambda" else rnd])
    h = hashlib.sha256(b"bench" + tag + np.ascontiguousarray(values, dtype="<u8").tobytes()).digest()
    return int.from_bytes(h + hashlib.sha256(h).digest()[:8], "little") % S.P


def verify(S, proof, has_num, num_eval, den_eval):
    """the verifier of the layered proof on integers; -> the number of sumcheck rounds it walked"""
    P = S.P
    Rinv = pow(S.R, -1, P)
    dec = lambda x: [v * Rinv % P for v in ints(np.asarray(x).reshape(-1, 4))]   # noqa: E731

    def interpolate(evals, x):
        d, total = len(evals) - 1, 0
        for i, y in enumerate(evals):
            num = den = 1
            for k in range(d + 1):
                if k != i:
                    num, den = num * (x - k) % P, den * (i - k) % P
            total += y * num * pow(den, -1, P)
        return total % P
    pp, qq = dec(proof.root)
    walked, r, cn, cd = 0, None, None, None
    nu = len(proof.layers)
    for k, (sc, values) in enumerate(proof.layers):
        v = dec(values)
        n0, n1, d0, d1 = [1, 1] + v if (not has_num and k + 1 == nu) else v
        rho = []
        if k == 0:
            assert (n0 * d1 + n1 * d0) % P == pp and d0 * d1 % P == qq, "layer 0"
        else:
            lam = challenge_int(S, k, "lambda", np.zeros((0, 4), dtype=np.uint64))
            rho, expected = dec(sc.point), (cn + lam * cd) % P
            assert len(sc.rounds) == k and len(rho) == k
            for i, (g, x) in enumerate(zip(sc.rounds, rho)):
                assert x == challenge_int(S, k, i, g), ("layer", k, "the point is not the transcript's")
                g = dec(g)
                assert (g[0] + g[1]) % P == expected, ("layer", k, "round", i)
                expected = interpolate(g, x)
                walked += 1
            eq = 1
            for x, y in zip(r, rho):
                eq = eq * (x * y + (1 - x) * (1 - y)) % P
            assert expected == eq * (n0 * d1 + n1 * d0 + lam * d0 * d1) % P, ("layer", k, "last round")
        tau = challenge_int(S, k, None, values)
        r = rho + [tau]
        cn, cd = (n0 + tau * (n1 - n0)) % P, (d0 + tau * (d1 - d0)) % P
    assert r == dec(proof.point), "the proof's point"
    assert cd == dec(den_eval)[0], "the last claim is den(point)"
    assert cn == (dec(num_eval)[0] if has_num else 1), "the last claim is num(point)"
    return walked


def proof_times(S):
    """FractionalSum.prove through the public mirror with a clock in its callback: the time between two asks is the step
    that produced the second one's values"""
    from algebra_amd._lib import check, lib
    A, L, nu = S.A, lib(), S.nu
    res = {}
    for has_num in (True, False):
        tag = "with_num" if has_num else "ones"
        t = {"trees_and_layer_0": 0.0, "eq_tables": 0.0, "sumcheck_large_layers": 0.0, "tail_layers": 0.0}
        clock = time.perf_counter
        last = [None]

        def challenge(layer, rnd, values):
            now = clock()
            dt = now - last[0]
            if layer == 0:
                t["trees_and_layer_0"] += dt
            elif layer < SMALL:
                t["tail_layers"] += dt
            elif rnd == 0:
                t["eq_tables"] += dt                       # lambda's ask -> round 0: the eq table, the list and the first round
            else:
                t["sumcheck_large_layers"] += dt
            out = limbs([challenge_int(S, layer, rnd, values) * S.R % S.P])[0]
            last[0] = clock()                              # the transcript's own time is not the prover's
            return out
        check(L.ark_hip_synchronize(), "sync")
        t0 = last[0] = clock()
        proof = A.FractionalSum(S.num if has_num else None, S.den).prove(challenge)
        whole = clock() - t0
        rounds = verify(S, proof, has_num, S.num.evaluate(proof.point) if has_num else None, S.den.evaluate(proof.point))
        res["proof_%s_ms" % tag] = round(whole * 1e3, 3)
        res["proof_%s_split_ms" % tag] = {k: round(v * 1e3, 3) for k, v in t.items()}
        res["proof_%s_tail_share" % tag] = round(t["tail_layers"] / whole, 3)
        res["proof_sumcheck_rounds"] = rounds
    res["proof_small_layers_below_num_vars"] = SMALL
    res["proof_split_note"] = ("eq_tables: from a large layer's ask for lambda to its round 0, i.e. the eq table, the list and the first "
                               "round; sumcheck_large_layers: its other rounds and final evaluations; the hashing of the callback is excluded")
    return res


def run(nu):
    from algebra_amd._lib import check, lib
    S = Setup(nu)
    A, L, n = S.A, lib(), S.n
    reps = 20 if nu <= 20 else 10 if nu <= 22 else 5
    res = {"num_vars": nu, "n": n, "reps": reps, "rounds": ROUNDS}
    others = [A.DeviceVec(FIELD, n, _zero=False) for _ in range(2)]
    srcs = [S.num.evaluations, S.den.evaluations]

    def copy():
        for o, s in zip(others, srcs):
            check(L.ark_hip_memcpy_d2d(o.ptr, s.ptr, n * 32), "d2d")
    res["d2d_two_tables_ms"] = round(timed(copy, reps), 4)
    pinned = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")

    def round_trip():
        for o, s in zip(others, srcs):
            check(L.ark_hip_memcpy_d2h(pinned, s.ptr, n * 32), "d2h")
            check(L.ark_hip_memcpy_h2d(o.ptr, pinned, n * 32), "h2d")
    res["d2h_h2d_two_tables_ms"] = round(timed(round_trip, max(3, reps // 2), warm=1), 3)
    check(L.ark_hip_host_free(pinned), "host_free")
    for o in others:
        o.free()
    res.update(tree_times(S, reps, True))
    res.update(proof_times(S))
    for tag in ("with_num", "ones"):
        a, b = res["tree_async_" + tag], res["tree_pointwise_launches_" + tag]
        res["tree_speedup_over_pointwise_" + tag] = round(b["median_ms"] / a["median_ms"], 2)
        res["tree_gain_exceeds_both_spreads_" + tag] = bool(b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"])
        res["tree_times_d2d_" + tag] = round(a["median_ms"] / res["d2d_two_tables_ms"], 2)
        res["proof_over_d2h_h2d_" + tag] = round(res["proof_%s_ms" % tag] / res["d2h_h2d_two_tables_ms"], 2)
    for name in ("num", "den"):
        assert np.array_equal(S.tables[name][2].to_evaluations()[:4096], S.tables[name][1][:4096]), "input changed"
    return res


def counts(log_n):
    import algebra_amd as A
    from algebra_amd import curves as cv
    from algebra_amd._lib import check, lib
    L, n = lib(), 1 << log_n
    P = cv.SCALAR_MODULUS[FIELD]
    R = (1 << 256) % P
    reps = 5
    res = {"n": n, "reps": reps, "rounds": ROUNDS, "cases": []}
    d_idx, d_copy = C.c_void_p(), C.c_void_p()
    check(L.ark_hip_malloc(n * 4, C.byref(d_idx)), "malloc")
    check(L.ark_hip_malloc(n * 4, C.byref(d_copy)), "malloc")
    res["d2d_indices_ms"] = round(timed(lambda: check(L.ark_hip_memcpy_d2d(d_copy, d_idx, n * 4), "d2d"), reps), 4)
    rng = np.random.default_rng(77)
    for table_log in (16, 24):
        table_len = 1 << table_log
        out = A.DeviceVec(FIELD, table_len, _zero=False)
        sets = {"uniform": rng.integers(0, table_len, size=n, dtype=np.uint32),
                "all_equal": np.full(n, table_len // 3, dtype=np.uint32),
                "witness_like_mix": np.where(rng.random(n) < 0.5, rng.integers(0, 256, size=n), rng.integers(0, table_len, size=n)).astype(np.uint32)}
        case = {"table_len": table_len}
        times = {k: [] for k in sets}
        for _ in range(ROUNDS):
            for name, idx in sets.items():
                check(L.ark_hip_memcpy_h2d(d_idx, idx.ctypes.data_as(C.c_void_p), idx.nbytes), "h2d")
                times[name].append(timed(lambda: check(L.ark_hip_fr_count_indices_device(out.field, d_idx, n, out.ptr, table_len), "count"), reps))
        for name, idx in sets.items():
            check(L.ark_hip_memcpy_h2d(d_idx, idx.ctypes.data_as(C.c_void_p), idx.nbytes), "h2d")
            check(L.ark_hip_memset_device(out.ptr, 0xAB, table_len * 32), "memset")
            check(L.ark_hip_fr_count_indices_device(out.field, d_idx, n, out.ptr, table_len), "count")
            want = np.bincount(idx, minlength=table_len)
            assert int(want.sum()) == n
            if table_log <= 16:
                assert np.array_equal(out.to_host(), limbs([int(c) * R % P for c in want])), (name, table_len)
            else:
                cells = sorted({0, table_len - 1, table_len // 3, 255, 256} | {int(v) for v in rng.integers(0, table_len, size=60)} | {int(v) for v in idx[:20]})
                got = np.zeros((len(cells), 4), dtype=np.uint64)
                for q, j in enumerate(cells):
                    check(L.ark_hip_memcpy_d2h(got[q].ctypes.data_as(C.c_void_p), C.c_void_p(out.ptr.value + j * 32), 32), "d2h")
                assert np.array_equal(got, limbs([int(want[j]) * R % P for j in cells])), (name, table_len)
            case[name] = spread(times[name])
        case["all_equal_over_uniform"] = round(case["all_equal"]["median_ms"] / case["uniform"]["median_ms"], 2)
        case["uniform_times_d2d_indices"] = round(case["uniform"]["median_ms"] / res["d2d_indices_ms"], 2)
        res["cases"].append(case)
        out.free()
    check(L.ark_hip_free(d_idx), "free")
    check(L.ark_hip_free(d_copy), "free")
    return res


def child(args, limit, env=None):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                         env=dict(os.environ, **(env or {})))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        print(out.stdout[-4000:] + out.stderr[-4000:])
        return None, out.returncode
    return json.loads(line[-1][len("RESULT "):]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fraction_sum.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--variants", default=None, help="a directory of libark_hip*.so builds to time the trees with")
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None)
    ap.add_argument("--tree", type=int, default=None)
    ap.add_argument("--counts", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    if args.tree is not None:
        nu = args.tree
        print("RESULT " + json.dumps(tree_times(Setup(nu), 20 if nu <= 20 else 10 if nu <= 22 else 5, False)), flush=True)
        return 0
    if args.counts is not None:
        print("RESULT " + json.dumps(counts(args.counts)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; the trees, their "
                     "baseline and the counts in `rounds` interleaved rounds; the proof host-observed, every round waits",
           "sizes": []}
    libs = sorted(glob.glob(os.path.join(args.variants, "libark_hip*.so"))) if args.variants else []
    for lg in (int(x) for x in args.logs.split(",")):
        # a fresh process per size and variant, under its own time limit; a failure ends the run: nothing more is started on the GPU
        r, rc = child(["--one", str(lg)], args.limit)
        if r is None:
            print("size 2^%d failed with status %d: stopping" % (lg, rc))
            return 1
        r["tree_variants"] = {}
        for path in libs:
            v, rc = child(["--tree", str(lg)], args.limit, {"ARK_HIP_LIB": os.path.abspath(path)})
            if v is None:
                print("variant %s at 2^%d failed with status %d: stopping" % (path, lg, rc))
                return 1
            r["tree_variants"][os.path.basename(path)] = v
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    c, rc = child(["--counts", "24"], args.limit)
    if c is None:
        print("the counts failed with status %d: stopping" % rc)
        return 1
    out["counts"] = c
    print(json.dumps(c), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
