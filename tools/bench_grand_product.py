"""Times the grand-product entries at nu = 20, 22 and 24 over BLS12-381 Fr, next to the routes they
replace and to yardsticks measured in the same run:

  tree       ark_hip_mle_product_tree_device (asynchronous, and with the product, which waits) against
             (a) nu calls of ark_hip_fr_mul_device on the half-levels, into the same tree buffer: the route a caller had;
             (b) ark_hip_memcpy_d2d of one table: the byte floor (the tree reads n elements and writes n - 1);
             (c) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d of the table through pinned memory: the floor of a host prover.
             With --variants DIR every libark_hip*.so in DIR (other builds of the library, such as ones that differ in
             PROD_TREE_MAX_W of csrc/grand_product.cuh) times the same tree in a process of its own.
  lincomb    ark_hip_fr_lincomb_device at K = 3 and 8 against K calls of ark_hip_fr_axpy_device.
  proof      GrandProduct.prove's steps, host-observed (every round waits for its evaluations, as in section 17), split into
             the tree, the eq tables, the sumcheck rounds of the layers of at least SMALL variables and the layers below.

tree and its baseline are timed in ROUNDS interleaved rounds; the JSON keeps every round, the median, and the spread
(max - min) so that a difference can be held against it.

Every timed result is checked.  The table is a base block of 2^12 random elements repeated, with planted cells (0 is not
among them: it would hide everything above it); level k >= 12 of its tree is the block's elementwise power, changed where a
planted cell reaches it, and the levels below are walked in full -- all on Python integers.  The linear combination is
checked at sampled rows.  The proof is checked by a verifier written out here (round sums chained by Lagrange interpolation,
the last round against eq(r, rho) left right) and its last claim against evaluate on the device.

Every size runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_grand_product.py [--out profiles/grand_product.json] [--logs 20,22,24] [--variants DIR] [--limit 300]
    python tools/bench_grand_product.py --one 24          (one size in this process, its JSON line on stdout)
    python tools/bench_grand_product.py --tree 24         (the tree alone, for a variant named by ARK_HIP_LIB)
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


class Setup:
    """the table on the device and its tree on integers"""

    def __init__(self, nu):
        import algebra_amd as A
        from algebra_amd import curves as cv
        self.A, self.nu, self.n = A, nu, 1 << nu
        self.P = cv.SCALAR_MODULUS[FIELD]
        self.R = (1 << 256) % self.P
        rng = np.random.default_rng(300 + nu)
        self.rng = rng
        rnd = lambda: int.from_bytes(rng.bytes(40), "little") % self.P or 1   # noqa: E731
        self.rnd = rnd
        self.base = [rnd() for _ in range(1 << LO)]                            # canonical values
        n = self.n
        self.cells = {i: v for i, v in ((1, 1), (2, self.P - 1), (n - 1, rnd()), (n // 2, rnd()), (n // 2 - 1, rnd()), (n - 1 - (1 << LO), rnd()))}
        blk = limbs([x * self.R % self.P for x in self.base])
        a = np.tile(blk, (n >> LO, 1))
        for i, v in self.cells.items():
            a[i] = limbs([v * self.R % self.P])[0]
        self.host = a
        self.m = A.DenseMultilinearExtension.from_evaluations(FIELD, nu, a)

    def level_models(self):
        """[(k, base block or full list, cells)] for k = nu .. 0 on canonical integers"""
        P, nu = self.P, self.nu
        base, cells = list(self.base), dict(self.cells)
        out = [(nu, base, cells)]
        for k in range(nu - 1, -1, -1):
            h = 1 << k
            if k >= LO:
                def at(i, base=base, cells=cells):
                    v = cells.get(i)
                    return base[i % len(base)] if v is None else v
                ncells = {}
                for i in cells:
                    o = i % h
                    ncells[o] = at(o) * at(o + h) % P
                base, cells = [b * b % P for b in base], ncells
            else:
                if cells is not None:                     # level LO in full, the planted cells applied
                    for i, v in cells.items():
                        base[i] = v
                    cells = None
                base = [base[i] * base[i + h] % P for i in range(h)]
            out.append((k, base, cells or {}))
        return out

    def check_tree(self, tree_ptr, tag):
        from algebra_amd._lib import check, lib
        L, n, P, R = lib(), self.n, self.P, self.R

        def rows(idx):
            out = np.zeros((len(idx), 4), dtype=np.uint64)
            for q, i in enumerate(idx):
                check(L.ark_hip_memcpy_d2h(out[q].ctypes.data_as(C.c_void_p), C.c_void_p(tree_ptr.value + int(i) * 32), 32), "d2h")
            return out
        product = None
        for k, base, cells in self.level_models()[1:]:
            size, off = 1 << k, n - (2 << k)
            idx = sorted({0, size - 1, size // 2} | set(cells) | {int(v) for v in self.rng.integers(0, size, size=12)})
            want = [cells.get(i, base[i % len(base)]) for i in idx]
            assert np.array_equal(rows([off + i for i in idx]), limbs([w * R % P for w in want])), (tag, "level", k)
            product = want[0]
        return product


def tree_times(S, reps, with_baseline):
    from algebra_amd._lib import check, lib
    L, A, nu, n = lib(), S.A, S.nu, S.n
    tab = S.m.evaluations
    tree = A.DeviceVec(FIELD, n - 1, _zero=False)
    out = np.zeros(4, dtype=np.uint64)
    out_p = out.ctypes.data_as(C.c_void_p)

    def fused():
        check(L.ark_hip_mle_product_tree_device(tab.field, tab.ptr, nu, tree.ptr, None), "tree")

    def pointwise():                                       # the route a caller had: one ark_hip_fr_mul_device per level
        src = tab.ptr.value
        for k in range(nu - 1, -1, -1):
            dst = tree.ptr.value + (n - (2 << k)) * 32
            check(L.ark_hip_fr_mul_device(tab.field, C.c_void_p(src), C.c_void_p(src + (32 << k)), C.c_void_p(dst), 1 << k), "mul")
            src = dst
    res = {}
    f, b = [], []
    for _ in range(ROUNDS):                                # interleaved, so that drift hits both alike
        f.append(timed(fused, reps))
        if with_baseline:
            b.append(timed(pointwise, reps))
    if with_baseline:
        check(L.ark_hip_memset_device(tree.ptr, 0, (n - 1) * 32), "memset")
        pointwise()
        check(L.ark_hip_synchronize(), "sync")
        S.check_tree(tree.ptr, "pointwise")
        res["tree_pointwise_launches"] = spread(b)
    check(L.ark_hip_memset_device(tree.ptr, 0, (n - 1) * 32), "memset")
    fused()
    check(L.ark_hip_synchronize(), "sync")
    product = S.check_tree(tree.ptr, "fused")
    res["tree_async"] = spread(f)
    res["tree_with_product_ms"] = round(timed(lambda: check(L.ark_hip_mle_product_tree_device(tab.field, tab.ptr, nu, tree.ptr, out_p), "tree"), reps), 4)
    assert np.array_equal(out, limbs([product * S.R % S.P])[0]), "product"
    res["plan"] = dict(zip(("levels_per_run", "group_log_per_run"), A.mle_product_tree_plan(nu)))
    tree.free()
    return res


def verify(S, proof, f_eval):
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
    product = dec(proof.product)[0]
    walked, r, claim = 0, None, None
    for k, (sc, pair) in enumerate(proof.layers):
        left, right = dec(pair)
        rho = []
        if k == 0:
            assert left * right % P == product, "layer 0"
        else:
            rho, expected = dec(sc.point), claim
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
            assert expected == eq * left % P * right % P, ("layer", k, "last round")
        tau = challenge_int(S, k, None, pair)
        r = rho + [tau]
        claim = (left + tau * (right - left)) % P
    assert r == dec(proof.point), "the proof's point"
    assert claim == dec(f_eval)[0], "the last claim is f(point)"
    return walked


def challenge_int(S, layer, rnd, values):
    tag = bytes([layer, 255 if rnd is None else rnd])
    h = hashlib.sha256(b"bench" + tag + np.ascontiguousarray(values, dtype="<u8").tobytes()).digest()
    return int.from_bytes(h + hashlib.sha256(h).digest()[:8], "little") % S.P


def proof_times(S):
    """GrandProduct.prove's own steps through the public mirror, with a clock around each kind"""
    from algebra_amd._lib import check, lib
    from algebra_amd.grand_product import GrandProductProof, _one
    A, L, nu, m = S.A, lib(), S.nu, S.m
    MLE = A.DenseMultilinearExtension
    challenge = lambda layer, rnd, values: limbs([challenge_int(S, layer, rnd, values) * S.R % S.P])[0]   # noqa: E731
    t = {"tree": 0.0, "eq_tables": 0.0, "sumcheck_large_layers": 0.0, "tail_layers": 0.0}
    clock = time.perf_counter
    check(L.ark_hip_synchronize(), "sync")
    t_all = clock()
    t0 = clock()
    product, levels = m.product_tree()
    t["tree"] = clock() - t0
    level = [m.evaluations] + levels
    one = _one(m.field)
    t0 = clock()
    pair = level[nu - 1].to_host()
    point = challenge(0, None, pair).reshape(1, 4)
    layers = [(None, pair)]
    t["tail_layers"] += clock() - t0
    for k in range(1, nu):
        up = level[nu - k - 1]
        t0 = clock()
        eq = MLE.eq(FIELD, point)
        check(L.ark_hip_synchronize(), "sync")
        t1 = clock()
        lp = A.ListOfProducts(FIELD, k)
        lp.add_product([eq, MLE(k, A.DeviceSegment(up, 0, 1 << k)), MLE(k, A.DeviceSegment(up, 1 << k, 1 << k))], one)
        proof = lp.prove(lambda i, evals, k=k: challenge(k, i, evals))
        lp.free()
        eq.free()
        pair = proof.final_evaluations[1:3].copy()
        point = np.concatenate([proof.point, challenge(k, None, pair).reshape(1, 4)])
        layers.append((proof, pair))
        t2 = clock()
        if k >= SMALL:
            t["eq_tables"] += t1 - t0
            t["sumcheck_large_layers"] += t2 - t1
        else:
            t["tail_layers"] += t2 - t0
    total = clock() - t_all
    levels[0].owner.free()
    proof = GrandProductProof(product, layers, point)
    rounds = verify(S, proof, m.evaluate(point))
    # the mirror's own prove, timed as one piece, writes the same proof
    t0 = clock()
    same = A.GrandProduct(m).prove(challenge)
    whole = clock() - t0
    assert np.array_equal(same.point, point) and np.array_equal(same.product, product), "GrandProduct.prove"
    res = {"proof_ms": round(whole * 1e3, 3), "proof_split_total_ms": round(total * 1e3, 3), "proof_sumcheck_rounds": rounds,
           "proof_split_ms": {k: round(v * 1e3, 3) for k, v in t.items()}, "proof_small_layers_below_num_vars": SMALL}
    res["proof_tail_share"] = round(t["tail_layers"] / total, 3)
    return res


def run(nu):
    from algebra_amd._lib import check, lib
    S = Setup(nu)
    A, L, n = S.A, lib(), S.n
    reps = 20 if nu <= 20 else 10 if nu <= 22 else 5
    tab = S.m.evaluations
    res = {"num_vars": nu, "n": n, "reps": reps, "rounds": ROUNDS}
    other = A.DeviceVec(FIELD, n, _zero=False)
    res["d2d_ms"] = round(timed(lambda: check(L.ark_hip_memcpy_d2d(other.ptr, tab.ptr, n * 32), "d2d"), reps), 4)
    pinned = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")

    def round_trip():
        check(L.ark_hip_memcpy_d2h(pinned, tab.ptr, n * 32), "d2h")
        check(L.ark_hip_memcpy_h2d(other.ptr, pinned, n * 32), "h2d")
    res["d2h_h2d_ms"] = round(timed(round_trip, max(3, reps // 2), warm=1), 3)
    check(L.ark_hip_host_free(pinned), "host_free")
    res.update(tree_times(S, reps, True))

    # the linear combination against K passes of a + k x
    for K in (3, 8):
        hosts = [np.roll(S.host, 17 * (k + 1), axis=0) for k in range(K)]
        devs = [A.DeviceVec.from_host(FIELD, h) for h in hosts]
        coeffs = [S.rnd() for _ in range(K)]
        gamma = S.rnd()
        kc = limbs([c * S.R % S.P for c in coeffs])
        g = limbs([gamma * S.R % S.P])[0]
        ptrs = (C.c_void_p * K)(*[d.ptr.value for d in devs])

        def lincomb():
            check(L.ark_hip_fr_lincomb_device(tab.field, ptrs, K, kc.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), other.ptr, n), "lincomb")

        def passes():
            for k in range(K):
                check(L.ark_hip_fr_axpy_device(tab.field, other.ptr, kc[k].ctypes.data_as(C.c_void_p), devs[k].ptr, other.ptr, n), "axpy")
        res["lincomb_%d_axpy_passes_ms" % K] = round(timed(passes, reps), 4)
        res["lincomb_%d_ms" % K] = round(timed(lincomb, reps), 4)
        idx = sorted({0, 1, n // 2, n - 1} | {int(v) for v in S.rng.integers(0, n, size=60)})
        got = np.zeros((len(idx), 4), dtype=np.uint64)
        for q, i in enumerate(idx):
            check(L.ark_hip_memcpy_d2h(got[q].ctypes.data_as(C.c_void_p), C.c_void_p(other.ptr.value + i * 32), 32), "d2h")
        want = [(gamma * S.R + sum(c * ints(h[i:i + 1])[0] for c, h in zip(coeffs, hosts))) % S.P for i in idx]
        assert np.array_equal(got, limbs(want)), ("lincomb", K)
        res["lincomb_%d_speedup" % K] = round(res["lincomb_%d_axpy_passes_ms" % K] / res["lincomb_%d_ms" % K], 2)
        for d in devs:
            d.free()
    other.free()

    res.update(proof_times(S))
    a, b = res["tree_async"], res["tree_pointwise_launches"]
    res["tree_speedup_over_pointwise"] = round(b["median_ms"] / a["median_ms"], 2)
    res["tree_gain_exceeds_spread"] = bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"]))
    res["tree_times_d2d"] = round(a["median_ms"] / res["d2d_ms"], 2)
    res["proof_over_d2h_h2d"] = round(res["proof_ms"] / res["d2h_h2d_ms"], 2)
    assert np.array_equal(S.m.to_evaluations()[:4096], S.host[:4096]), "input changed"
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grand_product.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--variants", default=None, help="a directory of libark_hip*.so builds to time the tree with")
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None)
    ap.add_argument("--tree", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    if args.tree is not None:
        nu = args.tree
        print("RESULT " + json.dumps(tree_times(Setup(nu), 20 if nu <= 20 else 10 if nu <= 22 else 5, False)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; tree and its "
                     "baseline in `rounds` interleaved rounds; the proof host-observed, every round waits",
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
            v, rc = child(["--tree", str(lg)], args.limit, {"ARK_HIP_LIB": path})
            if v is None:
                print("variant %s at 2^%d failed with status %d: stopping" % (path, lg, rc))
                return 1
            r["tree_variants"][os.path.basename(path)] = v
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
