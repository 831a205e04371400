"""Times the sumcheck prover's round (ark_hip_sumcheck_round_device) over BLS12-381 Fr at nu = 20, 22 and 24 for three shapes
of the sum --

  ab         one product of 2 tables                     a b                 (degree 2)
  eq_ab      one product of 3 tables                     eq a b              (degree 3)
  two_terms  4 tables in 2 terms of degree 3             eq a b + k eq c b

-- a plain round, a fused round (the previous challenge bound in the same launch) and a whole prove, next to three yardsticks
measured in the same run over the same M tables:

  (a) ark_hip_memcpy_d2d of the M tables: what moving their bytes in and out of HBM costs;
  (b) ark_hip_memcpy_d2h + ark_hip_memcpy_h2d of the M tables through pinned host memory: the only route there was before this
      entry (download, host arithmetic -- not even counted --, upload);
  (c) the unfused chain for one round: M calls of ark_hip_mle_fix_variables_device with dim = 1 -- the existing kernel over
      the same bytes -- and then a plain round over the halves.

Every timed result is checked against Python big integers: a table is a base block of 2^8 random elements repeated, with
a few cells planted (first and last pair, a workgroup seam, the grid-stride tail), and both parts fold exactly, so the model
costs 2^7 pairs per round whatever nu is.  Round evaluations are compared in full, bound tables at sampled rows, and a
proof goes through a verifier: g_0(0) + g_0(1) is the sum, g_i(r) by Lagrange interpolation is g_(i+1)(0) + g_(i+1)(1), the
last value is sum_j c_j prod_k f_k(point).

Timing: a round returns its evaluations to the host and waits inside the call, so every row here is HOST-OBSERVED LATENCY by
the wall clock over `reps` calls after warm-up calls; the copies are queued calls bracketed by ark_hip_synchronize().

Every size runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_sumcheck.py [--out profiles/sumcheck.json] [--logs 20,22,24] [--limit 300]
    python tools/bench_sumcheck.py --one 24          (one size in this process, its JSON line on stdout)
"""
import argparse
import ctypes as C
import datetime
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD = "BLS12_381_FR"
PERIOD_LOG = 8
SHAPES = {"ab": (2, [(None, [0, 1])]), "eq_ab": (3, [(None, [0, 1, 2])]), "two_terms": (4, [(None, [0, 1, 2]), ("k", [0, 3, 2])])}


def limbs(xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


class Periodic:
    """2^m canonical values: base[i mod len(base)] except at the planted cells"""

    def __init__(self, m, base, cells):
        self.m, self.base, self.cells = m, list(base), dict(cells)

    def at(self, i):
        v = self.cells.get(i)
        return self.base[i % len(self.base)] if v is None else v

    def fold(self, r, p):
        """out[b] = t[2b] + r (t[2b+1] - t[2b]): the base block on its own, a cell where either parent is planted"""
        b = self.base
        base = [(b[2 * i] + r * (b[2 * i + 1] - b[2 * i])) % p for i in range(len(b) // 2)] if len(b) > 1 else list(b)
        cells = {}
        for i in self.cells:
            o = i >> 1
            cells[o] = (self.at(2 * o) + r * (self.at(2 * o + 1) - self.at(2 * o))) % p
        return Periodic(self.m - 1, base, cells)


def pair_values(lo, hi, terms, degree, p):
    out = []
    for t in range(degree + 1):
        v = [(a + t * (b - a)) % p for a, b in zip(lo, hi)]
        s = 0
        for c, ix in terms:
            pr = c
            for k in ix:
                pr = pr * v[k] % p
            s += pr
        out.append(s % p)
    return out


def round_sums(tables, terms, degree, p):
    """the D + 1 round sums from the definition: whole periods from the base blocks, then what the planted pairs change"""
    npairs = 1 << (tables[0].m - 1)
    period = max(max(len(t.base) // 2, 1) for t in tables)

    def base_pair(b):
        return [t.base[(2 * b) % len(t.base)] for t in tables], [t.base[(2 * b + 1) % len(t.base)] for t in tables]
    acc = [0] * (degree + 1)
    for b in range(period):
        acc = [a + v for a, v in zip(acc, pair_values(*base_pair(b), terms, degree, p))]
    acc = [a * (npairs // period) % p for a in acc]
    for b in sorted({i >> 1 for t in tables for i in t.cells}):
        now = pair_values([t.at(2 * b) for t in tables], [t.at(2 * b + 1) for t in tables], terms, degree, p)
        acc = [(a + x - y) % p for a, x, y in zip(acc, now, pair_values(*base_pair(b), terms, degree, p))]
    return acc


def interpolate(evals, x, p):
    total = 0
    for i, y in enumerate(evals):
        num, den = 1, 1
        for k in range(len(evals)):
            if k != i:
                num, den = num * (x - k) % p, den * (i - k) % p
        total += y * num * pow(den, -1, p)
    return total % p


def products_per_pair(terms, degree, unit, ntables, fused):
    """(issued by the kernel, what the arithmetic needs): a term of len factors is evaluated at all D + 1 points and costs
    len - 1 products at each, 2 more when its coefficient is not one, 2 per table for the bind; needed: len - 1 products at
    the term's own len + 1 points, the coefficient applied to the sums, the same bind"""
    issued = sum((len(ix) - 1) * (degree + 1) + (0 if u else 2) for (_, ix), u in zip(terms, unit))
    needed = sum((len(ix) - 1) * (len(ix) + 1) for _, ix in terms)
    bind = 2 * ntables if fused else 0
    return issued + bind, needed + bind


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
    rng = np.random.default_rng(400 + nu)
    n = 1 << nu
    reps = 20 if nu <= 20 else 10 if nu <= 22 else 5
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % P   # noqa: E731
    mont = lambda xs: limbs([x * R % P for x in xs])            # noqa: E731
    spots = sorted(i for i in {0, 1, n - 1, n - 2, 511, 512, 1023, 1024, (1 << 19) + 3, (1 << 20) + 6, n // 2 + 1} if 0 <= i < n)
    models, mles = [], []
    for k in range(4):
        base = [rnd() for _ in range(1 << PERIOD_LOG)]
        cells = {i: (0, P - 1, rnd())[q % 3] for q, i in enumerate(spots[k % 2::2] if k else spots)}
        a = np.tile(mont(base), (n >> PERIOD_LOG, 1))
        for i, v in cells.items():
            a[i] = mont([v])[0]
        models.append(Periodic(nu, base, cells))
        mles.append(A.DenseMultilinearExtension.from_evaluations(FIELD, nu, a))
        del a
    kcoef = rnd()
    r1 = rnd()
    r1M = mont([r1])[0]
    sample = sorted({0, 1, 255, 256, 257, 511, 512, n // 4, n // 2 - 2, n // 2 - 1} | {int(v) for v in rng.integers(0, n // 2, size=16)})

    def rows(ptr, idx):
        out = np.zeros((len(idx), 4), dtype=np.uint64)
        for q, i in enumerate(idx):
            check(L.ark_hip_memcpy_d2h(out[q].ctypes.data_as(C.c_void_p), C.c_void_p(ptr + int(i) * 32), 32), "d2h")
        return out

    def challenge_of(evals_limbs, i):
        h = hashlib.sha256(bytes([i]) + np.ascontiguousarray(evals_limbs, dtype="<u8").tobytes()).digest()
        return int.from_bytes(h + h[:8], "little") % P

    res = {"num_vars": nu, "n": n, "reps": reps, "plan_plain": A.sumcheck_plan(nu), "plan_fused": A.sumcheck_plan(nu, fused=True), "shapes": {}}
    other = [A.DeviceVec(FIELD, n, _zero=False) for _ in range(4)]
    pinned = C.c_void_p()
    check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")
    for name, (nt, spec) in SHAPES.items():
        terms = [((1 if c is None else kcoef), ix) for c, ix in spec]
        unit = [c is None for c, _ in spec]
        degree = max(len(ix) for _, ix in terms)
        tm = models[:nt]
        row = {"tables": nt, "terms": [ix for _, ix in terms], "degree": degree}

        def new_list():
            lp = A.ListOfProducts(FIELD, nu)
            for c, ix in terms:
                lp.add_product([mles[k] for k in ix], mont([c])[0])
            return lp

        # yardsticks (a) and (b) over the same M tables
        row["d2d_ms"] = timed(lambda: [check(L.ark_hip_memcpy_d2d(other[k].ptr, mles[k].evaluations.ptr, n * 32), "d2d") for k in range(nt)], reps)

        def round_trip():
            for k in range(nt):
                check(L.ark_hip_memcpy_d2h(pinned, mles[k].evaluations.ptr, n * 32), "d2h")
                check(L.ark_hip_memcpy_h2d(other[k].ptr, pinned, n * 32), "h2d")
        row["d2h_h2d_ms"] = timed(round_trip, max(2, reps // 3), warm=1)

        # a plain round
        lp = new_list()
        want = mont(round_sums(tm, terms, degree, P))
        row["plain_ms"] = timed(lambda: lp.round(), reps)
        assert np.array_equal(lp.round(), want), (name, "plain")

        # a fused round, and (c) the unfused chain: every call starts from the caller's tables
        bound = [t.fold(r1, P) for t in tm]
        want = mont(round_sums(bound, terms, degree, P))
        for label, fused in (("fused_ms", True), ("unfused_chain_ms", False)):
            lp = new_list()
            lp.round(r1M, fused=fused)                      # allocates the list's tables

            def one():
                lp.reset()
                return lp.round(r1M, fused=fused)
            row[label] = timed(one, reps)
            assert np.array_equal(one(), want), (name, label)
            for k in range(nt):
                assert np.array_equal(rows(lp.bound_pointers()[k], sample), mont([bound[k].at(i) for i in sample])), (name, label, "bound table", k)
            lp.free()

        # a whole prove, bound in the round's launch and by the fold kernel
        for label, fused in (("prove_ms", True), ("prove_unfused_ms", False)):
            proof = [None]

            def prove():
                lp = new_list()
                proof[0] = lp.prove(lambda i, evals: mont([challenge_of(evals, i)])[0], fused=fused)
                lp.free()
            row[label] = timed(prove, max(2, reps // 3), warm=1)
            pr = proof[0]
            cur, g = list(tm), round_sums(tm, terms, degree, P)
            expected = (g[0] + g[1]) % P                    # the claimed sum, from the model
            for i in range(nu):
                got = [x * pow(R, -1, P) % P for x in ints(pr.rounds[i])]
                assert got == round_sums(cur, terms, degree, P), (name, label, "round", i)
                assert (got[0] + got[1]) % P == expected, (name, label, "verifier", i)
                r = challenge_of(pr.rounds[i], i)
                assert np.array_equal(pr.point[i], mont([r])[0])
                expected = interpolate(got, r, P)
                cur = [t.fold(r, P) for t in cur]
            finals = [t.at(0) for t in cur]
            assert np.array_equal(pr.final_evaluations, mont(finals)), (name, label, "final values")
            assert expected == pair_values(finals, finals, terms, degree, P)[0], (name, label, "the verifier's last check")
            assert np.array_equal(pr.final_value, mont([expected])[0]), (name, label, "final value")

        row["products_per_pair_plain"] = products_per_pair(terms, degree, unit, nt, False)
        row["products_per_pair_fused"] = products_per_pair(terms, degree, unit, nt, True)
        row["plain_vs_d2h_h2d"] = round(row["d2h_h2d_ms"] / row["plain_ms"], 1)
        row["fused_vs_d2h_h2d"] = round(row["d2h_h2d_ms"] / row["fused_ms"], 1)
        row["fused_vs_unfused_chain"] = round(row["unfused_chain_ms"] / row["fused_ms"], 2)
        row["plain_vs_d2d"] = round(row["plain_ms"] / row["d2d_ms"], 2)
        res["shapes"][name] = row
    check(L.ark_hip_host_free(pinned), "host_free")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck.json"))
    ap.add_argument("--logs", default="20,22,24")
    ap.add_argument("--limit", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--one", type=int, default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "host-observed wall clock per call over `reps` calls after warm-up; every round waits for its evaluations",
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
