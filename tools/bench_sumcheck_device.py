"""Times the whole sumcheck proof in one wait over BLS12-381 Fr against the route it replaces, in the
same session:

  device     ListOfProducts.prove_device(transcript) / GrandProduct.prove_device / FractionalSum.prove_device: the challenges
             derived on the device, one wait per proof (per layer for the layered provers);
  yardstick  the parent's route: prove(challenge) with the Transcript HOST entry as the callback -- a launch, a download and
             a wait per round.  It is not tuned here.

  `a b` and `eq a b` at nu = 12, 16, 20, 22, 24; GrandProduct and FractionalSum at nu = 20, 22, 24.  Each pair is timed in
  ROUNDS interleaved rounds (device, yardstick, device, ...); the JSON keeps every round, the median and the spread (max - min).
  Alongside: the tail_vars sweep {0, 6, 8, 10, 12, 14} for `eq a b` at nu = 20 in a process of its own and again next to
  every timed case (interleaved the same way; the layered provers pass it to every layer), the launches per
  proof from ark_hip_sumcheck_prove_plan, and the d2h + h2d round trip of the tables through pinned memory (section 19's (c)).

Every timed result is checked through the model's verifier (tests/transcript_ref.py, tests/sumcheck_ref.py,
tests/grand_product_ref.py, tests/fraction_sum_ref.py) on Python integers.  Tables are a base block of 2^12 random elements
repeated: such a table does not depend on the variables above the twelfth, so its sum over the cube is the block's sum times
the repeats, its value at a point is the block's at the point's first twelve coordinates, its product is a power of the
block's and its sum of fractions a multiple.

Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.

    python tools/bench_sumcheck_device.py [--out profiles/sumcheck_device.json] [--limit 300]
    python tools/bench_sumcheck_device.py --one eab:20        (one case in this process, its JSON line on stdout)
"""
import argparse
import ctypes as C
import datetime
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_mle_ops import FIELD, LO, limbs   # noqa: E402

ROUNDS = 3
SEED = bytes(range(32))
SWEEP = (0, 6, 8, 10, 12, 14)
CASES = ["ab:%d" % nu for nu in (12, 16, 20, 22, 24)] + ["eab:%d" % nu for nu in (12, 16, 20, 22, 24)] + ["sweep:20"] + \
        ["gp:%d" % nu for nu in (20, 22, 24)] + ["fs:%d" % nu for nu in (20, 22, 24)]


def spread(xs):
    return {"rounds_ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4), "spread_ms": round(max(xs) - min(xs), 4)}


def wall(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def interleaved(fns, reps):
    """{name: spread} of fns (name -> callable that waits for its result), ROUNDS rounds, every round all of them in turn"""
    for fn in fns.values():
        fn()                                                   # warm-up: scratch sized, code objects loaded
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            got[k].append(wall(fn, reps))
    return {k: spread(v) for k, v in got.items()}


class Tables:
    """`count` periodic tables of 2^nu elements on the device, and their base blocks on canonical integers"""

    def __init__(self, nu, count, seed):
        import algebra_amd as A
        from algebra_amd import curves as cv
        self.A, self.nu, self.p = A, nu, cv.SCALAR_MODULUS[FIELD]
        self.R = (1 << 256) % self.p
        rng = np.random.default_rng(seed + nu)
        self.lo = min(LO, nu)
        self.base = [[int.from_bytes(rng.bytes(40), "little") % self.p or 1 for _ in range(1 << self.lo)] for _ in range(count)]
        self.mles = [A.DenseMultilinearExtension.from_evaluations(FIELD, nu, np.tile(limbs([x * self.R % self.p for x in b]), (1 << (nu - self.lo), 1)))
                     for b in self.base]
        self.repeats = 1 << (nu - self.lo)

    def mont(self, x):
        return limbs([x % self.p * self.R % self.p])[0]

    def round_trip_ms(self, reps):
        from algebra_amd._lib import check, lib
        L, n = lib(), 1 << self.nu
        pinned = C.c_void_p()
        check(L.ark_hip_host_alloc(n * 32, C.byref(pinned)), "host_alloc")
        other = self.A.DeviceVec(FIELD, n, _zero=False)

        def trip():
            for m in self.mles:
                check(L.ark_hip_memcpy_d2h(pinned, m.evaluations.ptr, n * 32), "d2h")
                check(L.ark_hip_memcpy_h2d(other.ptr, pinned, n * 32), "h2d")
        trip()
        ms = wall(trip, reps)
        check(L.ark_hip_host_free(pinned), "host_free")
        other.free()
        return round(ms, 3)


def reps_for(nu):
    return 10 if nu <= 16 else 5 if nu <= 20 else 3


def run_sumcheck(kind, nu, tails=(None,)):
    import mle_ref
    import sumcheck_ref as S
    import transcript_ref as T
    nt = 2 if kind == "ab" else 3
    tb = Tables(nu, nt, 700)
    A, p = tb.A, tb.p
    terms = [(1, list(range(nt)))]
    claim = tb.repeats * sum(S.pair_values(row, row, terms, p)[0] for row in zip(*tb.base)) % p

    def make():
        lp = A.ListOfProducts(FIELD, nu)
        lp.add_product(tb.mles, tb.mont(1))
        return lp

    def check(proof, tr):
        rounds, point, finals = [S.decode(g, p) for g in proof.rounds], S.decode(proof.point, p), S.decode(proof.final_evaluations, p)
        tv = T.Transcript(p, SEED)
        assert T.verify(claim, rounds, point, finals, terms, tv, p) and tv.state == tr.state, "the model's verifier rejects"
        assert finals == [mle_ref.evaluate(b, point[:tb.lo], p) for b in tb.base], "final values"

    def device(tail):
        def fn():
            lp, tr = make(), A.Transcript(FIELD, SEED)
            fn.last = (lp.prove_device(tr, tail), tr)
            lp.free()
        return fn

    def host():
        lp, tr = make(), A.Transcript(FIELD, SEED)
        host.last = (lp.prove(lambda i, evals: tr.challenge(evals)), tr)
        lp.free()
    fns = {("device" if t is None else "tail_%d" % t): device(t) for t in tails}
    if tails == (None,):
        fns["yardstick"] = host
        fns.update({"tail_%d" % t: device(t) for t in SWEEP})   # the same sweep at every size, next to the default
    times = interleaved(fns, reps_for(nu))
    for fn in fns.values():
        check(*fn.last)
    res = {"case": kind, "num_vars": nu, "reps": reps_for(nu), "rounds": ROUNDS}
    res.update(times)
    if tails == (None,):
        w, launches, tail_from = A.sumcheck_prove_plan(nu, nt)
        res.update(launches=launches, tail_from=tail_from, yardstick_calls=nu + 1, d2h_h2d_ms=tb.round_trip_ms(3))
        finish(res)
    else:
        res["launches"] = {"tail_%d" % t: A.sumcheck_prove_plan(nu, nt, t)[1] for t in tails}
    return res


def finish(res):
    d, y = res["device"], res["yardstick"]
    res["speedup"] = round(y["median_ms"] / d["median_ms"], 2)
    res["faster_by_more_than_the_spreads"] = bool(y["median_ms"] - d["median_ms"] > max(d["spread_ms"], y["spread_ms"]))
    res["device_over_d2h_h2d"] = round(d["median_ms"] / res["d2h_h2d_ms"], 3)


def run_layered(kind, nu):
    import fraction_sum_ref as FS
    import grand_product_ref as GP
    import sumcheck_ref as S
    import transcript_ref as T
    tb = Tables(nu, 1 if kind == "gp" else 2, 900)
    A, p = tb.A, tb.p
    if kind == "gp":
        prover = A.GrandProduct(tb.mles[0])
    else:
        prover = A.FractionalSum(tb.mles[0], tb.mles[1])

    def device(tail=None):
        def fn():
            tr = A.Transcript(FIELD, SEED)
            fn.last = (prover.prove_device(tr, tail), tr)
        return fn

    def host():
        tr = A.Transcript(FIELD, SEED)
        host.last = (prover.prove(lambda layer, rnd, values: tr.challenge(values)), tr)
    fns = {"device": device(), "yardstick": host}
    fns.update({"tail_%d" % t: device(t) for t in SWEEP})
    times = interleaved(fns, 1 if nu >= 24 else 2)
    for fn in fns.values():
        proof, tr = fn.last
        tv = T.Transcript(p, SEED)
        ch = lambda layer, rnd, values: tv.challenge(list(values))   # noqa: E731
        if kind == "gp":
            product, layers, point = GP.decode_proof(proof, p)
            blk = 1
            for x in tb.base[0]:
                blk = blk * x % p
            assert product == pow(blk, tb.repeats, p), "product"
            ok, vpoint, claim = GP.verify(nu, product, layers, ch, p)
            assert ok and vpoint == point and tv.state == tr.state, "the model's verifier rejects"
            assert np.array_equal(tb.mles[0].evaluate(proof.point), S.encode([claim], p)[0]), "the last claim is f(point)"
        else:
            root, layers, point = FS.decode_proof(proof, p)
            pb, qb = FS.tree(list(tb.base[0]), list(tb.base[1]), p)[0]
            assert root[0] * qb % p == tb.repeats * pb * root[1] % p and root[1] == pow(qb, tb.repeats, p), "root"
            ok, vpoint, cn, cd = FS.verify(nu, True, root, layers, ch, p)
            assert ok and vpoint == point and tv.state == tr.state, "the model's verifier rejects"
            assert np.array_equal(tb.mles[0].evaluate(proof.point), S.encode([cn], p)[0]), "the last claim is num(point)"
            assert np.array_equal(tb.mles[1].evaluate(proof.point), S.encode([cd], p)[0]), "the last claim is den(point)"
    res = {"case": kind, "num_vars": nu, "reps": 1 if nu >= 24 else 2, "rounds": ROUNDS}
    res.update(times)
    nt = 3 if kind == "gp" else 5
    res["launches_of_the_sumchecks"] = sum(A.sumcheck_prove_plan(k, nt)[1] for k in range(1, nu))
    res["yardstick_calls_of_the_sumchecks"] = sum(k + 1 for k in range(1, nu))
    res["d2h_h2d_ms"] = tb.round_trip_ms(3)
    finish(res)
    return res


def run(case):
    kind, nu = case.split(":")
    nu = int(nu)
    if kind == "sweep":
        return run_sumcheck("eab", nu, SWEEP)
    return run_sumcheck(kind, nu) if kind in ("ab", "eab") else run_layered(kind, nu)


def child(args, limit):
    out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        print(out.stdout[-4000:] + out.stderr[-4000:])
        return None, out.returncode
    return json.loads(line[-1][len("RESULT "):]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck_device.json"))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    ap.add_argument("--one", default=None)
    args = ap.parse_args()
    if args.one is not None:
        print("RESULT " + json.dumps(run(args.one)), flush=True)
        return 0
    out = {"field": FIELD, "date": datetime.date.today().isoformat(),
           "timing": "wall clock per whole proof, host-observed (every route waits for its result), after one warm-up; device and "
                     "yardstick in `rounds` interleaved rounds of `reps` proofs each; yardstick = prove(challenge) with the Transcript "
                     "host entry as the callback",
           "cases": []}
    for case in args.cases.split(","):
        # a fresh process per case under its own time limit; a failure ends the run: nothing more is started on the GPU
        r, rc = child(["--one", case], args.limit)
        if r is None:
            print("case %s failed with status %d: stopping" % (case, rc))
            return 1
        out["cases"].append(r)
        print(json.dumps(r), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
