"""Times the FRI fold, the commit phase and the combination of columns (ark_hip_fri_*, ark_hip_xfp_*) on device-resident data, by
the method of tools/bench_small_fft.py, next to yardsticks measured in the same run:

  fold (2^20 and 2^24 extension elements, BabyBear and Goldilocks, log-arity 1 and 3)
    (a) the composed route a caller had before for ONE 2-fold: ark_hip_sfp_add / sub / scale / mul_device on component columns with
        temporaries, the twiddle vector (2 h w^i)^-1 prebuilt and not timed (16 launches at d = 2, 48 at d = 4);
    (b) ark_hip_memcpy_d2d of the bytes the fold moves (it reads the layer and writes 2^-a of it; a copy of B bytes moves 2 B);
    (c) the download plus upload of the layer through pinned host memory.
  commit phase (2^20, log-arity 1 and 3, down to 2^5 or below)
    against the sum of its commits and folds timed alone (what the per-layer waits cost) and the download of layer 0.
  combine: 64 columns of 2^20 against 64 x (scale + add) per component on the base-field entries, and a copy of the matrix.

`accepted`: the fused 2-fold is faster than the composed route by more than the two recorded spreads at both sizes and both
fields.  Every timed result is checked first at sampled positions against the model of tests/fri_ref.py; the composed route
against the fused fold word for word.

    python tools/bench_fri.py [--out profiles/fri.json] [--logs 20,24] [--quick]
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
import fri_ref as X  # noqa: E402

ROUNDS = 5


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


def dt(x):
    return np.uint64 if x.bytes == 8 else np.uint32


def elem4(e):
    a = (C.c_uint64 * 4)()
    for k, v in enumerate(e):
        a[k] = int(v)
    return a


def random_ext(x, n, rng):
    return A.SmallExtVec.from_host(x.name, rng.integers(0, x.p, size=(x.d, n), dtype=np.uint64).astype(dt(x)))


def put(row, t):
    for k, (med, spread) in t.items():
        row[k + "_ms"], row[k + "_spread_ms"] = med, spread


class Composed:
    """one 2-fold from the base-field pointwise entries: per component s = (lo + hi) / 2 and e = (lo - hi) * tw, then
    out_c = s_c + sum_k M[c][k] e_k with M the matrix of the multiplication by beta"""

    def __init__(self, x, vin, dom, beta):
        self.x, self.vin, self.half = x, vin, vin.n // 2
        L = lib()
        h = self.half
        # tw[i] = (2 h w^i)^-1: 1 / (2 offset) times the powers of group_gen_inv, built once by scale calls on a doubling prefix
        tw = np.empty(h, dtype=dt(x))
        cur = x.st(pow(2 * x.pl(dom.coset_offset()), x.p - 2, x.p))
        tw[0] = cur
        self.tw = A.SmallDeviceVec.from_host(x.name, tw)
        filled, gi = 1, dom.group_gen_inv()
        step = gi
        while filled < h:       # tw[filled : 2 filled] = tw[0 : filled] * gi^filled
            check(L.ark_hip_sfp_scale_device(x.sid, self.tw._p, step, C.c_void_p(self.tw.ptr + filled * x.bytes), filled), "scale")
            step = A.small_field_pow(x.name, step, 2)
            filled *= 2
        self.inv2 = x.st(pow(2, x.p - 2, x.p))
        basis = [tuple(x.st(1) if j == k else 0 for j in range(x.d)) for k in range(x.d)]
        cols = [A.ext_mul(x.name, beta, e) for e in basis]          # column k = beta * e_k
        self.m = [[cols[k][c] for k in range(x.d)] for c in range(x.d)]
        self.s = A.SmallExtVec(x.name, h)
        self.e = A.SmallExtVec(x.name, h)
        self.tmp = A.SmallDeviceVec(x.name, h)
        self.out = A.SmallExtVec(x.name, h)

    def comp(self, v, k, off=0):
        return C.c_void_p(v.ptr + (k * v.stride + off) * self.x.bytes)

    def run(self):
        L, x, h = lib(), self.x, self.half
        sid = x.sid
        for k in range(x.d):
            lo, hi = self.comp(self.vin, k), self.comp(self.vin, k, h)
            check(L.ark_hip_sfp_add_device(sid, lo, hi, self.comp(self.s, k), h), "add")
            check(L.ark_hip_sfp_scale_device(sid, self.comp(self.s, k), self.inv2, self.comp(self.s, k), h), "scale")
            check(L.ark_hip_sfp_sub_device(sid, lo, hi, self.comp(self.e, k), h), "sub")
            check(L.ark_hip_sfp_mul_device(sid, self.comp(self.e, k), self.tw._p, self.comp(self.e, k), h), "mul")
        for c in range(x.d):
            o = self.comp(self.out, c)
            check(L.ark_hip_sfp_scale_device(sid, self.comp(self.e, 0), self.m[c][0], o, h), "scale")
            for k in range(1, x.d):
                check(L.ark_hip_sfp_scale_device(sid, self.comp(self.e, k), self.m[c][k], self.tmp._p, h), "scale")
                check(L.ark_hip_sfp_add_device(sid, o, self.tmp._p, o, h), "add")
            check(L.ark_hip_sfp_add_device(sid, o, self.comp(self.s, c), o, h), "add")

    launches = property(lambda self: 4 * self.x.d + self.x.d * (2 * self.x.d - 1) + self.x.d)


def check_fold(x, k, a, h, host_in, out_vec, beta, rng):
    m = 1 << (k - a)
    got = out_vec.to_host()
    w = x.omega(k)
    for i in [0, m - 1] + [int(v) for v in rng.integers(0, m, size=14)]:
        row = [tuple(x.pl(int(host_in[c, i + j * m])) for c in range(x.d)) for j in range(1 << a)]
        want = x.stored(x._fold_small(row, a, h * pow(w, i, x.p) % x.p, x.plain(beta)))
        assert tuple(int(got[c, i]) for c in range(x.d)) == want, (x.name, k, a, i)


def bench_fold(x, log_n, rng):
    L = lib()
    n = 1 << log_n
    reps = 50 if log_n <= 20 else 10
    dom = A.SmallRadix2EvaluationDomain.new(x.name, n).get_coset(x.st(x.gen))
    vin = random_ext(x, n, rng)
    host_in = vin.to_host()
    beta = tuple(int(v) for v in rng.integers(1, x.p, size=x.d, dtype=np.uint64))
    layer_bytes = x.d * n * x.bytes
    row = {"field": x.name, "log_n": log_n, "reps": reps, "rounds": ROUNDS, "layer_bytes": layer_bytes}
    outs = {a: A.SmallExtVec(x.name, n >> a) for a in (1, 3)}
    for a in (1, 3):
        A.fri_fold(vin, dom, a, beta, out=outs[a])
        check_fold(x, log_n, a, x.gen, host_in, outs[a], beta, rng)
    comp = Composed(x, vin, dom, beta)
    comp.run()
    assert np.array_equal(comp.out.to_host(), outs[1].to_host()), (x.name, log_n, "the composed route is not the fold")
    scratch = A.SmallDeviceVec(x.name, x.d * n)
    pin = C.c_void_p()
    check(L.ark_hip_host_alloc(layer_bytes, C.byref(pin)), "host_alloc")

    def down_up():
        check(L.ark_hip_memcpy_d2h(pin, vin._p, layer_bytes), "d2h")
        check(L.ark_hip_memcpy_h2d(scratch._p, pin, layer_bytes), "h2d")

    moved = {a: layer_bytes + (layer_bytes >> a) for a in (1, 3)}
    t = rounds({
        "fold_a1": lambda: A.fri_fold(vin, dom, 1, beta, out=outs[1]),
        "fold_a3": lambda: A.fri_fold(vin, dom, 3, beta, out=outs[3]),
        "composed_2fold": comp.run,
        "copy_a1": lambda: check(L.ark_hip_memcpy_d2d(scratch._p, vin._p, moved[1] // 2), "d2d"),
        "copy_a3": lambda: check(L.ark_hip_memcpy_d2d(scratch._p, vin._p, moved[3] // 2), "d2d"),
    }, reps)
    t.update(rounds({"download_upload": down_up}, max(2, reps // 10), warm=1))
    check(L.ark_hip_host_free(pin), "host_free")
    put(row, t)
    row["composed_launches"] = comp.launches
    row["composed_over_fused"] = round(t["composed_2fold"][0] / t["fold_a1"][0], 2)
    row["fold_a1_times_copy"] = round(t["fold_a1"][0] / t["copy_a1"][0], 2)
    row["fold_a3_times_copy"] = round(t["fold_a3"][0] / t["copy_a3"][0], 2)
    row["fold_a1_gb_per_s"] = round(moved[1] / t["fold_a1"][0] / 1e6, 1)
    row["fold_a3_gb_per_s"] = round(moved[3] / t["fold_a3"][0] / 1e6, 1)
    row["fused_faster_beyond_spreads"] = bool(t["composed_2fold"][0] - t["fold_a1"][0] > t["composed_2fold"][1] + t["fold_a1"][1])
    print(json.dumps(row), flush=True)
    return row


def bench_commit_phase(x, log_n, a, rng):
    L = lib()
    n = 1 << log_n
    num_folds = (log_n - 5 + a - 1) // a
    dom = A.SmallRadix2EvaluationDomain.new(x.name, n).get_coset(x.st(x.gen))
    vin = random_ext(x, n, rng)
    prover = A.FriProver(vin, dom, a, num_folds)
    challenge = lambda: X.shake_challenge(x, [])   # noqa: E731
    prover.commit_phase(challenge())
    per_layer = prover.query([0, n - 1, 12345, n // 2 + 7])
    for q, index in enumerate([0, n - 1, 12345, n // 2 + 7]):
        mo = [(rows[q].tolist(), [bytes(pp) for pp in paths[q]]) for _, rows, paths in per_layer]
        assert x.verify_query(log_n, x.gen, a, num_folds, prover.roots, prover.betas, prover.final_poly.tolist(), index, mo), (x.name, a, q)
    betas, doms = prover.betas, prover.domains
    lays = prover.plan["layers"]

    def alone():     # the same commits and folds, queued without a wait between them
        for l in range(num_folds):
            al, rows = lays[l]["log_arity"], 1 << (lays[l]["log_size"] - lays[l]["log_arity"])
            tree = C.c_void_p(prover._trees.value + lays[l]["tree_offset"])
            check(L.ark_hip_merkle_commit_sfp_device(x.sid, C.c_void_p(prover.layer_ptr(l)), x.d << al, rows, rows, tree, None), "commit")
            check(L.ark_hip_fri_fold(x.sid, C.byref(doms[l]._s), al, elem4(betas[l]), C.c_void_p(prover.layer_ptr(l)), 1 << lays[l]["log_size"],
                                     C.c_void_p(prover.layer_ptr(l + 1)), rows), "fold")

    pin = C.c_void_p()
    nbytes = x.d * n * x.bytes
    check(L.ark_hip_host_alloc(nbytes, C.byref(pin)), "host_alloc")
    t = rounds({
        "commit_phase": lambda: prover.commit_phase(challenge()),
        "commits_and_folds_queued": alone,
        "download_layer0": lambda: check(L.ark_hip_memcpy_d2h(pin, vin._p, nbytes), "d2h"),
    }, 5)
    check(L.ark_hip_host_free(pin), "host_free")
    row = {"field": x.name, "log_n": log_n, "log_arity": a, "num_folds": num_folds, "final_size": prover.plan["final_size"]}
    put(row, t)
    row["waits_and_final_ms"] = round(t["commit_phase"][0] - t["commits_and_folds_queued"][0], 5)
    row["per_layer_wait_ms"] = round(row["waits_and_final_ms"] / num_folds, 5)
    print(json.dumps(row), flush=True)
    prover.free()
    return row


def bench_combine(x, rng, quick):
    L = lib()
    count, rows = (8, 1 << 12) if quick else (64, 1 << 20)
    host = rng.integers(0, x.p, size=(count, rows), dtype=np.uint64).astype(dt(x))
    mat = A.SmallDeviceMatrix.from_host(x.name, host)
    alpha = tuple(int(v) for v in rng.integers(1, x.p, size=x.d, dtype=np.uint64))
    out = A.combine_columns(mat, rows, alpha)
    got = out.to_host()
    pa = x.plain(alpha)
    for i in [0, rows - 1] + [int(v) for v in rng.integers(0, rows, size=6)]:
        want = x.stored(x.combine([[x.pl(int(host[j, i]))] for j in range(count)], pa)[0])
        assert tuple(int(got[c, i]) for c in range(x.d)) == want, (x.name, "combine", i)
    pws = [tuple(x.st(1) if c == 0 else 0 for c in range(x.d))]
    for _ in range(count - 1):
        pws.append(A.ext_mul(x.name, pws[-1], alpha))
    acc, tmp, other = A.SmallExtVec(x.name, rows), A.SmallDeviceVec(x.name, rows), A.SmallDeviceVec(x.name, count * rows)

    def composed():
        for j in range(count):
            col = C.c_void_p(mat.vec.ptr + j * rows * x.bytes)
            for c in range(x.d):
                o = C.c_void_p(acc.ptr + c * rows * x.bytes)
                if j == 0:
                    check(L.ark_hip_sfp_scale_device(x.sid, col, pws[j][c], o, rows), "scale")
                else:
                    check(L.ark_hip_sfp_scale_device(x.sid, col, pws[j][c], tmp._p, rows), "scale")
                    check(L.ark_hip_sfp_add_device(x.sid, o, tmp._p, o, rows), "add")

    composed()
    assert np.array_equal(acc.to_host(), got), (x.name, "the composed combination is not the fused one")
    t = rounds({
        "combine": lambda: A.combine_columns(mat, rows, alpha, out=out),
        "composed_scale_add": composed,
        "copy_matrix": lambda: check(L.ark_hip_memcpy_d2d(other._p, mat.vec._p, count * rows * x.bytes), "d2d"),
    }, 5)
    row = {"field": x.name, "columns": count, "rows": rows}
    put(row, t)
    row["combine_times_copy"] = round(t["combine"][0] / t["copy_matrix"][0], 2)
    row["composed_over_fused"] = round(t["composed_scale_add"][0] / t["combine"][0], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri.json"))
    ap.add_argument("--logs", default="20,24")
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    logs = [12, 14] if args.quick else [int(v) for v in args.logs.split(",")]
    rng = np.random.default_rng(30)
    out = {"date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; median and spread "
                     "(max - min) of `rounds` interleaved rounds; device-resident data",
           "quick": bool(args.quick), "fold": [], "commit_phase": [], "combine": []}
    for name in ("BABYBEAR", "GOLDILOCKS"):
        x = X.FIELDS[name]
        for log_n in logs:
            out["fold"].append(bench_fold(x, log_n, rng))
        for a in (1, 3):
            out["commit_phase"].append(bench_commit_phase(x, min(logs[0], 20), a, rng))
        out["combine"].append(bench_combine(x, rng, args.quick))
    out["accepted"] = all(r["fused_faster_beyond_spreads"] for r in out["fold"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out, "accepted:", out["accepted"])


if __name__ == "__main__":
    main()
