"""Times the point-vector entries (ark_hip_sw_mul_device / ark_hip_sw_add_device / ark_hip_sw_fold_device, csrc/pointvec.cuh) on
one GPU:

    mul, one scalar per point      out[i] = [k_i] P_i
    mul, one shared scalar         out[i] = [a] P_i
    fold                           out[i] = [a] Lo_i + [b] Hi_i on one joint doubling chain
    two mul + one add              the same result composed from the other two entries
    add                            out[i] = A_i + B_i

for BLS12-381 G1 and BN254 G1 at 2^16 and 2^20 points and BLS12-381 G2 at 2^16, next to two yardsticks from the same run: the
MSM of the same size over the same points (ark_hip_msm_sw_device), and a download plus upload of the Projective vector (what the
host loop these entries replace pays before it multiplies anything).

The G1 curves run twice: on the carry-free limbs (the default) and on saturated limbs (ARK_HIP_MSM_LAZY=0, read once per
process).  Each (curve, size, form) is a child process under its own time limit; the two forms ALTERNATE, `--repeats` children
each, and the JSON keeps every child's median next to the spread over the children (max - min of their medians).
"carry_free_is_default_by_measurement" is true for a curve when the carry-free form is faster at both sizes by more than
the larger of the two spreads.

Before anything is timed a child checks its results at the timed size: the sum of the outputs (normalize_batch on the device,
then ark_hip_msm_sw_small_device with one-bit scalars all set) must be the MSM of the same inputs, for per-point scalars,
a shared scalar and the fold.

Timing: wall clock per call between two ark_hip_synchronize(), after a warm-up call; the median over `--reps` calls.

    python tools/bench_point_vectors.py [--out profiles/point_vectors.json] [--repeats 3] [--limit 200]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

G1_JOBS = [("BLS12_381_G1", 16), ("BLS12_381_G1", 20), ("BN254_G1", 16), ("BN254_G1", 20)]
G2_JOBS = [("BLS12_381_G2", 16)]
AFFINE, PROJECTIVE = 0, 1


def run(cname, log_n, reps):
    import torch
    import algebra_amd as A
    from algebra_amd import curves as cv
    from algebra_amd._lib import check, lib
    import synth
    L = lib()
    cid = cv.curve_id(cname)
    n = 1 << log_n
    r = synth.R[cv.scalar_field(cname)]
    ab, pb = cv.affine_bytes(cid), 8 * cv.projective_words(cid)
    vp = C.c_void_p
    res = {"curve": cname, "n": n, "reps": reps, "form": "saturated" if os.environ.get("ARK_HIP_MSM_LAZY") == "0" or cname.endswith("G2")
           else "carry_free"}

    def sync():
        check(L.ark_hip_synchronize(), "sync")

    def timed(fn):
        fn()
        sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 4)

    lo = synth.grow_bases(cid, n, synth.A0, synth.B0, r)                    # Affine P_i
    hi = synth.grow_bases(cid, n, synth.A0 + 0x1234567, synth.B0 + 2, r)
    ks_host = synth.gen_scalars(n, 77, r)
    ks = torch.from_numpy(ks_host.view(np.int64)).cuda()
    a4, b4 = synth.gen_scalars(2, 78, r)
    a_dev = torch.from_numpy(a4.view(np.int64)).cuda()
    b_dev = torch.from_numpy(b4.view(np.int64)).cuda()
    out = torch.empty(n * pb, dtype=torch.uint8, device="cuda")
    tmp = torch.empty(n * pb, dtype=torch.uint8, device="cuda")
    aff = torch.empty(n * ab, dtype=torch.uint8, device="cuda")
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ap, bp = a4.ctypes.data_as(vp), b4.ctypes.data_as(vp)

    def mul(pts, form, sc, ns, dst):
        check(L.ark_hip_sw_mul_device(cid, pts.data_ptr(), form, sc.data_ptr(), ns, 0, n, dst.data_ptr()), "ark_hip_sw_mul_device")

    def add(x, y, dst):
        check(L.ark_hip_sw_add_device(cid, x.data_ptr(), y.data_ptr(), 0, n, dst.data_ptr()), "ark_hip_sw_add_device")

    def fold(dst):
        check(L.ark_hip_sw_fold_device(cid, lo.data_ptr(), hi.data_ptr(), AFFINE, ap, bp, 0, n, dst.data_ptr()), "ark_hip_sw_fold_device")

    def msm(bases, sc):
        o = np.zeros(cv.projective_words(cid), dtype=np.uint64)
        check(L.ark_hip_msm_sw_device(cid, bases.data_ptr(), sc.data_ptr(), n, 0, o.ctypes.data_as(vp)), "ark_hip_msm_sw_device")
        return o

    def sum_of(vec):
        """the sum of a Projective device vector: normalize_batch, then the one-bit MSM with every bit set"""
        check(L.ark_hip_sw_normalize_batch_device(cid, vec.data_ptr(), aff.data_ptr(), n), "normalize")
        o = np.zeros(cv.projective_words(cid), dtype=np.uint64)
        check(L.ark_hip_msm_sw_small_device(cid, aff.data_ptr(), ones.data_ptr(), n, 1, 1, o.ctypes.data_as(vp)), "msm_u1")
        return A.into_affine(cid, o)

    # ---- results at the timed size, before anything is timed ----
    a_all = torch.from_numpy(np.tile(a4, (n, 1)).view(np.int64)).cuda()
    b_all = torch.from_numpy(np.tile(b4, (n, 1)).view(np.int64)).cuda()
    torch.cuda.synchronize()
    mul(lo, AFFINE, ks, n, out)
    assert np.array_equal(sum_of(out), A.into_affine(cid, msm(lo, ks))), "sum of [k_i] P_i is not the MSM"
    mul(lo, AFFINE, a_dev, 1, out)
    m_a = msm(lo, a_all)
    assert np.array_equal(sum_of(out), A.into_affine(cid, m_a)), "sum of [a] P_i is not the MSM"
    fold(out)
    both = A.sum_projective(cid, np.stack([m_a, msm(hi, b_all)]))
    assert np.array_equal(sum_of(out), A.into_affine(cid, both)), "sum of the fold is not the sum of the two MSMs"
    fold_sum = sum_of(out)
    mul(lo, AFFINE, a_dev, 1, out)
    mul(hi, AFFINE, b_dev, 1, tmp)
    add(out, tmp, out)
    assert np.array_equal(sum_of(out), fold_sum), "two mul + add is not the fold"
    del a_all, b_all
    res["checked"] = True

    # ---- timings ----
    res["mul_per_point_ms"] = timed(lambda: mul(lo, AFFINE, ks, n, out))
    res["mul_shared_ms"] = timed(lambda: mul(lo, AFFINE, a_dev, 1, out))
    mul(lo, AFFINE, ks, n, out)                                              # a Projective vector with z != 1 for the rest
    res["mul_per_point_projective_in_place_ms"] = timed(lambda: mul(out, PROJECTIVE, ks, n, out))
    res["fold_ms"] = timed(lambda: fold(out))

    def composed():
        mul(lo, AFFINE, a_dev, 1, out)
        mul(hi, AFFINE, b_dev, 1, tmp)
        add(out, tmp, out)

    res["two_mul_one_add_ms"] = timed(composed)
    mul(lo, AFFINE, ks, n, out)
    mul(hi, AFFINE, ks, n, tmp)
    sync()
    res["add_ms"] = timed(lambda: add(out, tmp, tmp))                        # B is overwritten in place
    res["msm_ms"] = timed(lambda: msm(lo, ks))

    def round_trip():
        h = out.cpu()
        out.copy_(h, non_blocking=False)
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    res["download_upload_ms"] = timed(round_trip)
    return res


def child(cname, lg, lazy, reps, limit):
    env = dict(os.environ)
    env.pop("ARK_HIP_MSM_LAZY", None)
    if not lazy:
        env["ARK_HIP_MSM_LAZY"] = "0"
    c = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", "%s:%d" % (cname, lg),
                        "--reps", str(reps)], capture_output=True, text=True, env=env)
    line = [ln for ln in c.stdout.splitlines() if ln.startswith("RESULT ")]
    if c.returncode != 0 or not line:
        print(c.stdout[-3000:] + c.stderr[-3000:])
        print("%s 2^%d failed with status %d: stopping" % (cname, lg, c.returncode))
        return None
    return json.loads(line[-1][len("RESULT "):])


KEYS = ("mul_per_point_ms", "mul_shared_ms", "mul_per_point_projective_in_place_ms", "fold_ms", "two_mul_one_add_ms", "add_ms", "msm_ms",
        "download_upload_ms")


def summarise(runs):
    out = {"curve": runs[0]["curve"], "n": runs[0]["n"], "form": runs[0]["form"], "children": len(runs)}
    for k in KEYS:
        v = [r[k] for r in runs]
        out[k] = {"median": round(statistics.median(v), 4), "spread": round(max(v) - min(v), 4), "children": v}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_vectors.json"))
    ap.add_argument("--limit", type=int, default=200, help="seconds a child may take")
    ap.add_argument("--repeats", type=int, default=3, help="children per (curve, size, form); the two forms alternate")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per child and entry")
    ap.add_argument("--one", default=None)
    args = ap.parse_args()
    if args.one is not None:
        cname, lg = args.one.split(":")
        print("RESULT " + json.dumps(run(cname, int(lg), args.reps)), flush=True)
        return 0
    out = {"date": datetime.date.today().isoformat(),
           "timing": "wall clock per call between two ark_hip_synchronize(), after a warm-up call; median over %d calls per child; "
                     "%d children per (curve, size, form), the two forms alternating; spread = max - min of the children's medians"
                     % (args.reps, args.repeats),
           "sizes": []}
    # a fresh process per (curve, size, form) under its own time limit; a failure ends the run: nothing more is started on the GPU
    for cname, lg in G1_JOBS:
        runs = {True: [], False: []}
        for _ in range(args.repeats):
            for lazy in (True, False):
                r = child(cname, lg, lazy, args.reps, args.limit)
                if r is None:
                    return 1
                runs[lazy].append(r)
                print(json.dumps(r), flush=True)
        out["sizes"] += [summarise(runs[True]), summarise(runs[False])]
    for cname, lg in G2_JOBS:
        runs = []
        for _ in range(args.repeats):
            r = child(cname, lg, True, args.reps, args.limit)
            if r is None:
                return 1
            runs.append(r)
            print(json.dumps(r), flush=True)
        out["sizes"].append(summarise(runs))
    decision = {}
    for cname in sorted(set(c for c, _ in G1_JOBS)):
        ok = True
        for s in [s for s in out["sizes"] if s["curve"] == cname and s["form"] == "carry_free"]:
            t = [t for t in out["sizes"] if t["curve"] == cname and t["n"] == s["n"] and t["form"] == "saturated"][0]
            for k in ("mul_per_point_ms", "mul_shared_ms"):
                ok = ok and s[k]["median"] + max(s[k]["spread"], t[k]["spread"]) < t[k]["median"]
        decision[cname] = bool(ok)
    out["carry_free_is_default_by_measurement"] = decision
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
