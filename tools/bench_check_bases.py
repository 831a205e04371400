"""Times the base-set check (ark_hip_sw_check_device, csrc/pointcheck.cuh) at 2^20 and 2^22 points on all five curves and at
2^24 on BLS12-381 G1:

    checks = 1              coordinates are field elements, points on the curve
    checks = 3, method 1    ... and [r]P = O by double-and-add over the bits of r
    checks = 3, method 2    ... and phi(P) = -[x^2]P (BLS12-381 G1 only)

next to three yardsticks from the same run:

  (a) ark_hip_memcpy_d2d of the set: what reading and writing its bytes costs;
  (b) ark_hip_msm_sw_device over the same set with full-width scalars: what the set is then used for;
  (c) the oracle's scalar multiplication by r on the host cores this process is granted, extrapolated from 256 points: the
      only route there was before this entry (not for BN254 G1: cofactor one, its subgroup test is the constant true on
      the host as well).

Base sets P_i = (a + i b)G are grown on the device (tools/synth.py), so they are valid by construction; every timed result is
checked: an all-valid set gives {n, 0, 0, 0}, and a set with planted bad points (a non-element, a point off the curve, for
cofactor > 1 a curve point outside the subgroup: a random x with x^3 + b a square, y by the oracle-free square root of
tests/check_fixtures.py) gives their indices' status, the smallest index and the three counts.

Timing: wall clock per call between two ark_hip_synchronize() (the entry synchronises itself), after a warm-up call.
Products per point are counted from the formulas: a doubling is 9 base-field products (xyzz_dbl), a mixed addition 10
(xyzz_madd), the curve equation 3; an Fp2 product is counted as 3 Fp products (a square as 2) -- the multiplier work of its
two sums of two products.  "multiplier_fraction" is products / time over the Fp product rate DESIGN.md sections 4 / 9 record
for that field (profiles/r1_ubench_instruction_rates.txt: 58.7 G Fp384 products/s, 124 G Fp256 products/s).

Each size runs in a child process under its own time limit; a failure ends the run.

    python tools/bench_check_bases.py [--out profiles/check_bases.json] [--limit 240]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CURVES = ["BN254_G1", "BLS12_381_G1", "BLS12_377_G1", "BLS12_377_G2", "BLS12_381_G2"]
JOBS = [(c, lg) for lg in (20, 22) for c in CURVES] + [("BLS12_381_G1", 24)]
FP_RATE = {"BN254_G1": 124e9, "BLS12_381_G1": 58.7e9, "BLS12_377_G1": 58.7e9, "BLS12_377_G2": 58.7e9, "BLS12_381_G2": 58.7e9}
X2 = 0xd201000000010000 ** 2


def products(cname, r, checks, method):
    """base-field (Fp) products per valid point"""
    fp2 = cname.endswith("G2")
    mul, sqr = (3, 2) if fp2 else (1, 1)
    dbl = 6 * mul + 3 * sqr                         # xyzz_dbl: u^2, u v, x v, x^2, m^2, m (s - x3), w y, v zz, w zzz
    madd = 8 * mul + 2 * sqr                        # xyzz_madd: x2 zz, y2 zzz, p^2, p pp, x pp, r^2, r (q - x3), y ppp, zz pp, zzz ppp
    total = 2 * sqr + mul if checks & 1 else 0      # y^2, x^2, x^2 x
    if checks & 2 and cname != "BN254_G1":
        k = X2 if method == 2 else r
        total += (k.bit_length() - 1) * dbl + (bin(k).count("1") - 1) * madd
        if method == 2:
            total += 3 * mul                        # beta x, (beta x) zz, (-y) zzz
    return total


def timed(fn, reps):
    from algebra_amd._lib import check, lib
    fn()
    check(lib().ark_hip_synchronize(), "sync")
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    check(lib().ark_hip_synchronize(), "sync")
    return (time.perf_counter() - t0) * 1e3 / reps


def run(cname, log_n):
    import torch
    import algebra_amd as A
    from algebra_amd import curves as cv
    from algebra_amd._lib import check, lib
    import check_fixtures as CF
    import oracle_lib as O
    import point_fixtures as PF
    import synth
    L = lib()
    cid = cv.curve_id(cname)
    n = 1 << log_n
    r = synth.R[cv.scalar_field(cname)]
    ab = cv.affine_bytes(cid)
    reps = 5 if log_n <= 20 else 3 if log_n <= 22 else 2
    bases = synth.grow_bases(cid, n, synth.A0, synth.B0, r)
    res = {"curve": cname, "n": n, "reps": reps}

    def call(checks, method, status=None):
        out = (C.c_uint64 * 4)()
        check(L.ark_hip_sw_check_device(cid, bases.data_ptr(), n, checks, method, status, out), "ark_hip_sw_check_device")
        return [int(v) for v in out]

    # yardsticks (a) and (b)
    other = torch.empty(n * ab, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res["d2d_ms"] = timed(lambda: check(L.ark_hip_memcpy_d2d(other.data_ptr(), bases.data_ptr(), n * ab), "d2d"), reps)
    del other
    scalars = torch.from_numpy(synth.gen_scalars(n, 77, r).view(np.int64)).cuda()
    torch.cuda.synchronize()
    out_xyz = np.zeros(cv.projective_words(cid), dtype=np.uint64)
    res["msm_ms"] = timed(lambda: check(L.ark_hip_msm_sw_device(cid, bases.data_ptr(), scalars.data_ptr(), n, 0,
                                                                out_xyz.ctypes.data_as(C.c_void_p)), "msm"), reps)
    del scalars

    # the check, all valid
    cofactor_one = cname == "BN254_G1"               # its subgroup test is the constant true: no ladder, here or in the reference
    variants = [("on_curve", 1, 1), ("subgroup_constant_true" if cofactor_one else "subgroup_ladder", 3, 1)]
    if cname == "BLS12_381_G1":
        variants.append(("subgroup_endo", 3, 2))
    for label, checks, method in variants:
        assert call(checks, method) == [n, 0, 0, 0], label
        res[label + "_ms"] = timed(lambda: call(checks, method), reps)
        prods = products(cname, r, checks, method)
        res[label + "_products_per_point"] = prods
        res[label + "_multiplier_fraction"] = round(prods * n / (res[label + "_ms"] * 1e-3) / FP_RATE[cname], 3)
    assert call(3, 0) == [n, 0, 0, 0]

    # ... and with planted bad points: every timed variant sees them
    planted = [q for q in CF.planted(cname) if q.name in ("plus_p_0", "swapped_0", "random0", "chain3")]
    where = [n - 1, n // 2 + 129, 4097, 77][:len(planted)]
    saved = bases.view(n, ab)[torch.tensor(where, device="cuda")].clone()
    for i, q in zip(where, planted):
        bases.view(n, ab)[i] = torch.from_numpy(q.row.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for label, checks, method in variants:
        want = {i: CF.model_status(cname, q.row, checks, method) for i, q in zip(where, planted)}
        bad = sorted(i for i, s in want.items() if s)
        got = call(checks, method, status.data_ptr())
        assert got == [bad[0] if bad else n] + [sum(1 for s in want.values() if s == k) for k in (1, 2, 3)], (label, got)
        st = status.cpu().numpy()
        assert all(st[i] == s for i, s in want.items()) and int(np.count_nonzero(st)) == len(bad), label
    bases.view(n, ab)[torch.tensor(where, device="cuda")] = saved
    torch.cuda.synchronize()
    assert call(3, 0) == [n, 0, 0, 0]

    if cofactor_one:
        return res
    # yardstick (c): [r]P on the host cores granted, by the oracle, extrapolated from 256 points
    m = 256
    host = bases[:m * ab].cpu().numpy().view(np.uint64).reshape(m, -1)
    r4 = synth.limbs4(r)
    cores = max(1, min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        outs = list(ex.map(lambda row: O.scalar_mul(O.CID[cname], row, r4), host))
    dt = time.perf_counter() - t0
    fw = cv.fe_words(cid)
    assert all(not o[2 * fw:].any() for o in outs), "[r]P = O on the host too"
    res["host_cores"] = cores
    res["host_ladder_ms_extrapolated"] = round(dt * 1e3 * n / m, 1)
    best = min(res[k] for k in ("subgroup_ladder_ms", "subgroup_endo_ms") if k in res)
    res["speedup_over_host"] = round(res["host_ladder_ms_extrapolated"] / best, 1)
    if cname == "BLS12_381_G1":
        res["endo_faster_than_ladder"] = bool(res["subgroup_endo_ms"] < res["subgroup_ladder_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_bases.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--jobs", default=None, help="CURVE:LOG,... (default: every curve at 20 and 22, BLS12_381_G1 at 24)")
    ap.add_argument("--one", default=None)
    args = ap.parse_args()
    if args.one is not None:
        cname, lg = args.one.split(":")
        print("RESULT " + json.dumps(run(cname, int(lg))), flush=True)
        return 0
    jobs = JOBS if args.jobs is None else [(j.split(":")[0], int(j.split(":")[1])) for j in args.jobs.split(",")]
    out = {"date": datetime.date.today().isoformat(),
           "timing": "wall clock per call between two ark_hip_synchronize(), after a warm-up call", "sizes": []}
    for cname, lg in jobs:
        # a fresh process per size, under its own time limit; a failure ends the run: nothing more is started on the GPU
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one",
                                "%s:%d" % (cname, lg)], capture_output=True, text=True)
        line = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")]
        if child.returncode != 0 or not line:
            print(child.stdout + child.stderr)
            print("%s 2^%d failed with status %d: stopping" % (cname, lg, child.returncode))
            return 1
        r = json.loads(line[-1][len("RESULT "):])
        out["sizes"].append(r)
        print(json.dumps(r), flush=True)
    endo = [s["endo_faster_than_ladder"] for s in out["sizes"] if "endo_faster_than_ladder" in s]
    out["method_0_on_bls12_381_g1"] = 2 if endo and all(endo) else 1
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
