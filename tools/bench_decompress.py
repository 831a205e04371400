"""Times the compressed-point codec (ark_hip_sw_decompress_device / ark_hip_sw_compress_device, csrc/pointcodec.cuh) at 2^20 and
2^22 points on all five curves and at 2^24 on BLS12-381 G1:

    decompress, validate = 0                     one square root per point
    decompress, validate = 1, method 1           ... and [r]P = O by double-and-add over r (BN254 G1: the constant true)
    decompress, validate = 1, method 2           ... and phi(P) = -[x^2]P (BLS12-381 G1 only)
    compress

next to yardsticks from the same run:

  (a) ark_hip_memcpy_d2d of the point array;
  (b) ark_hip_memcpy_h2d of the compressed bytes against that of the uncompressed points (pageable host memory);
  (c) ark_hip_sw_check_device with checks = 3 on the decompressed set;
  (d) ark_hip_msm_sw_device over it with full-width scalars;
  (e) THIS REPOSITORY'S host build of the same per-point function (ark_hip_test_host_sw_decompress) on the host cores this
      process is granted, extrapolated from 256 points.  It is not ark-serialize's speed: the host twin runs the device
      algorithm (fixed-trip-count Tonelli-Shanks, 64-bit-limb CIOS products) and exists for testing.

Base sets P_i = (a + i b)G are grown on the device (tools/synth.py) and compressed there; every timed decompression is checked:
summary {n, 0, 0, 0, 0} and points bit-identical to the set that was compressed; compress is checked against the Python model
of tests/compress_fixtures.py on sampled rows.

Products per point are counted from the formulas (csrc/codec_consts.hpp SQRT_<field>::PRODUCTS per Fp root; an Fp2 product
counts as 3 Fp products, a square as 2).  Over BLS12-377 G2 the count depends on the input (a second attempt on delta for about
half of the points): mean and worst case are both given, the fraction uses the mean.  "multiplier_fraction" is products / time
over the Fp product rate DESIGN.md sections 4 / 9 record for the field (58.7 G Fp384 products/s, 124 G Fp256 products/s).

Each size runs in a child process under its own time limit; a failure ends the run.

    python tools/bench_decompress.py [--out profiles/decompress.json] [--limit 240]
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
BASE_FIELD = {"BN254_G1": "BN254_FQ", "BLS12_381_G1": "BLS12_381_FQ", "BLS12_377_G1": "BLS12_377_FQ", "BLS12_377_G2": "BLS12_377_FQ",
              "BLS12_381_G2": "BLS12_381_FQ"}


def decompress_products(cname):
    """(mean, worst) base-field products per valid point without validation"""
    import gen_constants as G
    p, g = [(q, gen) for name, q, gen in G.FIELDS if name == BASE_FIELD[cname]][0]
    root = G.sqrt_plan(p, g)["products"]
    if not cname.endswith("G2"):
        n = 1 + 2 + root + 1                          # to_mont, x^2 and x^2 x, the root, from_mont for the larger test
        return n, n
    fixed = 2 + 2 + 3 + 1                             # to_mont (2), x^2 (2), x^2 x (3), from_mont of the deciding component
    tail = 2 + 1 + 2 + 2                              # norm (2 squares), delta / 2, c1 w / 2, the acceptance square
    if cname == "BLS12_381_G2":
        n = fixed + 2 * root + tail                   # two exponentiations, always
        return n, n
    inv = (p.bit_length() - 1) + bin(p - 2).count("1") - 1
    return fixed + 2.5 * root + inv + tail, fixed + 3 * root + inv + tail


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
    from algebra_amd import curves as cv
    from algebra_amd._lib import check, lib, test_lib
    import bench_check_bases as BC
    import compress_fixtures as X
    import point_fixtures as PF
    import synth
    L = lib()
    cid = cv.curve_id(cname)
    n = 1 << log_n
    r = synth.R[cv.scalar_field(cname)]
    ab = cv.affine_bytes(cid)
    e = L.ark_hip_sw_compressed_size(cid)
    reps = 5 if log_n <= 20 else 3 if log_n <= 22 else 2
    bases = synth.grow_bases(cid, n, synth.A0, synth.B0, r)
    res = {"curve": cname, "n": n, "reps": reps, "bytes_per_point": e}
    enc = torch.zeros(n * e, dtype=torch.uint8, device="cuda")
    dec = torch.zeros(n * ab, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def compress():
        check(L.ark_hip_sw_compress_device(cid, bases.data_ptr(), n, enc.data_ptr()), "ark_hip_sw_compress_device")

    def decompress(validate, method):
        out = (C.c_uint64 * 5)()
        check(L.ark_hip_sw_decompress_device(cid, enc.data_ptr(), n, validate, method, dec.data_ptr(), None, out),
              "ark_hip_sw_decompress_device")
        return [int(v) for v in out]

    res["compress_ms"] = timed(compress, reps)
    cvp = PF.curve(cname)
    for i in (0, 1, n // 2 + 129, n - 1):             # compress against the model
        row = bases[i * ab:(i + 1) * ab].cpu().numpy().view(np.uint64)
        assert enc[i * e:(i + 1) * e].cpu().numpy().tobytes() == X.encode(cname, cvp.dec(row)), i

    mean, worst = decompress_products(cname)
    res["decompress_products_per_point"] = round(mean, 1)
    res["decompress_products_per_point_worst"] = worst
    cofactor_one = cname == "BN254_G1"
    variants = [("decompress", 0, 0), ("decompress_validate_constant_true" if cofactor_one else "decompress_validate_ladder", 1, 1)]
    if cname == "BLS12_381_G1":
        variants.append(("decompress_validate_endo", 1, 2))
    for label, validate, method in variants:
        dec.zero_()
        torch.cuda.synchronize()
        assert decompress(validate, method) == [n, 0, 0, 0, 0], label
        assert torch.equal(dec, bases), label          # every timed variant: all ok, the very points that were compressed
        res[label + "_ms"] = timed(lambda: decompress(validate, method), reps)
        prods = mean + (BC.products(cname, r, 2, method) if validate else 0)
        res[label + "_products_per_point"] = round(prods, 1)
        res[label + "_multiplier_fraction"] = round(prods * n / (res[label + "_ms"] * 1e-3) / FP_RATE[cname], 3)
    assert decompress(1, 0) == [n, 0, 0, 0, 0]

    # yardsticks
    other = torch.empty(n * ab, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res["d2d_points_ms"] = timed(lambda: check(L.ark_hip_memcpy_d2d(other.data_ptr(), dec.data_ptr(), n * ab), "d2d"), reps)
    host_enc, host_pts = enc.cpu().numpy(), dec.cpu().numpy()
    res["h2d_compressed_ms"] = timed(lambda: check(L.ark_hip_memcpy_h2d(other.data_ptr(), host_enc.ctypes.data_as(C.c_void_p), n * e), "h2d"), reps)
    res["h2d_uncompressed_ms"] = timed(lambda: check(L.ark_hip_memcpy_h2d(other.data_ptr(), host_pts.ctypes.data_as(C.c_void_p), n * ab), "h2d"), reps)
    del other, host_pts

    def sw_check():
        out = (C.c_uint64 * 4)()
        check(L.ark_hip_sw_check_device(cid, dec.data_ptr(), n, 3, 0, None, out), "ark_hip_sw_check_device")
        assert [int(v) for v in out] == [n, 0, 0, 0]

    res["sw_check_3_ms"] = timed(sw_check, reps)
    scalars = torch.from_numpy(synth.gen_scalars(n, 77, r).view(np.int64)).cuda()
    torch.cuda.synchronize()
    out_xyz = np.zeros(cv.projective_words(cid), dtype=np.uint64)
    res["msm_ms"] = timed(lambda: check(L.ark_hip_msm_sw_device(cid, dec.data_ptr(), scalars.data_ptr(), n, 0,
                                                                out_xyz.ctypes.data_as(C.c_void_p)), "msm"), reps)
    del scalars

    # (e) this repository's host twin on the granted cores, extrapolated from 256 points
    m = 256
    cores = max(1, min(16, len(os.sched_getaffinity(0))))
    T = test_lib()
    want = host_enc[:m * e].reshape(m, e)
    for label, validate in (("host_twin_decompress", 0), ("host_twin_decompress_validate", 1)):
        pts = np.zeros((m, ab // 8), dtype=np.uint64)

        def one(i):
            return T.ark_hip_test_host_sw_decompress(cid, want[i].ctypes.data_as(C.c_void_p), 1, validate, 0,
                                                     pts[i].ctypes.data_as(C.c_void_p), None)

        t0 = time.perf_counter()
        with ThreadPoolExecutor(cores) as ex:
            rcs = list(ex.map(one, range(m)))
        dt = time.perf_counter() - t0
        assert not any(rcs) and pts.tobytes() == bases[:m * ab].cpu().numpy().tobytes(), label
        res[label + "_ms_extrapolated"] = round(dt * 1e3 * n / m, 1)
    res["host_cores"] = cores
    res["host_twin_is"] = "this repository's own per-point function built for the host, not ark-serialize"
    best = min(v for k, v in res.items() if k.startswith("decompress_validate") and k.endswith("_ms"))
    res["speedup_over_host_twin_validate"] = round(res["host_twin_decompress_validate_ms_extrapolated"] / best, 1)
    res["speedup_over_host_twin"] = round(res["host_twin_decompress_ms_extrapolated"] / res["decompress_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decompress.json"))
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
        with open(args.out, "w") as f:               # written after every size: a later failure keeps what was measured
            json.dump(out, f, indent=1)
            f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
