"""Child process of tests/test_gpu_point_arrays.py: batch_mul and the MSM with ARK_HIP_MSM_LAZY=0 in the environment this
process was started with (msm_lazy_enabled() reads it once per process), everything checked against the oracle.
    ARK_HIP_MSM_LAZY=0 python tests/msm_saturated_child.py

What the switch replaces, and which input below reaches it:

  batchmul_run (batchmul.cuh:155)     batchmul_lazy_kernel<C> -> batchmul_kernel<C> on the three G1 curves (G2 always runs the
                                      latter).  Reached by batch_mul() below: about 700 scalars per G1 curve, among them 0, 1,
                                      r - 1, 2^256 - 1 and the unreduced scalar whose lower rows add up to the top row's entry,
                                      where the plain xyzz_madd must double.
  msm_run, plain path (msm.cuh,       msm_accumulate_lazy_kernel<C>, or msm_accumulate_parts_kernel<C> + msm_sum_parts_kernel<C>
   MsmCall::accumulate_group)         when a run is walked by several lanes, -> msm_accumulate_kernel<C>, on every curve.
                                      Reached by every plain MSM below: the random vectors at n = 33, 1000, 4096, the edge
                                      cases (identity bases, P with P and P with -P in one bucket, one bucket per window),
                                      every base twice (the mixed addition's doubling branch in most buckets, msm_u16
                                      included) and thousands of copies of one base (the run of a lane-per-bucket lane
                                      holds the same point again and again; the heavy-run kernels are not switched).
  msm_run, prepared set (the same)    msm_accumulate_shared_lazy_kernel<C> -> msm_accumulate_shared_kernel<C>.  Reached by the
                                      PreparedBases runs of "every base twice" and "identical bases".
  the plan (msm_plan.hpp)             msm_default_plan: msm_make_plan(..., split_runs = false): between 256 and 73 728 pairs (G2: 24 576,
                                      BLS12-377 G1: 20 480) the plain path no longer takes the narrow windows that count on
                                      split runs but the model's own width, so n = 1000 and 4096 run another window layout
                                      than in the parent process.  plan() below checks that ark_hip_msm_plan reports the
                                      model's choice: the same (c, W) as for a prepared == 0 plan with the small-split rule off.

None of these needs a larger n: every replaced kernel is launched by any MSM of its path, whatever the size."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import algebra_amd as A
import oracle_lib as O
import pyref as P
import test_gpu_msm as M
from test_gpu_msm_prepared import unreduced_doubling_scalar

G1 = ("BN254_G1", "BLS12_381_G1", "BLS12_377_G1")


def batch_mul():
    for cname in G1:
        cid = O.CID[cname]
        fid = O.curve_info(cid)[1]
        r = P.Curve(cname).r
        n = 700
        canon = O.gen_scalars(fid, 0x5A7, n)
        planted = {0: 0, 1: 1, 2: r - 1, 127: unreduced_doubling_scalar(r), 128: (1 << 256) - 1, n - 1: unreduced_doubling_scalar(r)}
        for i, v in planted.items():
            canon[i] = P.to_limbs(v, 4)
        base = O.scalar_mul(cid, O.generator(cid), np.array([0x5EED, 0, 0, 0], dtype=np.uint64))
        baff = O.to_affine(cid, base)
        # the oracle's batch_mul for the reduced scalars, its scalar_mul of v mod r for the two that are not
        red = canon.copy()
        for i, v in planted.items():
            red[i] = P.to_limbs(v % r, 4)
        exp = O.batch_mul(cid, base, red)
        for i, v in planted.items():
            assert np.array_equal(exp[i], O.to_affine(cid, O.scalar_mul(cid, baff, P.to_limbs(v % r, 4)))), (cname, i)
        assert not exp[0].any() and np.array_equal(exp[1], baff)
        t = A.BatchMulPreprocessing(cid, base, n)
        got = t.batch_mul(canon, montgomery=False)
        t.free()
        assert np.array_equal(got, exp), (cname, np.flatnonzero((got != exp).any(axis=1))[:8])
        print("ok batch_mul", cname, flush=True)


def plan():
    # with the switch off the plain plan is the model's own: the narrow-window rule for small MSMs is not applied
    for cname in O.CURVES:
        cid = O.CID[cname]
        for n in (1000, 4096):
            c, W = A.msm_plan(cid, n)
            assert c > (10 if n == 4096 else 8), (cname, n, c, W)     # the split-run rule would give log2(n) - 2
    print("ok plan", flush=True)


def msm():
    for cname in O.CURVES:
        for n in (33, 1000, 1 << 12):
            M.test_msm_random_matches_oracle(cname, n)
        M.test_msm_edge_cases(cname)
        M.test_msm_every_base_twice_doubles_in_most_buckets(cname)
        M.test_msm_identical_bases_in_heavy_buckets(cname)
        print("ok msm", cname, flush=True)


if __name__ == "__main__":
    assert os.environ.get("ARK_HIP_MSM_LAZY") == "0", "start this with ARK_HIP_MSM_LAZY=0"
    batch_mul()
    plan()
    msm()
    print("saturated-kernels ok", flush=True)
