"""Child process of tests/test_gpu_point_vec.py: the point-vector entries under an environment that is read once per process.
    ARK_HIP_POINTVEC_SLAB_LOG=6 python tests/point_vec_child.py slabs       n = 200 in slabs of 64 lanes (fold: 32), all curves
    ARK_HIP_MSM_LAZY=0 python tests/point_vec_child.py saturated            the G1 curves on saturated limbs, n = 65 and 1000
Everything is checked against the oracle by the parent module's own checks."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O
import test_gpu_point_vec as T


def slabs():
    assert os.environ.get("ARK_HIP_POINTVEC_SLAB_LOG") == "6", "start this with ARK_HIP_POINTVEC_SLAB_LOG=6"
    T.NMAX = 200                                  # the oracle's work for 200 points, not for the parent's 1000
    for cname in O.CURVES:
        T.check_mul(cname, 200, T.AFFINE)
        T.check_mul(cname, 200, T.PROJECTIVE, shared=True, montgomery=True, in_place=True)
        T.check_fold(cname, 200, T.PROJECTIVE, in_place=True)
        T.check_fold(cname, 200, T.AFFINE, montgomery=True)
        print("ok slabs", cname, flush=True)


def saturated():
    assert os.environ.get("ARK_HIP_MSM_LAZY") == "0", "start this with ARK_HIP_MSM_LAZY=0"
    for cname in ("BN254_G1", "BLS12_381_G1", "BLS12_377_G1"):
        for n in (65, 1000):
            T.check_mul(cname, n, T.AFFINE)
            T.check_mul(cname, n, T.PROJECTIVE, shared=True, in_place=True)
            T.check_mul(cname, n, T.PROJECTIVE, montgomery=True)
            T.check_fold(cname, n, T.AFFINE)
            T.check_fold(cname, n, T.PROJECTIVE, montgomery=True, in_place=True)
        print("ok saturated", cname, flush=True)


if __name__ == "__main__":
    mode = sys.argv[1]
    {"slabs": slabs, "saturated": saturated}[mode]()
    print("point-vec-child ok " + mode, flush=True)
