"""DevicePoints<Curve> and sw_mul of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU at n = 65; the
expected values it is handed are the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref as P
import test_point_vec_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_device_points(tmp_path):
    cname = "BLS12_381_G1"
    cid = O.CID[cname]
    fid = O.curve_info(cid)[1]
    r = P.Curve(cname).r
    n = 65
    pts = O.gen_bases(cid, H.A4, H.B4, 2 * n)
    p, q = pts[:n].copy(), pts[n:].copy()
    p[7] = 0                                                                  # an identity among the inputs
    ks = [P.from_limbs(s) for s in O.gen_scalars(fid, 65, n)]
    ks[0], ks[1], ks[64] = 0, 1, r - 1
    a, b = (P.from_limbs(s) for s in O.gen_scalars(fid, 66, 2))
    one = np.concatenate([H.jacobian(cname, np.zeros_like(p[0]))])

    def jmul(xy, k):
        return O.scalar_mul(cid, xy, H.limbs4(k % r)) if (k % r and xy.any()) else one

    want_mul = np.stack([H.oracle_mul(cname, p[i], ks[i]) for i in range(n)])
    want_fold = H.affine_of(cname, np.stack([O.point_op(cid, "jac_add", jmul(p[i], ks[i] * a), jmul(q[i], b)) for i in range(n)]))
    want_shared = np.stack([H.oracle_mul(cname, p[i], a) for i in range(n)])
    path = tmp_path / "points.bin"
    with open(path, "wb") as f:
        f.write(np.array([n], dtype=np.uint64).tobytes())
        for arr in (H.mont4(cname, a), H.mont4(cname, b), p, q, np.stack([H.mont4(cname, k) for k in ks]), want_mul, want_fold, want_shared):
            f.write(np.ascontiguousarray(arr, dtype=np.uint64).tobytes())
    exe = str(tmp_path / "points_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "points_check.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
