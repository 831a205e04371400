"""The polynomial operations of the C++ mirror (include/ark_hip.hpp: DeviceVec::evaluate / divide_by_linear /
divide_by_vanishing_poly / inner_product, Radix2EvaluationDomain::evaluate_all_lagrange_coefficients) from a compiled C++
program on the GPU at 2^16; the expected values it is handed are computed here with Python big integers."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_poly_ops(tmp_path):
    fname = "BLS12_381_FR"
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    n = 1 << 16
    coeffs = [pyref.from_limbs(row) for row in O.gen_scalars(fid, 41, n, montgomery=True)]   # Montgomery residues as integers
    rinv = pow(pyref.R_of(p), -1, p)
    rng = np.random.default_rng(4242)
    z, s, tau = (int.from_bytes(rng.bytes(40), "little") % p for _ in range(3))

    def horner(x):   # (a R) rides along: the result is p(x) R, the Montgomery form of the value
        acc = 0
        for c in reversed(coeffs):
            acc = (acc * x + c) % p
        return acc

    g = pyref.root_of_unity(fname, 16)
    zh = (pow(tau, n, p) - 1) % p

    def lagrange(i):   # Z_H(tau) g^i / (n (tau - g^i))
        gi = pow(g, i, p)
        return zh * gi % p * pow(n * (tau - gi) % p, -1, p) % p

    mont = lambda x: x * pyref.R_of(p) % p                      # noqa: E731
    args = [mont(z), mont(s), mont(tau), horner(z), horner(s), horner(tau), mont(lagrange(0)), mont(lagrange(n - 1))]
    assert horner(1) * rinv % p == sum(coeffs) * rinv % p       # the reference's own sanity
    exe = str(tmp_path / "poly_ops_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "poly_ops_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    out = subprocess.run([exe] + ["%064x" % v for v in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
