"""The DenseMultilinearExtension of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU at 13
variables; the expected values it is handed are computed here with Python big integers (tests/mle_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import mle_ref
import oracle_lib as O
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_mle(tmp_path):
    fname = "BLS12_381_FR"
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    nv, dim = 13, 5
    table = mle_ref.ints(O.gen_scalars(fid, 43, 1 << nv, montgomery=True))   # Montgomery residues as integers: R rides along
    rng = np.random.default_rng(1313)
    r = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(nv)]
    f = int.from_bytes(rng.bytes(40), "little") % p
    value = mle_ref.evaluate(table, r, p)
    fixed = mle_ref.fix_variables(table, r[:dim], p)
    rs = list(r)
    for i in range(3):
        rs[2 + i], rs[8 + i] = rs[8 + i], rs[2 + i]
    relabelled = mle_ref.evaluate(mle_ref.relabel(table, 2, 8, 3), rs, p)
    assert relabelled == value                                              # the reference's own sanity (dense.rs:507-542)
    axpy = mle_ref.evaluate([(u + f * v) % p for u, v in zip(table, reversed(table))], r, p)
    mont = lambda x: x * pyref.R_of(p) % p                                  # noqa: E731
    args = [value, fixed[0], fixed[-1], relabelled, axpy, mont(f)] + [mont(x) for x in r]
    exe = str(tmp_path / "mle_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "mle_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    out = subprocess.run([exe] + ["%064x" % v for v in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
