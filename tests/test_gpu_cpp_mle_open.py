"""eq, quotients and open of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU at 9 variables, on
each scalar field with its G1; the expected values it is handed are computed here with Python big integers
(tests/mle_ref.py, tests/mle_open_ref.py), the rest it checks against the oracle itself."""
import os
import subprocess

import numpy as np
import pytest

import mle_open_ref as R
import mle_ref
import oracle_lib as O
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NV = 9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mle_open") / "mle_open_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "mle_open_check.cpp"), "-o", path,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    return path


@pytest.mark.parametrize("field,fname", [("bn254", "BN254_FR"), ("bls12_381", "BLS12_381_FR"), ("bls12_377", "BLS12_377_FR")])
def test_cpp_mle_open(exe, field, fname):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    Rm = pyref.R_of(p)
    table = mle_ref.ints(O.gen_scalars(fid, 47, 1 << NV, montgomery=True))   # Montgomery residues as integers: R rides along
    rng = np.random.default_rng(909)
    r = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(NV)]
    scale = int.from_bytes(rng.bytes(40), "little") % p
    value, _ = R.quotients(table, r, p)
    assert value == mle_ref.evaluate(table, r, p)
    eq = R.eq_table_mont(r, scale, p, Rm)
    args = [value, eq[0], eq[-1], scale * Rm % p] + [x * Rm % p for x in r]
    out = subprocess.run([exe, field] + ["%064x" % v for v in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
