"""product_tree, linear_combination and GrandProduct::prove of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program
on the GPU at 9 variables over BLS12-381 Fr; the expected values it is handed are computed here with Python big integers
(tests/grand_product_ref.py), the rest it checks against the oracle's arithmetic itself."""
import os
import subprocess

import pytest

import grand_product_ref as R
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NV = 9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("grand_product") / "grand_product_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "grand_product_check.cpp"), "-o", path,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    return path


def test_cpp_grand_product(exe):
    fname = "BLS12_381_FR"
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    table = S.decode(O.gen_scalars(fid, 61, 1 << NV, montgomery=True), p)
    answers = iter(S.decode(O.gen_scalars(fid, 62, 64, montgomery=True), p))     # the challenges in the order they are asked for
    product, layers, point = R.prove(table, lambda layer, rnd, values: next(answers), p)
    replay = iter(S.decode(O.gen_scalars(fid, 62, 64, montgomery=True), p))
    ok, vpoint, claim = R.verify(NV, product, layers, lambda layer, rnd, values: next(replay), p)
    assert ok and vpoint == point and claim == mle_ref.evaluate(table, point, p)
    left, right = layers[-1][1]
    args = [mle_ref.ints(S.encode([v], p))[0] for v in (product, left, right, claim)]
    out = subprocess.run([exe] + ["%064x" % v for v in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
