"""fraction_tree, count_indices and FractionalSum::prove of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on
the GPU at 9 variables over BLS12-381 Fr; the expected values it is handed are computed here with Python big integers
(tests/fraction_sum_ref.py), the rest it checks against the oracle's arithmetic itself."""
import os
import subprocess

import pytest

import fraction_sum_ref as R
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NV = 9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fraction_sum") / "fraction_sum_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "fraction_sum_check.cpp"), "-o", path,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    return path


def test_cpp_fraction_sum(exe):
    fname = "BLS12_381_FR"
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    num = S.decode(O.gen_scalars(fid, 71, 1 << NV, montgomery=True), p)
    den = S.decode(O.gen_scalars(fid, 72, 1 << NV, montgomery=True), p)
    answers = iter(S.decode(O.gen_scalars(fid, 73, 64, montgomery=True), p))     # the challenges in the order they are asked for
    root, layers, point = R.prove(num, den, lambda layer, rnd, values: next(answers), p)
    replay = iter(S.decode(O.gen_scalars(fid, 73, 64, montgomery=True), p))
    ok, vpoint, cn, cd = R.verify(NV, True, root, layers, lambda layer, rnd, values: next(replay), p)
    assert ok and vpoint == point and cn == mle_ref.evaluate(num, point, p) and cd == mle_ref.evaluate(den, point, p)
    args = [mle_ref.ints(S.encode([v], p))[0] for v in root + tuple(layers[-1][1]) + (cn, cd)]
    out = subprocess.run([exe] + ["%064x" % v for v in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
