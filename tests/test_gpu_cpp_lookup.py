"""lookup and lookup_plan of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU: the single-column lookup
of tests/test_gpu_lookup.py (2^9 witness cells in 2^6 table values over BLS12-381 Fr, seeds from fraction_sum_ref.lookup_case)
end to end without an index array.  The table side's root it is handed is computed here with Python big integers
(tests/fraction_sum_ref.py); indices, counts and products it checks itself against a host join and the oracle's arithmetic."""
import os
import subprocess

import pytest

import fraction_sum_ref as R
import mle_ref
import pyref
import sumcheck_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lookup") / "lookup_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "lookup_check.cpp"), "-o", path,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    return path


def test_cpp_lookup(exe, tmp_path):
    fname = "BLS12_381_FR"
    p = pyref.MODULI[fname][0]
    t, idx, gamma, outside = R.lookup_case(p)
    m = R.counts([int(i) for i in idx], 64)
    root, _, _ = R.tree(m, [(gamma + v) % p for v in t], p)
    hexes = ["%064x" % v for v in mle_ref.ints(S.encode([gamma, outside] + t + list(root), p))]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(hexes[:66] + [str(int(i)) for i in idx]) + "\n")
    out = subprocess.run([exe, str(case)] + hexes[66:], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
