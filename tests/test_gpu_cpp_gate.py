"""SumOfProducts and DeviceVec::rotate of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU, on one
mixed expression -- a repeated column, a general coefficient, rotations 4, -1 and INT64_MIN, a constant; the vectors it is
handed are computed here with Python big integers (tests/gate_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import gate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_gate(tmp_path):
    f = R.Field("BLS12_381_FR")
    n = 777
    a, b, c = (R.planted(f, n, 900 + k) for k in range(3))
    k, c0 = R.rand_elems(f, 2, 903)
    terms = [(k, [(0, 0), (1, 4), (0, 0)]), (None, [(2, -1)]), (k, [(1, -(1 << 63)), (2, 0)])]
    want = R.sum_of_products(f, [a, b, c], n, terms, c0)
    plain = R.sum_of_products(f, [a, b, c], n, terms)
    assert want != plain and len(set(want)) > n // 2
    np.array([n], dtype="<u8").tofile(str(tmp_path / "dims.bin"))
    for part, elems in (("a", a), ("b", b), ("c", c), ("k", [k]), ("c0", [c0]), ("want", want), ("plain", plain),
                        ("rot", a[-3:] + a[:-3])):
        R.limbs(elems).astype("<u8").tofile(str(tmp_path / (part + ".bin")))
    exe = str(tmp_path / "gate_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gate_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
