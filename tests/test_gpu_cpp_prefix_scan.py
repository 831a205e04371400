"""The prefix scans of the C++ mirror (include/ark_hip.hpp: DeviceVec::prefix_product / prefix_sum / prefix_ratio) from a
compiled C++ program on the GPU at tile + 1 elements; the vectors it is handed are computed here with Python big integers
(tests/prefix_scan_ref.py)."""
import os
import subprocess

import pytest

import algebra_amd as A
import oracle_lib as O
import prefix_scan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_prefix_scan(tmp_path):
    fname = "BLS12_381_FR"
    f = R.Field(fname)
    n = A.prefix_scan_plan("product", 0)[0] + 1
    a = O.gen_scalars(O.FID[fname], 61, n, montgomery=True)
    b = O.gen_scalars(O.FID[fname], 62, n, montgomery=True)
    assert a.any(axis=1).all() and b.any(axis=1).all()
    ai, bi = R.ints(a), R.ints(b)
    a.astype("<u8").tofile(str(tmp_path / "a.bin"))
    b.astype("<u8").tofile(str(tmp_path / "b.bin"))
    for name, (vec, end) in (("product", R.prefix_product(f, ai, False)), ("sum_exclusive", R.prefix_sum(f, ai, True)),
                             ("ratio", R.prefix_ratio(f, ai, bi))):
        R.limbs(vec + [end]).astype("<u8").tofile(str(tmp_path / (name + ".bin")))
    exe = str(tmp_path / "prefix_scan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefix_scan_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(n), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
