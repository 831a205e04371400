"""CsrMatrix of the C++ mirror (include/ark_hip.hpp: mul, mul_t, bilinear) from a compiled C++ program on the GPU, on one
matrix of stream blocks only and one with long rows; the vectors it is handed are computed here with Python big integers
(tests/csr_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import algebra_amd as A
import csr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def write_case(tmp_path, f, name, lens, cols, seed):
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    col_idx = np.random.default_rng(seed).integers(0, cols, size=nnz).astype(np.uint32)
    vals, x, u = R.rand_elems(f, nnz, seed + 1), R.rand_elems(f, cols, seed + 2), R.rand_elems(f, rows, seed + 3)
    vals[0], vals[-1], x[0] = f.enc(-1), f.p - 1, 0
    y = R.mul(f, rows, row_ptr, col_idx, vals, x)
    t_ptr, t_idx, t_vals = R.transpose(rows, cols, row_ptr, col_idx, vals)
    yt = R.mul(f, cols, t_ptr, t_idx, t_vals, u)
    b = R.bilinear(f, rows, row_ptr, col_idx, vals, u, x)
    np.array([rows, cols, nnz], dtype="<u8").tofile(str(tmp_path / (name + "_dims.bin")))
    row_ptr.astype("<u4").tofile(str(tmp_path / (name + "_row_ptr.bin")))
    col_idx.astype("<u4").tofile(str(tmp_path / (name + "_col_idx.bin")))
    for part, elems in (("vals", vals), ("x", x), ("u", u), ("y", y), ("yt", yt), ("b", [b])):
        R.limbs(elems).astype("<u8").tofile(str(tmp_path / ("%s_%s.bin" % (name, part))))
    return A.csr_plan(rows, row_ptr)


def test_cpp_csr(tmp_path):
    f = R.Field("BLS12_381_FR")
    T = A.csr_plan(0, [0])[0]
    stream = write_case(tmp_path, f, "stream", [1 + (i * 5) % 4 for i in range(T + 77)], 900, 71)       # R1CS-like: 1 to 4 per row
    long_ = write_case(tmp_path, f, "long", [2, 0, 3 * T + 5, 1, T + 1, 0], 1500, 75)
    assert stream[2] >= 2 and stream[3] == 0 and long_[3:] == (2, 6)
    exe = str(tmp_path / "csr_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "csr_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(tmp_path), "stream", "long"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
