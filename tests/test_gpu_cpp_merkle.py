"""ark_hip::MerkleTree of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU: it commits, opens and
verifies one BabyBear matrix and two BLS12-381 Fr matrices (one of a single row) against roots written here by the Python model
(tests/merkle_ref.py)."""
import os
import subprocess

import pytest

import merkle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_merkle(tmp_path):
    lines = []
    for kind, field, count, log, idx in ((0, "BABYBEAR", 33, 11, [0, 2047, 1024, 1024, 77]), (1, "BLS12_381_FR", 3, 9, [511, 0, 300]),
                                         (1, "BLS12_381_FR", 5, 0, [0, 0])):
        n = 1 << log
        cols = R.random_columns(field, R.rng(700 + kind + log), count, n)
        cols[0][0], cols[-1][n - 1] = R.modulus(field) - 1, 0
        lines.append("%d %d %d %d" % (kind, count, log, len(idx)))
        flat = [x for c in cols for x in c]
        lines.append(" ".join(str(x) for x in flat) if kind == 0 else " ".join(str(w) for x in flat for w in R.words64(x)))
        lines.append(" ".join(str(b) for b in R.tree(field, cols)[0]))
        lines.append(" ".join(map(str, idx)))
    vectors = tmp_path / "merkle_vectors.txt"
    vectors.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "merkle_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "merkle_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(vectors)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
