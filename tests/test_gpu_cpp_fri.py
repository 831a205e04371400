"""SmallExtVec, FriProver and fri_verify_query of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU: it
runs one commit phase per field, prints the roots and the final polynomial, and verifies a few queries itself; the roots and
coefficients are compared here with the model (tests/fri_ref.py).  The challenge of a layer is word k of its root modulo p, a rule
both sides can compute."""
import os
import subprocess

import pytest

import fri_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def root_challenge(x):
    return lambda root: tuple(int.from_bytes(root[8 * k:8 * k + 8], "little") % x.p for k in range(x.d))


def test_cpp_fri(tmp_path):
    lines, wants = [], []
    for name, k, a, folds in (("GOLDILOCKS", 9, 2, 4), ("BABYBEAR", 10, 3, 4), ("KOALABEAR", 8, 1, 5)):
        x = X.FIELDS[name]
        rng = X.rng(900 + k)
        layer = [x.random_element(rng) for _ in range(1 << k)]
        layer[3] = x.zero()
        cols = [[e[c] for e in layer] for c in range(x.d)]
        lines.append("%d %d %d %d %d" % (x.sid, k, a, folds, x.st(x.gen)))
        lines.append(" ".join(str(v) for c in cols for v in c))
        wants.append(x.commit_phase(cols, k, x.gen, a, folds, root_challenge(x)))
    vectors = tmp_path / "fri_vectors.txt"
    vectors.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "fri_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fri_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(vectors)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and out.stdout.count("verify ok") == 3
    roots = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("roots")]
    finals = [[int(v) for v in l.split()[1:]] for l in out.stdout.splitlines() if l.startswith("final")]
    for want, r, f in zip(wants, roots, finals):
        assert r == [d.hex() for d in want["roots"]]
        assert f == [v for c in want["final"] for v in c]
