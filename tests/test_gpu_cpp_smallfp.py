"""The one-word fields of the C++ mirror (include/ark_hip.hpp: SmallRadix2EvaluationDomain, SmallDeviceVec) from a compiled C++
program on the GPU; the vectors it checks against are written here by the Python big-integer model (tests/smallfp_ref.py)."""
import os
import subprocess

import pytest

import algebra_amd as A
import smallfp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_smallfp(tmp_path):
    lines = []
    for f in R.FIELDS.values():
        log = A.small_fft_plan(f.name, 0)[0] + 1   # the first two-pass size
        n = 1 << log
        rng = R.rng(600 + f.sid)
        a, b = f.random_elements(rng, n), f.random_elements(rng, n)
        a[0], a[1], a[n - 1], b[0], b[n - 1] = 0, f.p - 1, 0, f.p - 1, 0
        offset, k, nc = f.gen, rng.randrange(1, f.p), n // 4 + 1
        dom = f.get_coset(f.domain_new(n), offset)
        algebra = [(f.p - f.mul(f.sub(f.mul(f.add(x, y), y), x), k)) % f.p for x, y in zip(a, b)]
        inverse = [f.inv(x) for x in algebra]
        lines.append("%d %d %d %d %d" % (f.sid, log, offset, k, nc))
        for vec in (a, b, algebra, inverse, f.fft_fast(dom, a), f.fft_fast(dom, a[:nc]), [f.from_mont(x) for x in a]):
            lines.append(" ".join(map(str, vec)))
        lines.append(" ".join(str(dom[key]) for key in ("size_inv", "group_gen", "group_gen_inv", "offset_inv", "offset_pow_size")))
    vectors = tmp_path / "smallfp_vectors.txt"
    vectors.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "smallfp_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "smallfp_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd")],
                          timeout=300)
    out = subprocess.run([exe, str(vectors)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
