"""csrc/fp30s.cuh + ec30s.cuh (the signed 13 x 30-bit arithmetic of the plain accumulate kernel of BLS12-381 G1) checked on the
HOST: the portable twins of mul / sqr / sop2, the repacks in both directions and the mixed addition against the saturated-limb
arithmetic, and every stored bucket word for word against the 28-bit form -- random operands and the class limits.  The program
is built with the undefined-behaviour and address sanitizers on its host code: no signed multiply or shift of the portable forms
may overflow."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signed30_field_and_madd_match_saturated_and_28bit_forms(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "lazy30_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_host_check.hip"), "-o", exe], timeout=900)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "BLS12_381_FQ signed30: ok (0 bad)" in out.stdout, out.stdout
