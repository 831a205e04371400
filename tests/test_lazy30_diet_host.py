"""The unsigned gathered coordinate of the accumulate kernel's mixed addition (csrc/fp30s.cuh: from_canonical_u; ec30s.cuh) against
the path it replaces, on the HOST: tests/lazy30_diet_host_check.hip is built twice, as shipped and with
-DARK_S30_UNSIGNED_GATHER=0 (the retained old path), each with the undefined-behaviour and address sanitizers on its host code,
and run as a program.  Each build checks the new functions against the ones that stay; the two records of every product and
accumulator must be the same file."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unsigned_gather_equals_the_retained_path_word_for_word(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")

    def build_and_run(diet):
        exe, rec = str(tmp_path / ("diet%d" % diet)), str(tmp_path / ("rec%d.bin" % diet))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address",
                               "-Xarch_host", "-fno-sanitize-recover=undefined", "-DARK_S30_UNSIGNED_GATHER=%d" % diet,
                               "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                               os.path.join(ROOT, "tests", "lazy30_diet_host_check.hip"), "-o", exe], timeout=900)
        out = subprocess.run([exe, rec], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "BLS12_381_FQ signed30 unsigned gather=%d: ok (0 bad" % diet in out.stdout, out.stdout
        return open(rec, "rb").read()

    with ThreadPoolExecutor(2) as pool:
        new, old = pool.map(build_and_run, (1, 0))
    assert len(new) > 1 << 20 and new == old
