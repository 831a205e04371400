"""The ListOfProducts of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU: one whole prover at 9
variables on each scalar field; the transcript it prints is compared with the big-integer model (tests/sumcheck_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref
import sumcheck_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cpp") / "sumcheck_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "sumcheck_check.cpp"), "-o", path,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    return path


@pytest.mark.parametrize("fname", ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"])
def test_cpp_sumcheck(exe, fname):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    nv = 9
    tables = [S.decode(O.gen_scalars(fid, 51 + q, 1 << nv, montgomery=True), p) for q in range(3)]
    rng = np.random.default_rng(909)
    k = int.from_bytes(rng.bytes(40), "little") % p
    r = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(nv)]
    terms = [(1, [0, 1, 2]), (k, [2, 0])]
    rounds, point, finals, value = S.prove(tables, terms, lambda i, evals: r[i], p)
    assert point == r and S.verify_tables((rounds[0][0] + rounds[0][1]) % p, rounds, point, tables, terms, p)
    mont = lambda x: x * pyref.R_of(p) % p                                  # noqa: E731
    out = subprocess.run([exe, str(fid)] + ["%064x" % mont(v) for v in [k] + r], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if len(w) == 4 and w[0] in ("round", "final", "value"):
            got[(w[0], int(w[1]), int(w[2]))] = int(w[3], 16)
    want = {("round", i, t): mont(v) for i, g in enumerate(rounds) for t, v in enumerate(g)}
    want.update({("final", q, 0): mont(v) for q, v in enumerate(finals)})
    want[("value", 0, 0)] = mont(value)
    assert got == want, sorted(key for key in want if got.get(key) != want[key])[:5]
