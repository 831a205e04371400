"""ListOfProducts::prove_device and Transcript of the C++ mirror (include/ark_hip.hpp) from a compiled C++ program on the GPU:
the whole proof in one wait at 9 variables on each scalar field; what it prints -- rounds, point, final values, value and the
transcript's end state -- is compared with the big-integer model (tests/sumcheck_ref.py, tests/transcript_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref
import sumcheck_ref as S
import transcript_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEED = bytes(range(100, 132))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cpp") / "sumcheck_device_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "sumcheck_device_check.cpp"), "-o", path,
                           "-L", os.path.join(ROOT, "algebra_amd"), "-lark_hip", "-L", os.path.join(ROOT, "oracle"),
                           "-lark_oracle", "-Wl,-rpath," + os.path.join(ROOT, "algebra_amd"),
                           "-Wl,-rpath," + os.path.join(ROOT, "oracle")], timeout=300)
    return path


@pytest.mark.parametrize("fname", ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"])
def test_cpp_sumcheck_device(exe, fname):
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    nv = 9
    tables = [S.decode(O.gen_scalars(fid, 51 + q, 1 << nv, montgomery=True), p) for q in range(3)]
    k = int.from_bytes(np.random.default_rng(909).bytes(40), "little") % p
    terms = [(1, [0, 1, 2]), (k, [2, 0])]
    tr = T.Transcript(p, SEED)
    rounds, point, finals, value = T.prove(tables, terms, tr, p)
    assert T.verify((rounds[0][0] + rounds[0][1]) % p, rounds, point, finals, terms, T.Transcript(p, SEED), p)
    mont = lambda x: x * pyref.R_of(p) % p                                  # noqa: E731
    out = subprocess.run([exe, str(fid), "%064x" % mont(k), SEED.hex()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
    got, state = {}, None
    for line in out.stdout.splitlines():
        w = line.split()
        if len(w) == 4 and w[0] in ("round", "point", "final", "value"):
            got[(w[0], int(w[1]), int(w[2]))] = int(w[3], 16)
        if len(w) == 2 and w[0] == "state":
            state = bytes.fromhex(w[1])
    want = {("round", i, t): mont(v) for i, g in enumerate(rounds) for t, v in enumerate(g)}
    want.update({("point", i, 0): mont(v) for i, v in enumerate(point)})
    want.update({("final", q, 0): mont(v) for q, v in enumerate(finals)})
    want[("value", 0, 0)] = mont(value)
    assert got == want, sorted(key for key in want if got.get(key) != want[key])[:5]
    assert state == tr.state
