"""The unsigned gathered coordinate of the mixed addition of the plain accumulate kernel of BLS12-381 G1 (csrc/fp30s.cuh:
from_canonical_u; ec30s.cuh: s30_from_affine) on the device.

Raw ops, one at a time (ark_hip_test_s30_op, ops 8 and 9 of csrc/s30test_api.hpp and op 0 on the new operand class; rows and
expected digits from tests/lazy30_diet_rows.py): the unsigned repack on 0, 1, p - 1 and random words; a product of an unsigned
operand with every digit at 2^30 - 1 against normalised ones at +-2^29; the kernel's own entry to the mixed addition
(LazySK::madd: sign, repack, addition) over the branch chain of lazy30_model.madd_rows with both digit signs.  Each against the
model, and against the header's host forms where a compiler is at hand.

MSM level, the smallest jobs that run msm_accumulate_lazy_kernel (tests/test_gpu_lazy30.py says which sizes do): its one-piece and
three-piece branch cases with NEGATIVE digit signs on the doubling and cancelling buckets, every bucket behind every piece against
tests/msm_bucket_ref.py; one 2^10 MSM with the split of runs switched off, against the oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import algebra_amd as A
import lazy30_diet_model as D
import lazy30_diet_rows as R
import lazy30_model as M
import msm_bucket_ref as BR
import msm_piece_cases as PC
import oracle_lib as O
from algebra_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = O.CID["BLS12_381_G1"]
CURVE = "BLS12_381_G1"
C_BRANCH = 8
OPS = {**M.OPS, **D.OPS}


@pytest.fixture(scope="module")
def cases():
    """rows and the model's answers, made once and never written to"""
    out = R.raw_cases(D.curve_points(12))
    for rows, want in out.values():
        rows.setflags(write=False)
        want.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    """the header's host forms as a program (tests/lazy30_raw_host.hip); None where no compiler is at hand"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = str(tmp_path_factory.mktemp("lazy30diet") / "lazy30_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_raw_host.hip"), "-o", exe], timeout=900)
    return exe


def run_host(exe, op, rows, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(rows, dtype=np.int32).tofile(fin)
    subprocess.run([exe, str(OPS[op]), fin, fout], check=True, timeout=300)
    return np.fromfile(fout, dtype=np.int32).reshape(len(rows), -1)


def run_device(op, rows, out_words):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((rows.shape[0], out_words), dtype=np.int32)
    _lib.check(_lib.test_lib().ark_hip_test_s30_op(OPS[op], rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), rows.shape[0]),
               "test_s30_op")
    return out


@pytest.mark.parametrize("op", ["from_canonical_u", "mul", "madd_entry"])
def test_device_forms_equal_model_and_host_forms(op, cases, host_runner, tmp_path):
    rows, want = cases[op]
    assert rows.shape[1] == (D.MADD_IN if op == "madd_entry" else M.L * {"from_canonical_u": 1, "mul": 2}[op])
    got = run_device(op, rows, want.shape[1])
    R.compare(op, got, want)
    if op == "madd_entry":      # the chain reaches the doubling and infinity, with both signs
        assert (want[rows[:, -1] == 1][:, -1] == 1).any() and (want[rows[:, -1] == 0][:, 4 * M.L] == 1).any()
    if host_runner:
        R.compare(op, got, run_host(host_runner, op, rows, tmp_path))


# ---- the branches of the addition under negative digits, bucket by bucket ---------------------------------------------------------
def branch_case_one_piece_negative():
    """test_gpu_lazy30's one-piece case with the scalar r - d on the doubling and cancelling buckets: window 0, bucket d - 1 holds
    exactly 1: -P -P | 2: -P -P -P | 3: -P P | 4: -P P -Q | 5: -P P -P -P | 6: P P P P (positive, beside them) | 7: -P alone;
    r - d has digits in every window, so every one of these meets its branch there too"""
    b = PC.Builder(CURVE)
    r = b.r
    k = b.new(10)
    b.run(1, 0, neg=True, logs_=[k[0], k[0]])
    b.run(2, 0, neg=True, logs_=[k[1]] * 3)
    b.run(3, 0, neg=True, logs_=[k[2], r - k[2]])
    b.run(4, 0, neg=True, logs_=[k[3], r - k[3], k[4]])
    b.run(5, 0, neg=True, logs_=[k[5], r - k[5], k[5], k[5]])
    b.run(6, 0, logs_=[k[6]] * 4)
    b.run(7, 0, neg=True, logs_=[k[7]])
    b.run(9, 0, logs_=[k[8], r - k[8], k[9]])
    b.background(200, 45)
    b.cut()
    return PC.Case("lazy30-diet-branches-negative", b.input(), C_BRANCH)


def branch_case_three_pieces_negative():
    """test_gpu_lazy30's three-piece case under negative digits: a RELOADED bucket meets  bucket 0: -P | -P (equal: the doubling) |
    2P (to infinity);  bucket 1: -P | P (infinity is stored) | -Q (a first point onto a reloaded identity);  bucket 2: -P -Q | -P |
    nothing;  bucket 3: -P | nothing | nothing;  bucket 4: nothing | -P | -P"""
    b = PC.Builder(CURVE)
    r = b.r
    k = b.new(8)
    n = dict(neg=True)
    b.run(1, 0, logs_=[k[0]], **n); b.run(2, 0, logs_=[k[1]], **n); b.run(3, 0, logs_=[k[2], k[3]], **n); b.run(4, 0, logs_=[k[4]], **n)
    b.background(120, 46)
    b.cut()
    b.run(1, 0, logs_=[k[0]], **n); b.run(2, 0, logs_=[r - k[1]], **n); b.run(3, 0, logs_=[k[2]], **n); b.run(5, 0, logs_=[k[5]], **n)
    b.background(120, 47)
    b.cut()
    b.run(1, 0, logs_=[(r - 2 * k[0]) % r], **n); b.run(2, 0, logs_=[k[6]], **n); b.run(5, 0, logs_=[k[5]], **n)
    b.background(120, 48)
    b.cut()
    return PC.Case("lazy30-diet-reloaded-negative", b.input(), C_BRANCH, all_identity=())


@pytest.mark.parametrize("make", [branch_case_one_piece_negative, branch_case_three_pieces_negative], ids=["one-piece", "three-pieces"])
def test_every_branch_under_negative_digits_bucket_by_bucket(make):
    case = make()
    d = BR.gpu_pieces(case.inp, **case.knobs())
    assert d["rc"] == 0, d["rc"]
    h = d["header"]
    ref = BR.plan_header(case.inp.curve, case.c, case.inp.sizes)
    assert (h["c"], h["W"], h["nbuckets"], h["npieces"]) == (ref["c"], ref["W"], ref["nbuckets"], ref["npieces"])
    # a piece takes msm_accumulate_lazy_kernel: lazy = 1, one window group, and pieces never split their runs over lanes
    assert h["lazy"] == 1 and h["pieces_run"] == h["npieces"] and [p["ngroups"] for p in h["pieces"]] == [1] * h["npieces"]
    m = case.model(h)
    BR.check_dump(d, m)                       # every bucket behind every piece, no tolerance
    for k in range(h["npieces"]):             # no run of these cases is heavy: every bucket is the accumulate kernel's own
        assert m.regime(k)[1] == []
    want = O.to_affine(CID, O.msm(CID, case.inp.bases, case.inp.scalars, O.SIGNED, 4)).reshape(-1)
    assert np.array_equal(O.to_affine(CID, d["result"]).reshape(-1), want), "the final point"


def test_msm_two_to_the_ten_one_lane_per_run_matches_oracle(monkeypatch):
    """ARK_HIP_MSM_RUN_PARTS=1 (read per call): msm_accumulate_lazy_kernel instead of the parts kernel"""
    monkeypatch.setenv("ARK_HIP_MSM_RUN_PARTS", "1")
    n = 1 << 10
    b = O.gen_bases(CID, np.array([0xD1E7, 5, 1, 0], dtype=np.uint64), np.array([0xF00D, 7, 0, 0], dtype=np.uint64), n)
    s = O.gen_scalars(O.curve_info(CID)[1], 31, n)
    want = O.to_affine(CID, O.msm(CID, b, s, O.SIGNED, 4))
    got = O.to_affine(CID, A.msm_bigint(CID, np.ascontiguousarray(b), np.ascontiguousarray(s)))
    assert np.array_equal(got, want)
