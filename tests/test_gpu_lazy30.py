"""The signed 13 x 30-bit form of the plain accumulate kernel of BLS12-381 G1 (csrc/fp30s.cuh, ec30s.cuh) on the device.

Field level: the asm column chains of mul / sqr / sop2, the sweeps, both repacks and the mixed addition run ONE OP AT A TIME on raw
digits (ark_hip_test_s30_op) over the class-limit vectors of tests/lazy30_model.py -- every digit at +-2^29, alternating signs,
0, +-1, +-(p - 1), residues at the value bounds -- and are compared word for word with the header's host twins
(tests/lazy30_raw_host.hip) and with the model.

MSM level.  WHICH KERNEL RUNS: at the default plan a plain BLS12-381 G1 MSM of 256 .. 73728 pairs splits every run over 4 or 8
lanes (msm_make_plan's `parts`) and runs msm_accumulate_parts_kernel, which keeps the 28-bit form; msm_accumulate_lazy_kernel -- the
signed form -- runs from 2^17 pairs on, in every piece of a streamed call, and wherever ARK_HIP_MSM_RUN_PARTS=1 (read per call)
switches the split off.  So:
  * the branch cases go through ark_hip_test_msm_pieces (pieces never split runs; the dump's header says lazy = 1) with buckets
    built to hold EXACTLY the points that reach a branch -- P, P (the doubling, through the device expansion of xyzz_mdbl_s);
    P, -P (to infinity); P, -P, Q (and back); a stored bucket reloaded by a later piece that meets its own point again, its
    inverse, or nothing -- and tests/msm_bucket_ref.py checks every bucket behind every piece against [sum of +-k_i] G;
  * the API-level cases (2^10, 2^13, scalars 0 / 1 / r - 1, repeated and inverse bases among others, 2^16) set
    ARK_HIP_MSM_RUN_PARTS=1 and are compared with the oracle bit for bit; one 2^16 case stays at the default plan and says so:
    there the accumulation is the parts kernel's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import algebra_amd as A
import lazy30_model as M
import msm_bucket_ref as BR
import msm_piece_cases as PC
import oracle_lib as O
from algebra_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = O.CID["BLS12_381_G1"]
R_ORDER = 52435875175126190479447740508185965837690552500527637822603658699938581184513
A4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)
B4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)


@pytest.fixture(scope="module")
def bases():
    """2^13 affine points (a + i b) G, canonical Montgomery words (x | y, 6 + 6 u64); made once, never written to"""
    b = O.gen_bases(CID, A4, B4, 1 << 13)
    b.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    """the header's host twins as a program; None where no compiler is at hand (the comparison with the model, which
    tests/test_lazy30_model_host.py ties to the host twins digit for digit, runs regardless)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = str(tmp_path_factory.mktemp("lazy30") / "lazy30_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_raw_host.hip"), "-o", exe], timeout=900)
    return exe


def run_host(exe, op, rows, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(rows, dtype=np.int32).tofile(fin)
    subprocess.run([exe, str(M.OPS[op]), fin, fout], check=True, timeout=300)
    return np.fromfile(fout, dtype=np.int32).reshape(len(rows), -1)


def run_device(op, rows, out_words):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((rows.shape[0], out_words), dtype=np.int32)
    _lib.check(_lib.test_lib().ark_hip_test_s30_op(M.OPS[op], rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), rows.shape[0]),
               "test_s30_op")
    return out


@pytest.mark.parametrize("op", ["mul", "sqr", "sop2", "sub", "add_2b", "from_canonical_shl", "to_canonical"])
def test_device_forms_equal_host_twins_at_the_class_limits(op, host_runner, tmp_path):
    rows = M.op_rows(op, np.random.default_rng(11))
    packed = M.pack_rows(op, rows)
    got = run_device(op, packed, M.L)
    assert np.array_equal(got, M.pack_rows("sqr", [[M.apply(op, r)] for r in rows])), "device != model"
    if host_runner:
        assert np.array_equal(got, run_host(host_runner, op, packed, tmp_path)), "device != host twin"


def words32(u64row):
    return [int(v) for v in np.ascontiguousarray(u64row, dtype=np.uint64).view(np.uint32)]


def test_mixed_addition_every_branch_equals_host_twin(bases, host_runner, tmp_path):
    pts = [(words32(bases[i, :6]), words32(bases[i, 6:])) for i in range(12)]
    ins, outs = M.madd_rows(pts)
    assert any(o[-1] == 1 for o in outs) and any(o[4 * M.L] == 1 for o in outs), "the chain reaches the doubling and infinity"
    packed = (np.array(ins, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)
    assert packed.shape[1] == M.MADD_IN
    got = run_device("madd", packed, M.MADD_OUT)
    want = (np.array(outs, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)
    # an accumulator gone to infinity keeps whatever coordinates it had: only its flag is compared
    live = want[:, 4 * M.L] == 0
    assert np.array_equal(got[:, 4 * M.L:], want[:, 4 * M.L:])
    assert np.array_equal(got[live], want[live]), "device != model"
    if host_runner:
        host = run_host(host_runner, "madd", packed, tmp_path)
        assert np.array_equal(host[:, 4 * M.L:], want[:, 4 * M.L:]) and np.array_equal(got[live], host[live]), "device != host twin"


# ---- the branches of the addition, bucket by bucket: ark_hip_test_msm_pieces ----------------------------------------------------
CURVE = "BLS12_381_G1"
C_BRANCH = 8


def branch_case_one_piece():
    """window 0, bucket d - 1 holds exactly: 1: P P | 2: P P P | 3: P -P | 4: P -P Q | 5: P -P P P | 6: P P P P | 7: P alone |
    and, under the scalar r - 9 (digits in every window), P P again: a doubling in every window.  Around them full-width
    scalars with no digit in window 0."""
    b = PC.Builder(CURVE)
    r = b.r
    k = b.new(10)
    b.run(1, 0, logs_=[k[0], k[0]])
    b.run(2, 0, logs_=[k[1]] * 3)
    b.run(3, 0, logs_=[k[2], r - k[2]])
    b.run(4, 0, logs_=[k[3], r - k[3], k[4]])
    b.run(5, 0, logs_=[k[5], r - k[5], k[5], k[5]])
    b.run(6, 0, logs_=[k[6]] * 4)
    b.run(7, 0, logs_=[k[7]])
    b.run(9, 0, neg=True, logs_=[k[8], k[8]])
    b.background(200, 41)
    b.cut()
    return PC.Case("lazy30-branches", b.input(), C_BRANCH)


def branch_case_three_pieces():
    """the same branches met by a RELOADED bucket (accum = 1: from_bucket brings the stored canonical point into the signed form):
    bucket 0: P | P (equal: the doubling) | -2P (to infinity);  bucket 1: P | -P (infinity is stored) | Q (a first point onto a
    reloaded identity);  bucket 2: P Q | P | nothing;  bucket 3: P | nothing | nothing;  bucket 4: nothing | P | P"""
    b = PC.Builder(CURVE)
    r = b.r
    k = b.new(8)
    b.run(1, 0, logs_=[k[0]]); b.run(2, 0, logs_=[k[1]]); b.run(3, 0, logs_=[k[2], k[3]]); b.run(4, 0, logs_=[k[4]])
    b.background(120, 42)
    b.cut()
    b.run(1, 0, logs_=[k[0]]); b.run(2, 0, logs_=[r - k[1]]); b.run(3, 0, logs_=[k[2]]); b.run(5, 0, logs_=[k[5]])
    b.background(120, 43)
    b.cut()
    b.run(1, 0, logs_=[(r - 2 * k[0]) % r]); b.run(2, 0, logs_=[k[6]]); b.run(5, 0, logs_=[k[5]])
    b.background(120, 44)
    b.cut()
    return PC.Case("lazy30-reloaded", b.input(), C_BRANCH, all_identity=())


@pytest.mark.parametrize("make", [branch_case_one_piece, branch_case_three_pieces], ids=["one-piece", "three-pieces"])
def test_every_branch_of_the_signed_addition_bucket_by_bucket(make):
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


# ---- whole MSMs through the API, the split of runs switched off -------------------------------------------------------------------
@pytest.fixture
def one_lane_per_run(monkeypatch):
    """ARK_HIP_MSM_RUN_PARTS=1 (msm_plan.hpp, read per call): msm_accumulate_lazy_kernel instead of the parts kernel"""
    monkeypatch.setenv("ARK_HIP_MSM_RUN_PARTS", "1")


def to_scalars(vals):
    return np.array([[(v >> (64 * i)) & 0xffffffffffffffff for i in range(4)] for v in vals], dtype=np.uint64)


def neg_base(row):
    out = np.array(row, dtype=np.uint64).copy()
    y = sum(int(v) << (64 * i) for i, v in enumerate(out[6:]))
    ny = M.P_INT - y
    out[6:] = [(ny >> (64 * i)) & 0xffffffffffffffff for i in range(6)]
    return out


def check_against_oracle(b, s):
    want = O.to_affine(CID, O.msm(CID, b, s, O.SIGNED, 4))
    got = O.to_affine(CID, A.msm_bigint(CID, np.ascontiguousarray(b), np.ascontiguousarray(s)))
    assert np.array_equal(got, want)


def random_scalars(n, seed):
    return O.gen_scalars(O.curve_info(CID)[1], seed, n)


@pytest.mark.parametrize("log_n", [10, 13])
def test_msm_matches_oracle(bases, log_n, one_lane_per_run):
    n = 1 << log_n
    check_against_oracle(bases[:n], random_scalars(n, 5 + log_n))


def test_msm_repeated_bases_among_others(bases, one_lane_per_run):
    n = 1 << 10
    b, s = bases[:n].copy(), random_scalars(n, 21)
    for k in range(0, 64, 2):                 # the same base with the same scalar: the same bucket in every window, twice
        b[k + 1], s[k + 1] = b[k], s[k]
    b[100], b[101], s[100], s[101] = b[3], b[3], s[3], s[3]   # and four times
    check_against_oracle(b, s)


def test_msm_inverse_pairs_among_others(bases, one_lane_per_run):
    n = 1 << 10
    b, s = bases[:n].copy(), random_scalars(n, 22)
    for k in range(0, 96, 3):                 # P, -P and a third point under one scalar
        b[k + 1] = neg_base(b[k])
        s[k + 1] = s[k]
        s[k + 2] = s[k]
    b[200], b[201], b[202], b[203] = b[0], neg_base(b[0]), b[0], neg_base(b[0])
    s[200] = s[201] = s[202] = s[203] = s[0]
    check_against_oracle(b, s)


def test_msm_scalars_zero_one_and_r_minus_one(bases, one_lane_per_run):
    n = 1 << 10
    s = random_scalars(n, 23).copy()
    s[0::5] = to_scalars([0])[0]
    s[1::5] = to_scalars([1])[0]
    s[2::5] = to_scalars([R_ORDER - 1])[0]
    check_against_oracle(bases[:n], s)
    check_against_oracle(bases[:n], to_scalars([R_ORDER - 1] * n))


def test_msm_streamed_in_three_pieces_reloads_stored_buckets(bases, monkeypatch):
    n = 1 << 10
    b, s = bases[:n].copy(), random_scalars(n, 24)
    third = n // 3
    for k in range(16):                       # across the piece boundaries: an earlier piece's point again, and an inverse
        b[third + k], s[third + k] = b[k], s[k]
        b[2 * third + k], s[2 * third + k] = neg_base(b[16 + k]), s[16 + k]
    monkeypatch.setenv("ARK_HIP_STREAM_PIECES", "3")
    monkeypatch.setenv("ARK_HIP_MSM_C", "6")
    A.base_cache_config(0, 0)                 # cache off: the bases ring through with the scalars, piece by piece
    try:
        check_against_oracle(b, s)
    finally:
        A.base_cache_config(-2, 0)
        A.base_cache_clear()


def test_msm_two_to_the_sixteen_one_lane_per_run(bases, one_lane_per_run):
    b = np.tile(bases, (8, 1))                # 2^16 pairs; a base meets itself under eight different scalars
    check_against_oracle(b, random_scalars(1 << 16, 25))


def test_msm_two_to_the_sixteen_at_the_default_plan(bases):
    """NOT the signed kernel: at the default plan 2^16 pairs run msm_accumulate_parts_kernel (28-bit form).  Kept because the issue
    names the job; what it shows is that the default path of this size is undisturbed."""
    b = np.tile(bases, (8, 1))
    check_against_oracle(b, random_scalars(1 << 16, 25))
