"""The differences folded into the products that compute them (csrc/fp30s.cuh: mul_sub, sqr_sub2; ec30s.cuh under
ARK_S30_FUSED_DIFF) on the device.

Raw ops (ark_hip_test_s30_op, ops 10 and 11 of csrc/s30test_api.hpp): the edge rows and 64 random rows of
tests/lazy30_fused_model.py -- every digit at +-2^29, the top digits at their class limits, the signs that put every term of a
high column on one side, an unsigned gathered operand at its limit -- device against the chain the operation replaces, computed by
tests/lazy30_model.py's own sub / mul / sqr / add_2b.

The mixed addition (op 7): the rows of lazy30_model.madd_rows (first point, P P, P -P and on from there), reloaded accumulators and
accumulators at the limits of the invariant; the digits are lazy30_model.madd's, which knows no fused operation.

MSM level: one streamed-piece case of 2^10 pairs at c = 8 whose buckets hold exactly P P, P -P and P -P Q, every bucket behind the
piece against tests/msm_bucket_ref.py."""
import ctypes as C

import numpy as np
import pytest

import lazy30_diet_model as D
import lazy30_fused_model as FM
import lazy30_model as M
import msm_bucket_ref as BR
import msm_piece_cases as PC
import oracle_lib as O
from algebra_amd import _lib

pytestmark = pytest.mark.gpu

CID = O.CID["BLS12_381_G1"]
CURVE = "BLS12_381_G1"
L = M.L


def run_device(op, rows, out_words):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((rows.shape[0], out_words), dtype=np.int32)
    _lib.check(_lib.test_lib().ark_hip_test_s30_op(op, rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), rows.shape[0]),
               "test_s30_op")
    return out


@pytest.mark.parametrize("op", ["mul_sub", "sqr_sub2"])
def test_fused_operation_on_the_device_equals_the_chain_it_replaces(op):
    rows = FM.op_rows(op, np.random.default_rng(19), 64)
    packed = FM.pack_rows(rows)
    assert packed.shape == (len(rows), 3 * L) and len(rows) >= 64 + 20
    got = run_device(FM.OPS[op], packed, L)
    assert np.array_equal(got, FM.pack_rows([[FM.unfused(op, r)] for r in rows])), "device != sub(mul) / sub(sqr, add_2b) of the model"
    # and the device's own unfused chain, op by op
    if op == "mul_sub":
        u = run_device(M.OPS["mul"], packed[:, :2 * L], L)
        want = run_device(M.OPS["sub"], np.concatenate([u, packed[:, 2 * L:]], axis=1), L)
    else:
        e = run_device(M.OPS["add_2b"], packed[:, L:], L)
        want = run_device(M.OPS["sub"], np.concatenate([run_device(M.OPS["sqr"], packed[:, :L], L), e], axis=1), L)
    assert np.array_equal(got, want), "device: fused != unfused"


def test_mixed_addition_digits_are_unchanged():
    pts = D.curve_points(12)
    ins, outs = M.madd_rows(pts)
    xin, xout = FM.madd_extra_rows(pts)
    ins, outs = ins + xin, outs + xout
    assert any(o[-1] == 1 for o in outs) and any(o[4 * L] == 1 for o in outs), "the rows reach the doubling and infinity"
    assert any(r[4 * L] == 1 for r in ins), "and a first point"
    packed = (np.array(ins, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)
    want = (np.array(outs, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)
    assert packed.shape[1] == M.MADD_IN
    got = run_device(M.OPS["madd"], packed, M.MADD_OUT)
    # an accumulator gone to infinity keeps whatever coordinates it had: only its flags are compared
    live = want[:, 4 * L] == 0
    assert np.array_equal(got[:, 4 * L:], want[:, 4 * L:])
    assert np.array_equal(got[live], want[live]), "device != model"


def piece_case():
    """2^10 pairs in one piece at c = 8: window 0, bucket d - 1 holds exactly  1: P P | 2: P -P | 3: P -P Q | 4: -P -P (negative
    digits) | 5: -P P -Q | 6: P alone; around them full-width scalars with no digit in window 0"""
    b = PC.Builder(CURVE)
    r = b.r
    k = b.new(8)
    b.run(1, 0, logs_=[k[0], k[0]])
    b.run(2, 0, logs_=[k[1], r - k[1]])
    b.run(3, 0, logs_=[k[2], r - k[2], k[3]])
    b.run(4, 0, neg=True, logs_=[k[4], k[4]])
    b.run(5, 0, neg=True, logs_=[k[5], r - k[5], k[6]])
    b.run(6, 0, logs_=[k[7]])
    b.background((1 << 10) - b.open, 49)
    b.cut()
    return PC.Case("lazy30-fused-branches", b.input(), 8)


def test_streamed_piece_of_two_to_the_ten_bucket_by_bucket():
    case = piece_case()
    assert case.inp.sizes == [1 << 10]
    d = BR.gpu_pieces(case.inp, **case.knobs())
    assert d["rc"] == 0, d["rc"]
    h = d["header"]
    ref = BR.plan_header(case.inp.curve, case.c, case.inp.sizes)
    assert (h["c"], h["W"], h["nbuckets"], h["npieces"]) == (ref["c"], ref["W"], ref["nbuckets"], ref["npieces"])
    # the piece takes msm_accumulate_lazy_kernel: lazy = 1, one window group, no run split over lanes
    assert h["lazy"] == 1 and h["pieces_run"] == 1 and [p["ngroups"] for p in h["pieces"]] == [1]
    m = case.model(h)
    BR.check_dump(d, m)                       # every bucket behind the piece, no tolerance
    assert m.regime(0)[1] == []               # no run is heavy: every bucket is the accumulate kernel's own
    want = O.to_affine(CID, O.msm(CID, case.inp.bases, case.inp.scalars, O.SIGNED, 4)).reshape(-1)
    assert np.array_equal(O.to_affine(CID, d["result"]).reshape(-1), want), "the final point"
