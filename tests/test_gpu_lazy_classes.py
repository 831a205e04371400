"""The carry-free limb arithmetic ON THE DEVICE at the limits of its operand classes (csrc/fp28.cuh FpL, fp28x2.cuh Fp2L,
fft.cuh Fft29, ec28.cuh / ec28x2.cuh), against the exact model of tests/lazy_model.py.

The device forms are not the code the host checks run: products are the asm column chains, Fp2L exists for the device
only.  None of it has a conditional subtraction or a carry flag to fall back on; it is right because of hand-derived bounds.
So every op is fed RAW limbs (ark_hip_test_lazy_raw_op) chosen at the edge of its documented class -- every limb at the
class maximum, one limb at the maximum, values 0 / p / j p +- 1 / the largest the class admits, the same value in several
limb shapes -- plus 4096 seeded random in-class rows, and compared with the model limb for limb.  The model carries every
op's precondition (a product column below 2^64, no limb of a limb-wise difference negative), so a row outside the contract
fails here rather than being skipped.  The accumulators go in and come out in LazyK's parked layout
(ark_hip_test_lazy_acc_op), so the bounds of the state that comes OUT are visible (the invariant asks for normalised
limbs, so an accumulator coordinate has one limb shape per value: its edge is the multiple of p added to it).  The same
vectors run through the host forms in tests/test_lazy_model_host.py.  No vector is skipped and nothing is compared with a
tolerance: every comparison is exact equality of integers."""
import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
import lazy_model as M
import pyref as P

pytestmark = pytest.mark.gpu

NRAND = 4096
FIELD_CASES = [(f, n, k, h) for f in P.FIELD_ORDER for (n, k, h) in M.all_field_ops(f)]
X2_CASES = [(f, n, k, h) for f in M.NEG_BETA for (n, k, h) in M.all_x2_ops()]


def _run(field, name, k, h, rows):
    g = M.GEO[field]
    rc, out = H.lazy_raw_op(M.FIELD_ID[field], M.TABLE[name]["op"], k, h, M.rows_to_array(g, rows), g.L)
    assert rc == 0, (field, name, k, h, rc)
    return out


def _compare(field, name, k, h, got, exp):
    want = M.expected_to_array(M.GEO[field], exp)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s %s<%d,%d>: %d of %d rows differ; first row %d: device %s, model %s" % (
        field, name, k, h, bad.size, len(exp), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("field,name,k,h", FIELD_CASES, ids=["%s-%s-%d-%d" % c for c in FIELD_CASES])
def test_field_op_matches_model_limb_for_limb(field, name, k, h):
    """the full deterministic extreme list of every legal operand-class combination (every operand at its limb maximum
    simultaneously first) + 4096 random in-class rows: device == model, limbs and flag"""
    rows = M.field_vectors(field, name, k, h, NRAND)
    exp = M.expected(field, name, k, h, rows)   # raises OutOfContract on a vector outside the op's precondition
    assert len(rows) >= NRAND
    _compare(field, name, k, h, _run(field, name, k, h, rows), exp)


@pytest.mark.parametrize("field,name,k,h", X2_CASES, ids=["%s-%s-%d-%d" % c for c in X2_CASES])
def test_fp2_lane_pair_op_matches_model(field, name, k, h):
    """Fp2L: one element per lane pair, partner fetched by DPP; mul<KA> / sqr<KW> (value and zero flag) / mul_sub<KA, KY> as
    Fp2 arithmetic per lane through the exact product rule, operands at their class limits"""
    rows, exp = M.x2_vectors(field, name, k, h, NRAND)
    assert len(rows) % 2 == 0
    _compare(field, name, k, h, _run(field, name, k, h, rows), exp)


def test_parameters_outside_the_table_are_refused():
    g = M.GEO["BLS12_381_FQ"]
    z = np.zeros((2, 8 * g.L), dtype=np.uint32)
    fid = M.FIELD_ID["BLS12_381_FQ"]
    for name, k, h in (("sub_semi", 5, 0), ("sub_sweep", 7, 0), ("mul", 1, 0), ("shr_mod", 5, 0), ("dif", 4, 1), ("x2_mul", 3, 0),
                       ("x2_mul_sub", 4, 4)):
        rc, _ = H.lazy_raw_op(fid, M.TABLE[name]["op"], k, h, z, g.L)
        assert rc == -1, (name, k, h, rc)   # ARK_HIP_ERR_ARG
    rc, _ = H.lazy_raw_op(fid, 99, 0, 0, z, g.L)
    assert rc == -1
    rc, _ = H.lazy_raw_op(M.FIELD_ID["BN254_FQ"], M.TABLE["x2_mul"]["op"], 2, 0, np.zeros((2, 18), dtype=np.uint32), 9)
    assert rc == -1   # no Fp2L over BN254's base field
    rc, _ = H.lazy_raw_op(fid, M.TABLE["x2_mul"]["op"], 2, 0, z[:1], g.L)
    assert rc == -1   # an odd lane count has no partner


# ---- accumulator level: LazyK's parked layout in, parked layout out -------------------------------------------------------
def _acc_run(A, kind, accs, others):
    a, o, ow = M.acc_pack(A, kind, accs, others)
    return H.lazy_acc_op(A.cid, M.ACC_KIND[kind], a, o, ow)


def _generator(A):
    G = A.C.dec(O.generator(A.cid))
    assert A.C.on_curve(G) and G is not None
    return G


def _check_output(A, got_words, want_acc, want_point, what):
    """device == model limb for limb; (a) the right group element, (b) ZZ^3 = ZZZ^2, (c) closure: normalised and inside the
    invariant, hence a legal input again"""
    got = A.unpark(got_words)
    assert [int(w) for w in got_words] == A.park(want_acc) or (got["inf"] and want_acc["inf"]), \
        "%s: device %s, model %s" % (what, list(map(int, got_words)), A.park(want_acc))
    assert A.affine(got) == want_point, what
    assert A.consistent(got), what
    assert A.in_invariant(got), "%s: output leaves the accumulator invariant %s" % (what, M.ACC_INVARIANT[A.curve])


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_accumulator_ops_at_the_edge_of_the_invariant(curve):
    """valid points whose XYZZ coordinates sit at the edge of the accumulator invariant (X = x zz + j p for every j the bound
    admits, ...), every branch: other point, equal point (double the base / in-place doubling), inverse point (to infinity),
    accumulator or operand at infinity, with P = U2 - U1 + K p a 0-representative of different multiples of p"""
    A = M.AccModel(curve)
    cases = M.acc_edge_cases(A, _generator(A))
    outs = []
    for kind in sorted({c[0] for c in cases}):
        sel = [c for c in cases if c[0] == kind]
        want = [M.acc_apply(A, kind, c[1], c[2]) for c in sel]   # OutOfContract here = a case outside the contract: fails
        got = _acc_run(A, kind, [c[1] for c in sel], [c[2] for c in sel])
        for i, (c, w) in enumerate(zip(sel, want)):
            _check_output(A, got[i], w, c[3], "%s %s case %d" % (curve, kind, i))
        outs += [(A.unpark(got[i]), c[3]) for i, c in enumerate(sel)]
    # (d) after to_bucket: canonical limbs, the same point -- on the DEVICE outputs
    tb = _acc_run(A, "to_bucket", [o[0] for o in outs], None)
    n = A.g.N * A.ext
    for i, (acc, pt) in enumerate(outs):
        words = [int(w) for w in tb[i]]
        assert words == A.to_bucket(acc), (curve, i)
        for c in range(4 * A.ext):
            assert A.g.from_words(words[c * A.g.N:(c + 1) * A.g.N]) < A.g.p, (curve, i, c)
        assert M.bucket_point(A, words) == pt, (curve, i)
    assert len(outs) == len(cases)


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_accumulator_chains_through_the_parked_layout(curve):
    """64 random steps of mixed ops from edge states; the device result of step i is the device input of step i + 1, model
    and device compared after every step"""
    A = M.AccModel(curve)
    lanes, steps = 8, 64
    starts, mult, sched, pt = M.acc_chain_ops(A, _generator(A), lanes, steps)
    dev = np.array([A.park(s) for s in starts], dtype=np.uint64).astype(np.uint32)
    model = list(starts)
    cur = list(mult)
    hit = set()
    for step, (kind, ops, ms) in enumerate(sched):
        o = None
        if kind == "add_acc":
            o = np.array([A.park(x) for x in ops], dtype=np.uint64).astype(np.uint32)
        elif kind != "dbl":
            o = np.array(ops, dtype=np.uint64).astype(np.uint32)
        dev = H.lazy_acc_op(A.cid, M.ACC_KIND[kind], dev, o, A.words)
        for i in range(lanes):
            before = cur[i]
            model[i] = M.acc_apply(A, kind, model[i], ops[i])
            cur[i] = cur[i] - ms[i] if kind == "msub" else cur[i] + ms[i]
            _check_output(A, dev[i], model[i], pt(cur[i]), "%s step %d (%s) lane %d" % (curve, step, kind, i))
            if kind != "dbl" and before % A.C.r:
                eff = -ms[i] if kind == "msub" else ms[i]
                hit.add("equal" if eff == before else "inverse" if eff == -before else "other")
            if before % A.C.r == 0:
                hit.add("from infinity")
    assert hit == {"equal", "inverse", "other", "from infinity"}, hit   # the schedule reaches every branch
