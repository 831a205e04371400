"""The relaxed [0, 2p) arithmetic on saturated 32-bit limbs ON THE DEVICE at the limits of its operand classes (csrc/fp.cuh: Fp's
mul_r / add_r2 / sop2_r & co., Fp2, the lane-pair Fp2Half; csrc/ec.cuh: xyzz_madd_relaxed, xyzz_add_relaxed, xyzz_canonical),
against the exact model of tests/relaxed_model.py.

This is the arithmetic of every default FFT pass (fft_pass_kernel's butterflies; over BLS12-381 Fr, p = 0.45 R, add_r2 runs
through its carry-out case), of every G2 MSM's saturated accumulate form and of everything under ARK_HIP_MSM_LAZY=0.  It is
right only because of hand-derived bounds, and random canonical inputs never place the values that decide them.  So every op
is fed RAW limbs (ark_hip_test_relaxed_raw_op): the cross product of each operand class's edge list -- 0, 1, p - 1, p, p + 1,
2p - 1, 2p, R mod p, the class maximum, all-ones low limbs under an in-class top limb, one limb at 0xffffffff -- directed sums
and differences on the decisions themselves, and 4096 seeded random in-class rows.  The device result of every op is a definite
integer, (a b + m p) / R whatever the column schedule, so the comparison is limb for limb; residue and closure (the documented
output class) are asserted on the device's own outputs.  The Fp2Half ops run on lane pairs, so the DPP exchange is what runs.
The model carries every precondition: a row outside a contract fails, none is skipped.  The XYZZ accumulators go in and come
out as raw limbs (ark_hip_test_relaxed_acc_op), coordinates placed at value + j p.  The same vector files go through the
header's host forms in tests/test_relaxed_model_host.py."""
import numpy as np
import pytest

import hip_lib as H
import oracle_lib as O
import pyref as P
import relaxed_model as M

pytestmark = pytest.mark.gpu

NRAND = 4096
CASES = [(f, n) for f in P.FIELD_ORDER for n in M.ops_of(f)]


def _device(field, name, rows):
    g = M.GEO[field]
    rc, out = H.relaxed_raw_op(M.FIELD_ID[field], M.TABLE[name][0], M.rows_to_array(field, name, rows), g.N)
    assert rc == 0, (field, name, rc)
    return out


@pytest.mark.parametrize("field,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_op_matches_model_limb_for_limb(field, name):
    """device == model, limbs and flag, on every edge row, directed row and random row; then (b) the residue and (c) the
    output class on what the DEVICE returned"""
    g = M.GEO[field]
    rows, exp = M.case(field, name, NRAND)   # raises OutOfContract on a vector outside the op's precondition
    assert len(rows) >= NRAND
    got = _device(field, name, rows)
    want = M.expected_to_array(field, name, exp)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s %s: %d of %d lanes differ; first lane %d: device %s, model %s" % (
        field, name, bad.size, got.shape[0], bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
    for row, (res, flag) in zip(rows, M.array_to_results(field, name, got)):
        M.check_row(g, name, row, res, flag)


@pytest.mark.parametrize("field", M.SCALAR)
def test_butterfly_chains(field):
    """64 radix-2 butterfly steps as fft_pass_kernel runs them (fft.cuh:341-343: sum = add_r2, dif = mul_r1(sub_r, canonical
    twiddle)) from edge states, the device output of step i the device input of step i + 1, model == device after every step;
    then the relaxed x canonical mul that leaves the relaxed domain (fft.cuh:390)"""
    g = M.GEO[field]
    rng = np.random.default_rng(21)
    ed = M.edges(g, "2p")
    lo = [ed[i % len(ed)] for i in range(256)]
    hi = [ed[(i // len(ed) + 3 * i) % len(ed)] for i in range(256)]
    rnd = lambda bound: int.from_bytes(rng.bytes(40), "little") % bound

    def step(name, a, b):
        rows = [[x, y] for x, y in zip(a, b)]
        exp = M.expected(field, name, rows)
        got = M.array_to_results(field, name, _device(field, name, rows))
        assert got == exp, (field, name, next(i for i in range(len(rows)) if got[i] != exp[i]))
        return [r for r, _ in got]

    tw_edges = M.edges(g, "p")
    for s in range(64):
        tw = [tw_edges[(i + s) % len(tw_edges)] if (i + s) % 3 == 0 else rnd(g.p) for i in range(256)]
        sm = step("add_r2", lo, hi)
        df = step("mul_r1", step("sub_r", lo, hi), tw)
        assert all(v < 2 * g.p for v in sm + df)
        lo, hi = (sm[:128] + df[:128], sm[128:] + df[128:]) if s % 2 else (df, sm)
    out = step("mul", lo + hi, [rnd(g.p) for _ in range(512)])
    assert all(v < g.p for v in out)


def test_arguments_outside_the_table_are_refused():
    fq, fr = M.FIELD_ID["BLS12_381_FQ"], M.FIELD_ID["BLS12_381_FR"]
    z12, z8 = np.zeros((2, 8 * 12), dtype=np.uint32), np.zeros((2, 8 * 8), dtype=np.uint32)
    op = lambda n: M.TABLE[n][0]
    for field, name, z in ((fr, "mul_r", z8), (fr, "add_r", z8), (fr, "reduce_2p", z8), (fr, "half_mul_r", z8), (fq, "add_r2", z12),
                           (fq, "mul_r1", z12), (M.FIELD_ID["BN254_FQ"], "sop2", z8), (M.FIELD_ID["BN254_FQ"], "half_mul_r", z8),
                           (M.FIELD_ID["BN254_FQ"], "fp2_mul", z8)):
        rc, _ = H.relaxed_raw_op(field, op(name), z, z.shape[1] // 8)
        assert rc == -1, (field, name, rc)   # ARK_HIP_ERR_ARG
    for bad in (15, 19, 24, 40, 99, -1):
        assert H.relaxed_raw_op(fq, bad, z12, 12)[0] == -1
    assert H.relaxed_raw_op(6, op("sub_r"), z8, 8)[0] == -1
    for name in ("half_mul_r", "fp2_mul"):
        assert H.relaxed_raw_op(fq, op(name), z12[:1], 12)[0] == -1      # an odd lane count has no partner
    T = H.test_lib()
    assert T.ark_hip_test_relaxed_acc_op(1, 3, H._p(z12), H._p(z12), H._p(z12.copy()), 1) == -1
    assert T.ark_hip_test_relaxed_acc_op(5, 0, H._p(z12), H._p(z12), H._p(z12.copy()), 1) == -1
    assert T.ark_hip_test_relaxed_acc_op(1, 0, H._p(z12), None, H._p(z12.copy()), 1) == -1


# ---- accumulator level: raw XYZZ limbs in, raw XYZZ limbs out -----------------------------------------------------------------
def _acc_run(A, kind, accs, others):
    a = np.array([A.words(x) for x in accs], dtype=np.uint64).astype(np.uint32)
    o = None if kind == "canonical" else np.array([A.other_words(kind, x) for x in others], dtype=np.uint64).astype(np.uint32)
    return [A.from_words(w) for w in H.relaxed_acc_op(A.cid, M.ACC_KIND[kind], a, o).tolist()]


def _generator(A):
    G = A.C.dec(O.generator(A.cid))
    assert A.C.on_curve(G) and G is not None
    return G


def _check_output(A, got, want_acc, want_point, what):
    """device == model limb for limb; the right group element, ZZ^3 = ZZZ^2, every coordinate below 2p (a legal input again)"""
    assert got == want_acc, "%s: device %s, model %s" % (what, got, want_acc)
    assert A.affine(got) == want_point, what
    assert A.consistent(got) and A.closed(got), what


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_accumulator_ops_on_relaxed_representatives(curve):
    """valid points whose coordinates are value + j p (all four at value + p among them); y2 canonical and 2p - y; over G2 a
    base whose y has a zero component (neg_r returns 2p, beta_times its maximum); another point, the equal point (madd:
    xyzz_mdbl(x2, y2.canonical()); add: xyzz_dbl(xyzz_canonical(acc))), the inverse point (the exact (1, 1, 0, 0)),
    accumulator or operand at infinity; P and R come out as 0 in some rows and as p in others"""
    A = M.AccModel(curve)
    cases = M.acc_edge_cases(A, _generator(A))
    zero_forms = set()
    for kind in sorted({c[0] for c in cases}):
        sel = [c for c in cases if c[0] == kind]
        want = []
        for c in sel:
            A.trace = None
            want.append(A.apply(kind, c[1], c[2]))   # OutOfContract here = a case outside the contract: fails
            if c[4] in ("equal", "inverse"):
                zero_forms.add((c[4],) + tuple(v // A.g.p for t in A.trace for v in A.F.comps(t)))
        got = _acc_run(A, kind, [c[1] for c in sel], [c[2] for c in sel])
        for i, (c, w) in enumerate(zip(sel, want)):
            _check_output(A, got[i], w, c[3], "%s %s case %d (%s)" % (curve, kind, i, c[4]))
            if c[3] is None:
                assert got[i] == A.infinity()
            if kind == "canonical":
                assert all(v < A.g.p for co in got[i] for v in A.F.comps(co))
    for tag in ("equal", "inverse"):
        assert {v for f in zero_forms if f[0] == tag for v in f[1:]} == {0, 1}, (curve, tag)


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_accumulator_chains_on_raw_relaxed_state(curve):
    """64 mixed madd / add steps on 8 lanes (G2: 8 lane pairs); the relaxed device state of step i is the device input of step
    i + 1, never canonicalised in between; model and device compared after every step"""
    A = M.AccModel(curve)
    lanes, steps = 8, 64
    starts, mult, sched, pt = M.acc_chain(A, _generator(A), lanes, steps)
    dev, model, cur, hit = list(starts), list(starts), list(mult), set()
    for step, (kind, ops, ms) in enumerate(sched):
        dev = _acc_run(A, kind, dev, ops)
        for i in range(lanes):
            if cur[i] % A.C.r == 0:
                hit.add("from infinity")
            elif ms[i] % A.C.r:
                hit.add("equal" if ms[i] == cur[i] else "inverse" if ms[i] == -cur[i] else "other")
            model[i] = A.apply(kind, model[i], ops[i])
            cur[i] += ms[i]
            _check_output(A, dev[i], model[i], pt(cur[i]), "%s step %d (%s) lane %d" % (curve, step, kind, i))
    assert hit == {"equal", "inverse", "other", "from infinity"}, hit   # the schedule reaches every branch
    fin = _acc_run(A, "canonical", dev, None)
    for i in range(lanes):
        assert fin[i] == A.canonical(model[i]) and A.affine(fin[i]) == pt(cur[i])
