"""The bounds of the signed 13 x 30-bit form (csrc/fp30s.cuh, ec30s.cuh), proved on the Python model of tests/lazy30_model.py:
every column of every product of the mixed addition stays inside the signed 64-bit accumulator in the WORST case its operand
classes and the real digits of p allow; the value bounds chain through one mixed addition and close on the accumulator
invariant; a class one step too wide is rejected.  And the model is the header: the host twins give its digits.  No GPU."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import lazy30_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_what_they_claim():
    c = M.consts()
    assert (c["W"], c["L"]) == (M.W, M.L)
    assert c["P"] == M.PD == M.balanced(M.P_INT) and M.val(c["P"]) == M.P_INT
    assert (c["INV"] * M.P_INT + 1) % (1 << M.W) == 0
    assert c["ONE"] == M.balanced(pow(2, M.RBITS, M.P_INT))
    assert c["OUT_KP"] == M.balanced(c["OUT_K"] * M.P_INT)
    assert all(-M.HALF <= d < M.HALF for d in c["P"][:-1] + c["ONE"][:-1] + c["OUT_KP"][:-1])
    # the generator emits exactly this struct
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_constants", os.path.join(ROOT, "tools", "gen_constants.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    assert g.signed_digits(M.P_INT, M.L, M.W) == M.PD and g.S30_OUT_K == c["OUT_K"] and g.S30_FIELDS == ["BLS12_381_FQ"]


def test_every_column_of_the_mixed_addition_fits_the_accumulator():
    worst = {}
    for name, square, ops in M.madd_products():
        worst[name] = max(M.column_bounds(ops, square))
        assert worst[name] < 1 << 63, name
    # the figures of fp30s.cuh's header: one product below 2^62.3, the two-product sum below 30.8 x 2^58
    assert all(v < 2 ** 62.3 for n, v in worst.items() if not n.startswith("y3")), worst
    assert worst["y3 = rd t - y1 ppp"] < 30.8 * 2 ** 58
    # the sum of |p_j| the header quotes
    assert sum(abs(d) for d in M.PD) < 6.21 * M.HALF


def test_worst_case_digits_run_through_the_columns_without_overflow():
    """the class limits as actual operands: every digit at +-2^29 in the sign pattern that makes every term of a column positive"""
    b = M.madd_value_chain()
    top = M.top_digit_bound(b["pd"])
    a = [M.HALF] * 12 + [top]
    for x in (a, M.neg(a), [M.HALF if i & 1 else -M.HALF for i in range(12)] + [top]):
        for y in (a, M.neg(a)):
            assert M.columns(x, y) == M.mul(x, y)
            assert M.columns(x, None, square=True) == M.sqr(x)
            assert M.columns(x, y, x, y) == M.sop2(x, y, x, y)       # 26 terms of one sign


def test_value_bounds_chain_through_one_addition_and_close():
    b = M.madd_value_chain()
    # the outputs of addition t are admissible inputs of addition t + 1
    assert b["x3"] <= M.INV_X and b["y3"] <= M.INV_Y and b["zz3"] <= M.INV_Z and b["zzz3"] <= M.INV_Z
    # so are the first point of a bucket and a reloaded bucket (one product with the residue 1 < p; zz = zzz = the residue 1)
    assert b["first"] <= M.INV_Y <= M.INV_X and M.val(M.consts()["ONE"]) < M.P_INT
    # the exact zero tests: PP and R^2 are below p in magnitude
    assert b["pp"] < 1 and b["rr"] < 1
    # every coordinate leaves through to_canonical's window
    assert max(M.INV_X, M.INV_Y, M.INV_Z) < M.consts()["OUT_K"]
    # sop2's operands have top digits below 2^27 (the class its column bound is written for), the base's too
    assert all(M.top_digit_bound(b[k]) < 1 << 27 for k in ("rd", "t", "ppp")) and M.top_digit_bound(M.INV_Y) < 1 << 27
    assert M.top_digit_bound(M.BASE) <= (1 << 27) + 1
    # the figures in ec30s.cuh's comments
    doc = dict(u2=0.602, pd=2.63, rd=1.22, pp=0.5111, rr=0.5025, ppp=0.5023, q=0.5018, e=1.506, x3=2.009, t=2.511, y3=0.506,
               zz3=0.501, zzz3=0.501, first=0.602)
    for k, v in doc.items():
        assert b[k] < Fraction(v).limit_denominator(10 ** 6), (k, float(b[k]), v)
    # R' / p
    assert M.RHO > Fraction(6299, 10)


def test_a_class_one_step_too_wide_is_rejected():
    b = M.madd_value_chain()
    n = lambda v: M.digit_class(v)
    wide = lambda v: M.digit_class(v, 2 * M.HALF)         # an UNSWEPT difference of two normalised values: digits up to 2^30
    M.column_bounds([n(b["rd"]), n(b["t"]), n(M.INV_Y), n(b["ppp"])])
    with pytest.raises(M.Overflow):
        M.column_bounds([wide(b["rd"]), n(b["t"]), n(M.INV_Y), n(b["ppp"])])
    with pytest.raises(M.Overflow):
        M.column_bounds([wide(b["pd"]), wide(b["pp"])])   # two unswept operands: 12 x 2^60
    with pytest.raises(M.Overflow):
        M.column_bounds([wide(b["pd"])], square=True)
    # and as digits: unswept operands overflow a real column
    a = [2 * M.HALF] * 12 + [1 << 20]
    with pytest.raises(M.Overflow):
        M.columns(a, a)
    # a sop2 operand with a full-size top digit (which no value below 64 p has) is one step too wide as well
    with pytest.raises(M.Overflow):
        M.column_bounds([[M.HALF] * 13] * 4)
    # an accumulator outside the invariant does not close
    assert M.madd_value_chain(x=Fraction(700))["x3"] > M.INV_X


def test_columns_and_closed_form_agree():
    rng = np.random.default_rng(3)
    for op in ("mul", "sqr", "sop2"):
        for row in M.op_rows(op, rng, 32):
            got = M.columns(row[0], None, square=True) if op == "sqr" else M.columns(*row)
            want = M.apply(op, row)
            assert got == want
            assert all(-M.HALF <= d < M.HALF for d in want[:-1])
            T = M.val(row[0]) ** 2 if op == "sqr" else sum(M.val(row[i]) * M.val(row[i + 1]) for i in range(0, len(row), 2))
            assert (M.val(want) << M.RBITS) % M.P_INT == T % M.P_INT
            assert abs(M.val(want)) * (1 << M.RBITS) <= abs(T) + M.P_INT * (M.HALF * ((1 << M.RBITS) - 1) // ((1 << M.W) - 1))


@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("lazy30") / "lazy30_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_raw_host.hip"), "-o", exe], timeout=900)
    return exe


def run_host(exe, op, rows, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(rows, dtype=np.int32).tofile(fin)
    subprocess.run([exe, str(M.OPS[op]), fin, fout], check=True, timeout=300)
    return np.fromfile(fout, dtype=np.int32).reshape(len(rows), -1)


@pytest.mark.parametrize("op", ["mul", "sqr", "sop2", "sub", "add_2b", "from_canonical_shl", "to_canonical"])
def test_host_twins_give_the_models_digits(op, host_runner, tmp_path):
    rows = M.op_rows(op, np.random.default_rng(11))
    got = run_host(host_runner, op, M.pack_rows(op, rows), tmp_path)
    want = M.pack_rows("sqr", [[M.apply(op, r)] for r in rows])
    assert np.array_equal(got, want)
