"""The unsigned gathered coordinate of the plain accumulate kernel's mixed addition (csrc/fp30s.cuh: from_canonical_u; ec30s.cuh),
proved on tests/lazy30_diet_model.py against tests/lazy30_model.py: the class fits every column of the three products it enters
(U2, S2, the first point's product by one), one step wider does not, the repack leaves that class and the recoded value, and the
whole addition gives lazy30_model.madd's digits with both digit signs.  And the header's host forms give the model's digits for
the new hook ops.  No GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import lazy30_diet_model as D
import lazy30_diet_rows as R
import lazy30_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF, L = M.HALF, M.L


def gathered_products():
    """the products of lazy30_model.madd_products whose first operand is a gathered coordinate, that operand in its new class"""
    return [(name, square, [D.U_CLASS, ops[1]]) for name, square, ops in M.madd_products() if name.startswith(("first", "u2", "s2"))]


def test_unsigned_gathered_class_fits_every_column():
    prods = gathered_products()
    assert [n.split(":")[0].split(" ")[0] for n, _, _ in prods] == ["first", "u2", "s2"]
    for name, square, ops in prods:
        worst = max(M.column_bounds(ops, square))
        assert worst < 1 << 63, name
        # 12 terms of 2^59 are 24 of 2^58: the two-product sum's figure
        assert worst < 2 ** 62.92, (name, math.log2(worst))
    # every other product of the addition keeps its operands and its bound
    assert len(M.madd_products()) == len(prods) + 7
    # one step wider is rejected: an unsigned operand on BOTH sides, beside an unswept difference, or in a two-product sum
    with pytest.raises(M.Overflow):
        M.column_bounds([D.U_CLASS, D.U_CLASS])
    with pytest.raises(M.Overflow):
        M.column_bounds([D.U_CLASS, M.digit_class(1, 2 * HALF)])
    with pytest.raises(M.Overflow):
        M.column_bounds([D.U_CLASS, M.digit_class(1), M.digit_class(1), M.digit_class(1)])


def test_the_repack_leaves_its_class_and_the_recoded_value():
    rng = np.random.default_rng(5)
    for row in [[M.to_words(v)] for v in (0, 1, M.P_INT - 1, (1 << 380) - 1)] + M.op_rows("from_canonical_shl", rng, 64):
        u, s = D.from_canonical_u(row[0]), M.from_canonical_shl(row[0])
        assert all(0 <= x < lim for x, lim in zip(u, D.U_CLASS))
        assert M.val(u) == M.from_words(row[0]) << M.SH == M.val(s) and M.balanced(M.val(u)) == s


def test_worst_case_digits_run_through_the_columns_without_overflow():
    """the class limits as actual operands: every unsigned digit at 2^30 - 1 against normalised digits at +-2^29, in the sign
    patterns that make every term of a column one sign; the product's digits are the closed form's"""
    top = M.top_digit_bound(1)
    u = [(1 << 30) - 1] * 12 + [(1 << 27) - 1]
    a = [HALF] * 12 + [top]
    alt = [HALF if i & 1 else -HALF for i in range(12)] + [top]
    for y in (a, M.neg(a), alt, M.neg(alt), [HALF - 1] * 12 + [top], list(M.consts()["ONE"])):
        assert M.columns(u, y) == M.mul(u, y) == M.mul(M.balanced(M.val(u)), y)
    with pytest.raises(M.Overflow):
        M.columns(u, [1 << 30] * 12 + [0])            # an unswept difference beside it
    with pytest.raises(M.Overflow):
        M.columns(u, a, a, a)                          # a two-product sum with it
    rng = np.random.default_rng(6)
    for row in M.op_rows("from_canonical_shl", rng, 32):
        u, s = D.from_canonical_u(row[0]), M.from_canonical_shl(row[0])
        for y in M.edge_digits()[:6] + M.random_digits(rng, 2):
            assert M.columns(u, y) == M.mul(s, y)


def test_the_whole_addition_gives_lazy30_models_digits_with_both_signs():
    pts = D.curve_points(12)
    ins, outs = M.madd_rows(pts)
    neg_y = lambda yw: M.to_words(M.P_INT - M.from_words(yw))
    assert any(o[-1] == 1 for o in outs) and any(o[4 * L] == 1 for o in outs)
    for row, want in zip(ins, outs):
        acc = (row[:L], row[L:2 * L], row[2 * L:3 * L], row[3 * L:4 * L], row[4 * L])
        xw, yw = row[4 * L + 1:4 * L + 13], row[5 * L + 1:5 * L + 13]
        for sign in (0, 1):
            got, eq = D.madd(acc, xw, neg_y(yw) if sign else yw, sign)
            assert eq == want[-1] and got[4] == want[4 * L]
            if not got[4]:
                assert list(got[0]) + list(got[1]) + list(got[2]) + list(got[3]) == want[:4 * L]


# ---- the header's host forms of the new hook ops against the model ---------------------------------------------------------------
@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("lazy30diet") / "lazy30_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_raw_host.hip"), "-o", exe], timeout=900)
    return exe


def run_host(exe, op, rows, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(rows, dtype=np.int32).tofile(fin)
    subprocess.run([exe, str(op), fin, fout], check=True, timeout=300)
    return np.fromfile(fout, dtype=np.int32).reshape(len(rows), -1)


def test_host_forms_of_the_new_ops_give_the_models_digits(host_runner, tmp_path):
    cases = R.raw_cases(D.curve_points(12))
    assert sorted(cases) == ["from_canonical_u", "madd_entry", "mul"]
    for op, (rows, want) in cases.items():
        got = run_host(host_runner, {**M.OPS, **D.OPS}[op], rows, tmp_path)
        R.compare(op, got, want)
