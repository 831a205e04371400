"""The differences folded into the products that compute them (csrc/fp30s.cuh: mul_sub, sqr_sub2; ec30s.cuh under
ARK_S30_FUSED_DIFF), without a GPU.

On tests/lazy30_fused_model.py against tests/lazy30_model.py: the worst case of every column of the three fused products of the
mixed addition stays below 2^63 (and the top digit inside its word), a class one step wider is rejected, and on the edge rows and 64
random rows the fused operation gives the digits of the chain it replaces, run column by column.  The header's host forms give the
same digits for the new hook ops (tests/lazy30_raw_host.hip), and tests/lazy30_fused_host_check.hip, built with every setting of
ARK_S30_FUSED_DIFF and with the undefined-behaviour and address sanitizers on its host code, leaves one and the same record of
every accumulator of its chains of additions."""
import math
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lazy30_diet_model as D
import lazy30_fused_model as FM
import lazy30_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF, L = M.HALF, M.L


def test_every_column_of_the_fused_products_fits():
    prods = FM.fused_products()
    assert [n.split(" ")[0] for n, *_ in prods] == ["pd", "rd", "x3"]
    worst = {}
    for name, square, ops, s, d in prods:
        cols, top = FM.column_bounds(ops, s, d, square)
        plain = M.column_bounds(ops, square)
        worst[name.split(" ")[0]] = max(cols)
        assert max(cols) < 1 << 63 and top < 1 << 31, name
        # what a column gains: one digit of s and two of d, and the carry that grows with them
        lim = HALF * (3 if d else 1)
        assert all(c == q for c, q in zip(cols[:L], plain[:L])), name
        assert all(0 < c - q <= lim + (lim >> (M.W - 1)) + 1 for c, q in zip(cols[L:], plain[L:])), name
    # the figures of fp30s.cuh: an unsigned gathered operand 2^62.92, a square 2^62.19; x3's 3 2^29 more change neither
    assert worst["pd"] < 2 ** 62.92 and worst["rd"] < 2 ** 62.92 and worst["x3"] < 2 ** 62.19, {k: math.log2(v) for k, v in worst.items()}


def test_a_class_one_step_wider_is_rejected():
    n = M.digit_class(1)
    wide = M.digit_class(1, 2 * HALF)                     # an unswept difference: digits up to 2^30
    with pytest.raises(M.Overflow):
        FM.column_bounds([D.U_CLASS, wide], n)            # beside the unsigned gathered operand
    with pytest.raises(M.Overflow):
        FM.column_bounds([D.U_CLASS, D.U_CLASS], n)
    with pytest.raises(M.Overflow):
        FM.column_bounds([wide], n, n, square=True)       # squared
    with pytest.raises(M.Overflow):
        FM.column_bounds([n, n], [1 << 62] * L)           # and what is subtracted has a limit too
    # as operands: the unsigned operand at its limit beside digits of 2^30 overflows a column on the way
    u = [(1 << 30) - 1] * 12 + [(1 << 27) - 1]
    with pytest.raises(M.Overflow):
        FM.columns(u, [1 << 30] * 12 + [0], [HALF] * 12 + [0])
    with pytest.raises(M.Overflow):
        FM.columns([1 << 30] * 12 + [0], None, [-HALF] * 12 + [0], [-HALF] * 12 + [0], square=True)


@pytest.mark.parametrize("op", ["mul_sub", "sqr_sub2"])
def test_fused_operation_equals_the_chain_it_replaces_digit_for_digit(op):
    rows = FM.op_rows(op, np.random.default_rng(19), 64)
    assert len(rows) >= 64 + 20
    for row in rows:
        want = FM.unfused(op, row)
        assert FM.apply(op, row) == want
        got = FM.columns(row[0], row[1], row[2]) if op == "mul_sub" else FM.columns(row[0], None, row[1], row[2], square=True)
        assert got == want, row
        assert all(-HALF <= v < HALF for v in got[:-1])


def test_edge_rows_put_every_term_of_a_high_column_on_one_side():
    """the rows the bounds are about: among the edge rows there is one whose product terms and subtracted digits all have one sign in
    every high column, in both directions, for both operations"""
    e = FM.edge_rows()
    for sign in (1, -1):
        assert any(all(a[i] * b[j] * sign > 0 for i in range(12) for j in range(12)) and all(-v * sign > 0 for v in s[:12])
                   for a, b, s in e["mul_sub"])
    assert any(all(-v > 0 for v in s[:12]) and all(-v > 0 for v in d[:12]) and all(abs(v) == HALF for v in a[:12]) for a, s, d in e["sqr_sub2"])


def test_the_addition_on_fused_operations_gives_lazy30_models_digits():
    """the model's mixed addition with pd, rd and x3 through the column schedule of the fused forms: the rows of
    lazy30_model.madd_rows, reloaded accumulators and accumulators at the limits of the invariant"""
    pts = D.curve_points(12)
    ins, outs = M.madd_rows(pts)
    xin, xout = FM.madd_extra_rows(pts)
    assert any(o[-1] == 1 for o in outs + xout) and any(o[4 * L] == 1 for o in outs + xout)
    steps = 0
    for row, want in zip(ins + xin, outs + xout):
        x, y, zz, zzz, inf = row[:L], row[L:2 * L], row[2 * L:3 * L], row[3 * L:4 * L], row[4 * L]
        if inf:
            continue
        x2 = D.from_canonical_u(row[4 * L + 1:4 * L + 13])
        y2 = D.from_canonical_u(row[5 * L + 1:5 * L + 13])
        pd, rd = FM.columns(x2, zz, x), FM.columns(y2, zzz, y)
        assert pd == M.sub(M.mul(x2, zz), x) and rd == M.sub(M.mul(y2, zzz), y)
        pp = M.sqr(pd)
        if not any(pp):
            assert want[-1] == 1 or want[4 * L] == 1
            continue
        ppp, q = M.mul(pd, pp), M.mul(x, pp)
        x3 = FM.columns(rd, None, ppp, q, square=True)
        assert x3 == want[:L]
        steps += 1
    assert steps >= 20


# ---- the header's host forms ---------------------------------------------------------------------------------------------------
def hipcc_or_skip():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def test_host_forms_of_the_new_ops_give_the_models_digits(tmp_path):
    hipcc = hipcc_or_skip()
    exe = str(tmp_path / "lazy30_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_raw_host.hip"), "-o", exe], timeout=900)
    for op in ("mul_sub", "sqr_sub2"):
        rows = FM.op_rows(op, np.random.default_rng(19), 64)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        FM.pack_rows(rows).tofile(fin)
        subprocess.run([exe, str(FM.OPS[op]), fin, fout], check=True, timeout=300)
        got = np.fromfile(fout, dtype=np.int32).reshape(len(rows), -1)
        assert np.array_equal(got, FM.pack_rows([[FM.unfused(op, r)] for r in rows])), op


def test_every_setting_of_the_build_switch_leaves_one_record(tmp_path):
    hipcc = hipcc_or_skip()

    def build_and_run(fused):
        exe, rec = str(tmp_path / ("fused%d" % fused)), str(tmp_path / ("rec%d.bin" % fused))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address",
                               "-Xarch_host", "-fno-sanitize-recover=undefined", "-DARK_S30_FUSED_DIFF=%d" % fused,
                               "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                               os.path.join(ROOT, "tests", "lazy30_fused_host_check.hip"), "-o", exe], timeout=900)
        out = subprocess.run([exe, rec], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "BLS12_381_FQ signed30 fused differences=%d: ok (0 bad" % fused in out.stdout, out.stdout
        return open(rec, "rb").read()

    with ThreadPoolExecutor(4) as pool:
        recs = list(pool.map(build_and_run, (3, 0, 1, 2)))
    assert len(recs[0]) > 1 << 18 and all(r == recs[0] for r in recs[1:])
