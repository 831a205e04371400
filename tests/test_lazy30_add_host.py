"""The full addition on 13 signed 30-bit digits (csrc/ec30s.cuh: xyzz_add_s, xyzz_dbl_s), without a GPU:

  * tests/lazy30_add_model.py restates the bounds of the addition for two operands that are both sums: every column of every
    product stays inside the signed 64-bit accumulator in the worst case its operand classes and the real digits of p allow, the
    value bounds close on the accumulator invariant of the mixed addition (so the two additions mix freely), and so do those of
    the doubling; the figures of ec30s.cuh's comments are the model's;
  * the model's digits are the field's: the addition on digits against add-2008-s on integers mod p;
  * tests/lazy30_add_host_check.hip, built with the undefined-behaviour and address sanitizers on its host code and run as a
    program: the portable forms of the addition against the 28-bit xyzz_add_lazy, canonical limb for canonical limb."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import lazy30_add_model as A
import lazy30_diet_model as D
import lazy30_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_column_of_the_full_addition_fits_the_accumulator():
    worst = A.column_maxima(A.add_products())
    assert len(worst) == 14
    for name, (col, top) in worst.items():
        assert col < 1 << 63, name
        assert top is None or top < 1 << 31, name
    # a product with one unsigned stored operand: the figure of fp30s.cuh's exception (2^62.92); everything else a plain product's
    # (2^62.3) but the two-product sum (30.8 x 2^58)
    for name, (col, _) in worst.items():
        unsigned = name.split(":")[0].split(" =")[0] in ("copy", "u1", "s1", "pd", "rd", "zz12")
        limit = 2 ** 62.92 if unsigned else 30.8 * 2 ** 58 if name.startswith("y3") else 2 ** 62.3
        assert col < limit, (name, col / 2 ** 58)
    # accumulator + accumulator: b normalised and inside the invariant, every product a plain one
    v = A.add_value_chain(b=M.INV_X)
    for name, (col, top) in A.column_maxima(A.add_products(v, b_class=M.digit_class(M.INV_X))).items():
        assert col < (30.8 * 2 ** 58 if name.startswith("y3") else 2 ** 62.3), name


def test_value_bounds_of_the_full_addition_close_on_the_invariant():
    v = A.add_value_chain()
    assert v["x3"] <= M.INV_X and v["y3"] <= M.INV_Y and v["zz3"] <= M.INV_Z and v["zzz3"] <= M.INV_Z
    assert v["copy"] <= M.INV_Y <= M.INV_X and v["copy"] <= M.INV_Z        # an empty accumulator taking b
    assert v["pp"] < 1 and v["rr"] < 1                                        # the zero tests are exact
    # sop2's operands have top digits below 2^27, and far below: |value| < 2.63 p as in the mixed addition
    assert all(v[k] < Fraction(263, 100) for k in ("rd", "t", "s1", "ppp"))
    assert all(M.top_digit_bound(v[k]) < 1 << 23 for k in ("rd", "t", "s1", "ppp"))
    # every coordinate leaves through to_canonical's window
    assert max(v["x3"], v["y3"], v["zz3"], v["copy"]) < M.consts()["OUT_K"]
    # the figures in ec30s.cuh's comments
    doc = dict(u1=0.706, s1=0.563, u2=0.602, pd=1.308, rd=1.165, pp=0.5029, rr=0.5023, ppp=0.5012, q=0.5007, x3=2.006, t=2.507,
               y3=0.5053, zz12=0.602, zz3=0.5006, zzz3=0.5006, copy=0.602)
    for k, lim in doc.items():
        assert v[k] < Fraction(lim).limit_denominator(10 ** 6), (k, float(v[k]), lim)
    # an accumulator + an accumulator is narrower in every value
    w = A.add_value_chain(b=M.INV_X)
    assert all(w[k] <= v[k] for k in v)
    # outside the invariant nothing closes
    assert A.add_value_chain(x=Fraction(2000))["x3"] > M.INV_X


def test_the_doubling_fits_the_accumulator_and_closes_on_the_invariant():
    v = A.dbl_value_chain()
    assert v["x3"] <= M.INV_X and v["y3"] <= M.INV_Y and v["zz3"] <= M.INV_Z and v["zzz3"] <= M.INV_Z
    # the two swept sums take digits up to 2^30 (u = y + y) and 3 2^29 (m = xx + 2 xx): the classes of FpS::sweep
    doc = dict(u=1.22, v=0.5025, w=0.5011, s=0.5018, xx=0.5066, m=1.52, x3=1.508, t=2.01, y3=0.5055, zz3=0.501, zzz3=0.501)
    for k, lim in doc.items():
        assert v[k] <= Fraction(lim).limit_denominator(10 ** 6), (k, float(v[k]), lim)
    assert all(M.top_digit_bound(v[k]) < 1 << 23 for k in ("m", "t", "w"))
    for name, (col, top) in A.column_maxima(A.dbl_products()).items():
        assert col < (30.8 * 2 ** 58 if name.startswith("y3") else 2 ** 62.3), name
        assert top is None or top < 1 << 31
    # digit for digit the field's doubling, and what the addition of equal points returns
    rinv = pow(1 << 384, -1, M.P_INT)
    pts = D.curve_points(6)
    one_words = M.to_words((1 << 384) % M.P_INT)
    empty = ([0] * M.L,) * 4 + (1,)
    for i in range(5):
        a4 = [pts[i][0], pts[i][1], one_words, one_words]
        acc = A.add(A.add(empty, A.operands_of(a4)), A.operands_of([pts[i + 1][0], pts[i + 1][1], one_words, one_words]))
        got = A.double(acc)
        assert tuple(A.residue(c) for c in got[:4]) == A.field_double([A.residue(c) for c in acc[:4]])
        assert all(-M.HALF <= d < M.HALF for c in got[:4] for d in c[:-1])
        stored = A.operands_of([M.to_canonical(c) for c in acc[:4]])          # the same point from memory
        assert A.add(acc, stored) == got and A.add(acc, A.add(empty, stored)) == got


def test_the_models_addition_is_the_fields():
    rng = np.random.default_rng(5)
    rnd = lambda: int.from_bytes(rng.bytes(48), "little") % M.P_INT
    rinv = pow(1 << 384, -1, M.P_INT)
    pts = D.curve_points(8)
    one_words = M.to_words((1 << 384) % M.P_INT)
    cases = [([pts[i][0], pts[i][1], one_words, one_words], [pts[i + 1][0], pts[i + 1][1], one_words, one_words]) for i in range(6)]
    cases += [([M.to_words(rnd()) for _ in range(4)], [M.to_words(rnd()) for _ in range(4)]) for _ in range(24)]
    for a4, b4 in cases:
        acc = A.add(([0] * M.L,) * 4 + (1,), A.operands_of(a4))          # an empty accumulator takes a
        assert [A.residue(c) for c in acc[:4]] == [M.from_words(w) * rinv % M.P_INT for w in a4]
        want = A.field_add([M.from_words(w) * rinv % M.P_INT for w in a4], [M.from_words(w) * rinv % M.P_INT for w in b4])
        for other in (A.operands_of(b4), A.add(([0] * M.L,) * 4 + (1,), A.operands_of(b4))):   # from memory, from an accumulator
            got = A.add(acc, other)
            assert got[4] == 0 and tuple(A.residue(c) for c in got[:4]) == want
            assert all(-M.HALF <= d < M.HALF for c in got[:4] for d in c[:-1])
            v = A.add_value_chain()
            for c, k in zip(got[:4], ("x3", "y3", "zz3", "zzz3")):
                assert abs(M.val(c)) < v[k] * M.P_INT
    # the special cases
    a4 = [pts[2][0], pts[2][1], one_words, one_words]
    neg = [a4[0], M.to_words(M.P_INT - M.from_words(a4[1])), one_words, one_words]
    inf4 = [one_words, one_words, [0] * M.N32, [0] * M.N32]
    acc = A.add(([0] * M.L,) * 4 + (1,), A.operands_of(a4))
    assert A.add(acc, A.operands_of(a4)) == A.double(acc)
    assert A.add(acc, A.operands_of(neg))[4] == 1
    assert A.add(acc, A.operands_of(inf4)) == acc
    assert A.add(([0] * M.L,) * 4 + (1,), A.operands_of(inf4))[4] == 1


@pytest.mark.parametrize("op", ["add_full", "add_full_acc"])
def test_host_twin_of_the_raw_hook_is_the_oracles(op, tmp_path):
    """the rows tests/test_gpu_reduce_s30.py sends to the device, through the portable forms (tests/lazy30_raw_host.hip)"""
    import reduce_s30_rows as R
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "lazy30_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_raw_host.hip"), "-o", exe], timeout=900)
    ps = R.pairs()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.packed_rows(ps).tofile(fin)
    subprocess.run([exe, str(A.OPS[op]), fin, fout], check=True, timeout=300)
    R.check_against_oracle(ps, np.fromfile(fout, dtype=np.int32).reshape(len(ps), A.ADD_OUT))


def test_full_addition_on_the_host_equals_the_28_bit_one_limb_for_limb(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "add_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "algebra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lazy30_add_host_check.hip"), "-o", exe], timeout=900)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "signed30 full addition: ok (0 bad of" in out.stdout, out.stdout
