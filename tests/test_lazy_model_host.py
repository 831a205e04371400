"""tests/lazy_model.py -- the exact model of the carry-free limb arithmetic -- checked WITHOUT a GPU:

  * against itself where two formulations exist, and against pyref.Fld / pyref.Curve for residues and group elements;
  * against the header's HOST forms: tests/lazy_raw_host.hip (built here with hipcc) reads the raw-limb vector files the GPU
    module (tests/test_gpu_lazy_classes.py) sends to the device and writes raw-limb results, for the prime-field ops and the G1
    accumulator ops -- so the vectors, their preconditions and the expected results are validated before a GPU is involved;
  * its geometry against csrc/params.hpp, its op table against the kernels' call sites, and the table of documented bounds
    (operand classes and output bounds as the comments state them, file and line) against an exact re-derivation.

Every comparison is exact equality of integers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lazy_model as M
import oracle_lib as O
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algebra_amd", "csrc")
NRAND = 4096   # the GPU module's count: the files are the same


@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("lazy_raw") / "lazy_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "lazy_raw_host.hip"), "-o", exe], timeout=600)
    return exe


def _run_host(exe, tmp_path, records):
    """records: [(kind, id, op, k, h, n, input array, output shape)] -> list of output arrays"""
    vec, res = str(tmp_path / "vectors.bin"), str(tmp_path / "results.bin")
    with open(vec, "wb") as f:
        for kind, ident, op, k, h, n, arr, oshape in records:
            arr = np.ascontiguousarray(arr, dtype=np.uint32)
            f.write(np.array([kind, ident, op, k, h, n, arr.size, int(np.prod(oshape))], dtype=np.int32).tobytes())
            f.write(arr.tobytes())
    out = subprocess.run([exe, vec, res], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "%d records" % len(records)
    flat = np.fromfile(res, dtype=np.uint32)
    outs, off = [], 0
    for r in records:
        size = int(np.prod(r[7]))
        outs.append(flat[off:off + size].reshape(r[7]))
        off += size
    assert off == flat.size
    return outs


# ---- geometry, op table, call sites ------------------------------------------------------------------------------------------
def test_geometry_derived_from_p_matches_params_header():
    lz = M.parse_params_lz()
    assert set(lz) == set(P.FIELD_ORDER)
    for name, d in lz.items():
        g = M.GEO[name]
        assert (d["N"], d["LZ_W"], d["LZ_L"]) == (g.N, g.W, g.L), name
        assert d["LZ_INV"] == g.INV and (g.INV * g.p + 1) % (1 << g.W) == 0, name
        assert d["LZ_RP"] == g.RP and d["LZ_CIN"] == g.CIN, name
        assert g.SH == g.W * g.L - 32 * g.N and 0 <= g.SH < g.W, name
        assert d["LZ_KP"] == [g.kp(k) for k in range(9)], name
        for k in (2, 3, 4, 6, 8):
            for h in (1, 2, 3):   # a spread k p is the same integer, and never lends more than it has
                assert g.val(g.spread(k, h)) == k * g.p and min(g.spread(k, h)) >= 0, (name, k, h)


def test_op_table_is_what_the_host_runner_serves(host_runner):
    out = subprocess.run([host_runner, "--table"], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = {}
    for line in filter(None, out):
        tok = line.split()
        seen[tok[1]] = (int(tok[0]), int(tok[2]), [tuple(int(v) for v in t.split(":")) for t in tok[3:]] or [(0, 0)])
    assert seen == {n: (r["op"], r["arity"], r["params"]) for n, r in M.TABLE.items()}


def _call_site_parameters():
    """every numeric template parameter at a call into FpL / Fp2L / Fft29 in the kernels' headers -> {(table name, k, h)}"""
    found = set()
    pat = re.compile(r"\b(\w+)::template (\w+)<([^<>]*)>\(|\.template (shr_mod)<([^<>]*)>\(\)")
    for fname in ("ec28.cuh", "ec28x2.cuh", "fp28x2.cuh", "fft.cuh", "devops.cuh", "lazyk.cuh", "msm.cuh", "batchmul.cuh"):
        for line in open(os.path.join(CSRC, fname)):
            code = line.split("//")[0]
            for m in pat.finditer(code):
                if m.group(4):
                    continue   # shr_mod<SH>: the field's own shift, served as k = SH
                cls, fn, args = m.group(1), m.group(2), [a.strip() for a in m.group(3).split(",")]
                if not all(re.fullmatch(r"\d+", a) for a in args):
                    continue   # a forwarding template (Fp2L::sub_sweep<K> -> FpL::sub_sweep<K>): its callers are counted
                ks = [int(a) for a in args]
                x2 = fname == "ec28x2.cuh" and cls == "F"
                if fn == "dif":
                    found.add(("dif", ks[0], ks[1]))
                elif x2 and fn == "mul_sub":
                    found.update({("x2_mul_sub", ks[0], ks[1]), ("x2_beta_neg", ks[0], 0), ("neg_semi", ks[1], 0), ("sop4", 0, 0)})
                elif x2 and fn in ("mul", "sqr"):
                    found.update({("x2_" + fn, ks[0], 0), ("x2_beta_neg", ks[0], 0)})
                elif x2:
                    found.update({("x2_" + fn, ks[0], 0), (fn, ks[0], 0)})
                elif fn == "sub_op":
                    found.update({("sub_op", ks[0], 0), ("sub_semi", ks[0], 0), ("sub_sweep", ks[0], 0)})
                else:
                    found.add((fn, ks[0], 0))
    return found


def test_every_call_site_parameter_is_in_the_op_table():
    found = _call_site_parameters()
    assert {f[0] for f in found} >= {"sub", "sub_semi", "sub_sweep", "sub_op", "sub_b_2c_norm", "neg", "neg_semi", "dif", "x2_mul",
                                     "x2_sqr", "x2_mul_sub", "x2_sub_sweep", "x2_sub_b_2c_norm"}, "the search lost a function"
    for name, k, h in sorted(found):
        assert name in M.TABLE and (k, h) in M.TABLE[name]["params"], "call-site parameter missing from THE TABLE: %s<%d,%d>" % (name, k, h)
    # and nothing is instantiated that no call site (or, for the three functions without one, tests/lazy_host_check.hip) uses
    free = {"negsub", "cond_neg_semi", "shr_mod"}
    for name, row in M.TABLE.items():
        if row["templated"] and name not in free:
            for k, h in row["params"]:
                assert (name, k, h) in found, "THE TABLE instantiates %s<%d,%d>, which no call site uses" % (name, k, h)


# ---- the model against itself and against pyref ------------------------------------------------------------------------------
@pytest.mark.parametrize("field", P.FIELD_ORDER)
def test_model_formulations_agree(field):
    g = M.GEO[field]
    cl = M.classes(g)
    F = P.Fld(g.p)
    rng = np.random.default_rng(5)
    res = g.residue
    ns = cl["n"].extremes() + cl["n"].random(rng, 64)
    for i, a in enumerate(ns):
        b, c, d = ns[(i + 7) % len(ns)], ns[(i + 13) % len(ns)], ns[(i + 29) % len(ns)]
        assert g.sqr(a) == g.mul(a, a)                                     # limb for limb
        assert res(g.mul(a, b)) == F.mul(res(a), res(b))
        assert res(g.sop2(a, b, c, d)) == F.add(res(g.mul(a, b)), res(g.mul(c, d)))
        assert res(g.add_lazy(a, b)) == F.add(res(a), res(b))
        assert g.val(g.mul(a, b)) * g.R % g.p == g.val(a) * g.val(b) % g.p and g.val(g.mul(a, b)) < g.val(a) * g.val(b) // g.R + g.p + 1
        w = g.pack32(cl["w32"].from_value(g.val(a) % (1 << (32 * g.N))))
        assert g.pack32(g.unpack32(w)) == w and g.val(g.unpack32_shl(w)) == g.from_words(w) << g.SH
    for k in (2, 3, 6):
        sub = cl["n<%d" % k]
        for a, b in zip(ns, sub.extremes() + sub.random(rng, 64)):
            semi, swept = g.sub_semi(k, a, b), g.sub_sweep(k, a, b)
            assert g.val(semi) == g.val(swept) == g.val(a) - g.val(b) + k * g.p
            assert max(semi) < (3 << g.W) and g.normalised(swept[:-1])     # "semi-normalised" is what the products were sized for
            assert res(swept) == F.sub(res(a), res(b))
            assert g.val(g.neg_semi(k, b)) == k * g.p - g.val(b) and max(g.neg_semi(k, b)) < (2 << g.W)
    for a in cl["n"].random(rng, 64):
        assert g.val(g.shr_mod(g.SH, a)) * (1 << g.SH) % g.p == g.val(a) % g.p and g.val(g.shr_mod(g.SH, a)) <= g.val(a) // (1 << g.SH) + g.p
    if g.NB:
        F2 = P.Fld(g.p, -g.NB)
        el = lambda A: (res(A[0]), res(A[1]))
        for i in range(0, len(ns) - 4, 3):
            A, B = (ns[i], cl["n<2"].from_value(g.val(ns[i + 1]))), (ns[i + 2], ns[i + 3])
            assert el(g.x2_mul(2, A, B)) == F2.mul(el(A), el(B))
            S = (cl["n<2"].from_value(g.val(ns[i])), cl["n<2"].from_value(g.val(ns[i + 1])))
            sq, zero = g.x2_sqr(2, S)
            assert el(sq) == F2.mul(el(S), el(S)) and zero == int(el(S) == (0, 0))
            Y, D = (cl["n<2"].from_value(g.val(ns[i + 3])), cl["n<2"].from_value(g.val(ns[i + 4]))), (ns[i + 1], ns[i])
            assert el(g.x2_mul_sub(4, 2, (A[0], cl["n<4"].from_value(g.val(A[1]))), B, Y, D)) == \
                F2.sub(F2.mul((res(A[0]), res(cl["n<4"].from_value(g.val(A[1])))), el(B)), F2.mul(el(Y), el(D)))


@pytest.mark.parametrize("field", P.FIELD_ORDER)
def test_generators_stay_inside_their_class(field):
    g = M.GEO[field]
    rng = np.random.default_rng(6)
    for name, c in M.classes(g).items():
        ex = c.extremes()
        assert [0] * g.L in ex
        if c.capped:
            assert max(g.val(l) for l in ex) == c.vmax - 1, name          # the largest value the class admits is there
        else:
            assert [c.M - 1] * g.L in ex, name                           # every limb at the class maximum
        for l in ex + c.random(rng, 200):
            assert c.contains(l), (field, name, l)


# ---- the model against the header's host forms, on the GPU module's vector files -----------------------------------------------
@pytest.mark.parametrize("field", P.FIELD_ORDER)
def test_host_forms_match_model_on_the_gpu_vectors(field, host_runner, tmp_path):
    g = M.GEO[field]
    records, wants = [], []
    for name, k, h in M.all_field_ops(field):
        rows = M.field_vectors(field, name, k, h, NRAND)
        exp = M.expected(field, name, k, h, rows)   # a vector outside its op's precondition raises: nothing is dropped
        arr = M.rows_to_array(g, rows)
        records.append((0, M.FIELD_ID[field], M.TABLE[name]["op"], k, h, len(rows), arr, (len(rows), g.L + 1)))
        wants.append(((name, k, h), M.expected_to_array(g, exp)))
    for (what, want), got in zip(wants, _run_host(host_runner, tmp_path, records)):
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, "%s %s: %d rows differ; first %d: host %s, model %s" % (
            field, what, bad.size, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


def test_fp2_vectors_are_inside_their_contract():
    """Fp2L is device code: no host form to compare with, but every vector the GPU module sends passes its preconditions here"""
    for field in M.NEG_BETA:
        for name, k, h in M.all_x2_ops():
            rows, exp = M.x2_vectors(field, name, k, h, 256)
            assert len(rows) == len(exp) and len(rows) % 2 == 0


def _generator(A):
    G = A.C.dec(O.generator(A.cid))
    assert G is not None and A.C.on_curve(G)
    return G


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_accumulator_model_against_the_group_law(curve, host_runner, tmp_path):
    """edge cases and chains on the model: the right group element (pyref.Curve), ZZ^3 = ZZZ^2, closure of the invariant,
    canonical buckets; for the G1 curves the same files through the host forms of ec28.cuh, limb for limb"""
    A = M.AccModel(curve)
    G = _generator(A)
    cases = M.acc_edge_cases(A, G)
    outs = [M.acc_apply(A, c[0], c[1], c[2]) for c in cases]
    for c, o in zip(cases, outs):
        assert A.affine(o) == c[3] and A.consistent(o) and A.in_invariant(o), (curve, c[0])
        b = A.to_bucket(o)
        assert M.bucket_point(A, b) == c[3]
        assert all(A.g.from_words(b[i * A.g.N:(i + 1) * A.g.N]) < A.g.p for i in range(4 * A.ext))
    starts, mult, sched, pt = M.acc_chain_ops(A, G, 8, 64)
    state, cur, chain_records = list(starts), list(mult), []
    for kind, ops, ms in sched:
        before = list(state)
        for i in range(len(state)):
            state[i] = M.acc_apply(A, kind, state[i], ops[i])
            cur[i] = cur[i] - ms[i] if kind == "msub" else cur[i] + ms[i]
            assert A.affine(state[i]) == pt(cur[i]) and A.consistent(state[i]) and A.in_invariant(state[i]), (curve, kind, i)
        chain_records.append((kind, before, ops, list(state)))
    if A.ext == 2:
        return   # ec28x2.cuh is device code
    records, wants = [], []
    groups = [(k, [c[1] for c in cases if c[0] == k], [c[2] for c in cases if c[0] == k], [o for c, o in zip(cases, outs) if c[0] == k])
              for k in sorted({c[0] for c in cases})] + chain_records
    groups.append(("to_bucket", outs, None, None))
    for kind, accs, others, want in groups:
        a, o, ow = M.acc_pack(A, kind, accs, others)
        arr = a.reshape(-1) if o is None else np.concatenate([a.reshape(-1), o.reshape(-1)])
        records.append((1, A.cid, M.ACC_KIND[kind], 0, 0, len(accs), arr, (len(accs), ow)))
        wants.append(np.array([A.to_bucket(x) for x in accs] if kind == "to_bucket" else [A.park(x) for x in want], dtype=np.uint64))
    for (kind, accs, _, _), want, got in zip(groups, wants, _run_host(host_runner, tmp_path, records)):
        for i in range(len(accs)):
            if kind != "to_bucket" and want[i][-1] == 1 and got[i][-1] == 1:
                continue   # at infinity the coordinates carry no meaning
            assert got[i].tolist() == want[i].tolist(), (curve, kind, i)


# ---- the table of documented bounds ------------------------------------------------------------------------------------------
def _figure_on_line(where, value):
    fname, line = where.split(":")
    text = open(os.path.join(CSRC, fname)).read().split("\n")[int(line) - 1]
    return re.search(r"(?<![\d.])" + re.escape(str(value)) + r"(?!\d)", text) is not None, text


def test_documented_figures_are_the_comments_own():
    for doc in (M.DOC_G1_28, M.DOC_G1_29, M.DOC_G2, M.DOC_FFT):
        for name, (lo, hi, where) in doc.items():
            for v in (lo, hi):
                if v != 0:
                    ok, text = _figure_on_line(where, v)
                    assert ok, "%s: the comment no longer states %s for %s: %s" % (where, v, name, text.strip())


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_documented_bounds_contain_the_derived_ones(curve):
    """every figure of the comments, re-derived exactly from the accumulator invariant with the field's own R' / p; the
    invariant itself is closed (what an addition leaves is a legal input again)"""
    rows = M.documented_bounds(curve)
    assert len(rows) >= 20
    for where, name, doc, der in rows:
        assert doc[0] <= der[0] and der[1] <= doc[1], "%s %s: documented (%s, %s), derived (%.4f, %.4f)" % (
            where, name, doc[0], doc[1], float(der[0]), float(der[1]))


@pytest.mark.parametrize("field", M.FR_FIELDS)
def test_fft29_table(field):
    g = M.GEO[field]
    for where, name, doc, der in M.documented_fft_bounds(field):
        assert der[1] <= doc[1], (where, name, float(der[1]))
    # reduce_sweep on everything the pass feeds it (limbs below 2^31, value below 13.02 p): normalised, the same residue,
    # below 3 p -- so that canon's two conditional subtractions end in [0, p)
    c = M.classes(g)["f31<13"]
    for l in c.extremes() + c.random(np.random.default_rng(8), 2000):
        r = g.fft_reduce_sweep(l)
        assert g.normalised(r) and g.val(r) % g.p == g.val(l) % g.p and g.val(r) < 3 * g.p
        assert g.val(g.fft_canon(l)) == g.val(l) % g.p
