"""tests/relaxed_model.py -- the exact model of the relaxed [0, 2p) arithmetic on saturated 32-bit limbs -- checked WITHOUT a GPU:

  * against pyref (residues, Fp2 products, group elements) and against its own contracts: every vector list the GPU module
    (tests/test_gpu_relaxed_classes.py) sends passes every precondition, and every model result is in its documented class;
  * against the header's HOST forms: tests/relaxed_raw_host.hip (built here with hipcc) reads the same vector files.  The ARK_HD
    limb functions are the statements the device runs and are compared exactly; the host products return canonical values
    and are compared as residues, the xyzz_*_relaxed host forms over the G1 fields as group elements;
  * its op table against the header and against a search of the kernels' call sites, and the table of documented bounds
    (file, line, the comment's own words) against an exact re-derivation from p;
  * two value-level mutants of the model that stand in for device-only code (FOLD, beta_times) must break closure or residue
    on a listed edge row.

Every comparison is exact equality of integers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pyref as P
import relaxed_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algebra_amd", "csrc")
NRAND = 4096   # the GPU module's count: the files are the same
HOST_UNITS = (M.U_FP, M.U_FP2)   # Fp2Half is device code
FIELD_OPS = [(f, n) for f in P.FIELD_ORDER for n in M.ops_of(f)]


@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("relaxed_raw") / "relaxed_raw_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "relaxed_raw_host.hip"), "-o", exe], timeout=600)
    return exe


def _run_host(exe, tmp_path, records):
    """records: [(kind, id, op, n, input array, output shape)] -> list of output arrays"""
    vec, res = str(tmp_path / "vectors.bin"), str(tmp_path / "results.bin")
    with open(vec, "wb") as f:
        for kind, ident, op, n, arr, oshape in records:
            arr = np.ascontiguousarray(arr, dtype=np.uint32)
            f.write(np.array([kind, ident, op, 0, 0, n, arr.size, int(np.prod(oshape))], dtype=np.int32).tobytes())
            f.write(arr.tobytes())
    out = subprocess.run([exe, vec, res], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "%d records" % len(records)
    flat = np.fromfile(res, dtype=np.uint32)
    outs, off = [], 0
    for r in records:
        size = int(np.prod(r[5]))
        outs.append(flat[off:off + size].reshape(r[5]))
        off += size
    assert off == flat.size
    return outs


# ---- op table and call sites -----------------------------------------------------------------------------------------------------
def test_op_table_is_what_the_host_runner_serves(host_runner):
    out = subprocess.run([host_runner, "--table"], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = {}
    for line in filter(None, out):
        op, name, arity, unit, fields = line.split()
        seen[name] = (int(op), int(arity), int(unit), int(fields))
    assert seen == {n: r[:4] for n, r in M.TABLE.items()}


def _call_sites():
    """every call into the relaxed arithmetic in the kernels' headers -> {(function, "base" | "scalar" | "ext")}: ec.cuh, msm.cuh,
    batchmul.cuh and gfft.cuh run over the base fields (F = Fp, and Fp2Half over the two with an extension), fft.cuh over the
    scalar fields, the bodies of Fp2 / Fp2Half in fp.cuh over the base fields with an extension"""
    pat = re.compile(r"\b[FB]::(?:template )?(\w+)(?:<[^<>()]*>)?\(|\.(canonical|is_zero_mod_p)\(\)|(?<![:\w])(beta_times|neg_beta_times_neg)\(")
    wanted = re.compile(r"\w+_r[12]?$|reduce_2p$|is_zero_mod_p$|canonical$|sop2(_call)?$|beta_times$|neg_beta_times_neg$")
    found = set()
    for fname, where in (("ec.cuh", "base"), ("msm.cuh", "base"), ("batchmul.cuh", "base"), ("gfft.cuh", "base"), ("fft.cuh", "scalar"),
                         ("fp.cuh", "ext")):
        inside = where != "ext"
        for line in open(os.path.join(CSRC, fname)):
            if not inside:
                inside = line.startswith("struct Fp2 {")
                continue
            code = line.split("//")[0]
            if "ARK_HD static" in code or "ARK_DEV static" in code or "ARK_HD bool" in code or "ARK_DEV bool" in code:
                code = code.split("{", 1)[1] if "{" in code else ""   # a definition's own name is no call
            for m in pat.finditer(code):
                name = m.group(1) or m.group(2) or m.group(3)
                if wanted.match(name):
                    found.add((name.replace("_call", ""), where))
    return found


def test_every_relaxed_call_site_is_in_the_op_table():
    found = _call_sites()
    assert found >= {("mul_r", "base"), ("sqr_r", "base"), ("sub_r", "base"), ("dbl_r", "base"), ("neg_r", "base"), ("sop2_r", "base"),
                     ("is_zero_mod_p", "base"), ("canonical", "base"), ("add_r2", "scalar"), ("sub_r", "scalar"), ("mul_r1", "scalar"),
                     ("sop2", "ext"), ("neg_beta_times_neg", "ext"), ("sop4_r", "ext"), ("beta_times", "ext"), ("add_r", "ext"),
                     ("mul_r", "ext")}, "the search lost a function"
    mask = {"base": M.M_BASE, "scalar": M.M_SCALAR, "ext": M.M_EXT}
    componentwise = {"add_r", "sub_r", "dbl_r"}     # Fp2Half forwards these to Fp per lane: the Fp row is the test
    for name, where in sorted(found):
        if name == "sop4_r":
            row = "half_sop2_r"                     # its one caller, with the FOLD of that call site
        elif name == "beta_times":
            row = "half_beta_times"
        else:
            row = name
        assert row in M.TABLE, "call site %s (%s) has no row in THE TABLE" % (name, where)
        assert M.TABLE[row][3] & mask[where] == mask[where], "%s is called over the %s fields but not served on all of them" % (name, where)
        if where == "base" and name not in componentwise:
            assert "half_" + name in M.TABLE, "%s runs over Fp2Half (G2) too: no half_%s row" % (name, name)


# ---- the model: contracts, closure, residues -------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,name", FIELD_OPS, ids=["%s-%s" % c for c in FIELD_OPS])
def test_vectors_stay_inside_their_contract_and_the_model_in_its_class(field, name):
    """the reference alone: no OutOfContract on any row of the lists both modules send, every result the residue its
    definition asks for (pyref arithmetic) and inside the documented output class"""
    rows, exp = M.case(field, name, NRAND)
    assert len(rows) == len(exp) >= NRAND + 10


@pytest.mark.parametrize("field", P.FIELD_ORDER)
def test_the_deciding_values_are_placed(field):
    g = M.GEO[field]
    p, R = g.p, g.R
    ops = M.ops_of(field)
    for name in ("mul_r", "mul_r1", "mul", "half_mul_r"):
        if name in ops:
            rows = M.case(field, name, NRAND)[0]
            a_p_b_1 = [p, 1] if M.TABLE[name][2] == M.U_FP else [(p, 0), (1, 0)]
            assert a_p_b_1 in rows                                   # m = R - 1: every multiplier limb 0xffffffff
            assert (p * g.ninv) % R == R - 1
    if "mul_r" in ops:
        assert [2 * p, 2 * p] in M.case(field, "mul_r", NRAND)[0] and g.mul_r(2 * p, 2 * p) < 2 * p
    for name in ("add_r", "add_r2"):
        if name in ops:
            sums = {a + b for a, b in M.case(field, name, NRAND)[0]}
            want = {2 * p - 1, 2 * p, 2 * p + 1, 4 * p - 2}
            if name == "add_r2" and 4 * p - 2 > R:
                want |= {R - 1, R, R + 1}
            assert want <= sums, (field, name)
    assert (field == "BLS12_381_FR") == (4 * p - 2 > R)               # the carry-out case of add_r2 exists there and only there
    diffs = {a - b for a, b in M.case(field, "sub_r", NRAND)[0]}
    assert {0, 1, -1, p, -p, -(2 * p - 1), -2 * p} <= diffs
    if "reduce_2p" in ops:
        assert {2 * p - 1, 2 * p, 2 * p + 1, 4 * p - 1} <= {r[0] for r in M.case(field, "reduce_2p", NRAND)[0]}
        assert [2 * p] in M.case(field, "neg_r", NRAND)[0] and [0] in M.case(field, "neg_r", NRAND)[0]
        assert {0, p, 1, p - 1, p + 1} <= {r[0] for r in M.case(field, "is_zero_mod_p", NRAND)[0]}
    if g.nb:
        bt = [g.beta_times(e[0][1]) for e in M.case(field, "half_mul_r", NRAND)[0]]
        assert max(bt) == 2 * g.nb * p                               # a beta_times operand at its maximum (10p over BLS12-377)
        assert [(0, 0)] in M.case(field, "half_neg_r", NRAND)[0]
        assert max(r[2] for r in M.case(field, "sop2", NRAND)[0]) == 6 * p
    low = (1 << (32 * (g.N - 1))) - 1
    cls = M.edges(g, "2p")
    assert any(v & low == low and v > low for v in cls) and sum(1 for v in cls if bin(v).count("1") == 32 and v % 0xFFFFFFFF == 0) >= g.N - 1


def test_value_level_mutants_break_the_model_on_listed_rows():
    """device-only decisions, mutated in the model: the listed edge rows must notice"""
    # FOLD forced false over BLS12-381: (16 p^2 + m p) / R reaches 2p -- closure fails on deterministic edge rows
    g = M.Geo("BLS12_381_FQ", fold=False)
    rows = M.case("BLS12_381_FQ", "half_sop2_r", NRAND)[0]
    assert rows[0] == [(2 * g.p, 2 * g.p)] * 4
    broken = []
    for i, row in enumerate(rows[:-NRAND]):
        try:
            M.expected("BLS12_381_FQ", "half_sop2_r", [row], g)
        except AssertionError as e:
            assert "leaves its class" in str(e)
            broken.append(i)
    assert len(broken) > 100, len(broken)
    # ... and the unmutated fold is what keeps BLS12-377 unfolded: there FOLD forced TRUE changes nothing (every t < 2p)
    g7 = M.Geo("BLS12_377_FQ", fold=True)
    rows7 = M.case("BLS12_377_FQ", "half_sop2_r", NRAND)
    assert M.expected("BLS12_377_FQ", "half_sop2_r", rows7[0][:512], g7) == rows7[1][:512]
    # beta_times as NEG_BETA (p - x): wrong for every x above p -- the listed row x = 2p - 1 leaves the class <= 2 NEG_BETA p
    for field in M.NEG_BETA:
        g = M.Geo(field, beta_2p=False)
        row = [(2 * g.p - 1, g.p + 1)]
        assert row in M.case(field, "half_beta_times", NRAND)[0]
        with pytest.raises(AssertionError, match="leaves its class"):
            M.expected(field, "half_beta_times", [row], g)


# ---- the model against the header's host forms, on the GPU module's vector files -------------------------------------------------
@pytest.mark.parametrize("field", P.FIELD_ORDER)
def test_host_forms_match_model_on_the_gpu_vectors(field, host_runner, tmp_path):
    g = M.GEO[field]
    names = M.ops_of(field, HOST_UNITS)
    records = []
    for name in names:
        rows, _ = M.case(field, name, NRAND)
        arr = M.rows_to_array(field, name, rows)
        records.append((0, M.FIELD_ID[field], M.TABLE[name][0], arr.shape[0], arr, (arr.shape[0], g.N + 1)))
    for name, got in zip(names, _run_host(host_runner, tmp_path, records)):
        rows, exp = M.case(field, name, NRAND)
        if name in M.HOST_EXACT:
            want = M.expected_to_array(field, name, exp)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, "%s %s: %d lanes differ; first %d: host %s, model %s" % (
                field, name, bad.size, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
        else:   # a product's host form returns the canonical representative of the same residue
            for i, ((res, flag), (hres, hflag)) in enumerate(zip(exp, M.array_to_results(field, name, got))):
                assert hres == res % g.p and hflag == flag, "%s %s row %d %s: host %x, model %x" % (field, name, i, rows[i], hres, res)


def _generator(A):
    G = A.C.dec(O.generator(A.cid))
    assert G is not None and A.C.on_curve(G)
    return G


@pytest.mark.parametrize("curve", P.CURVE_ORDER)
def test_accumulator_model_against_the_group_law(curve, host_runner, tmp_path):
    """edge cases and chains on the model: the right group element (pyref.Curve), ZZ^3 = ZZZ^2, every coordinate below 2p, the
    exact (1, 1, 0, 0) at infinity, P and R zero as 0 AND as p; for the G1 curves the same inputs through the host forms of ec.cuh,
    as group elements"""
    A = M.AccModel(curve)
    cases = M.acc_edge_cases(A, _generator(A))
    seen = set()
    groups = {}
    for kind, acc, other, want, tag in cases:
        A.trace = None
        out = A.apply(kind, acc, other)
        assert A.affine(out) == want and A.consistent(out) and A.closed(out), (curve, kind, tag)
        if want is None:
            assert out == A.infinity(), (curve, kind, tag)
        if kind == "canonical":
            assert all(c < A.g.p for co in out for c in A.F.comps(co))
        if tag in ("equal", "inverse"):
            seen.add((tag,) + tuple(c // A.g.p for v in A.trace for c in A.F.comps(v)))
        groups.setdefault(kind, []).append((acc, other, want))
    for tag in ("equal", "inverse"):   # P and R: every 0-representative
        forms = {s[1:] for s in seen if s[0] == tag}
        assert {f[i] for f in forms for i in range(len(f))} == {0, 1} and len(forms) >= 4, (curve, tag, forms)
    starts, mult, sched, pt = M.acc_chain(A, _generator(A), 8, 64)
    state, cur, hit = list(starts), list(mult), set()
    for kind, ops, ms in sched:
        before = list(state)
        for i in range(len(state)):
            if cur[i] % A.C.r == 0:
                hit.add("from infinity")
            elif ms[i] % A.C.r:
                hit.add("equal" if ms[i] == cur[i] else "inverse" if ms[i] == -cur[i] else "other")
            state[i] = A.apply(kind, state[i], ops[i])
            cur[i] += ms[i]
            assert A.affine(state[i]) == pt(cur[i]) and A.consistent(state[i]) and A.closed(state[i]), (curve, kind, i)
        groups.setdefault(kind, []).extend((b, o, pt(c)) for b, o, c in zip(before, ops, cur))
    assert hit == {"equal", "inverse", "other", "from infinity"}
    if A.ext == 2:
        return   # Fp2Half is device code
    records, kinds = [], sorted(groups)
    for kind in kinds:
        accs = np.array([A.words(c[0]) for c in groups[kind]], dtype=np.uint64).astype(np.uint32)
        arr = accs.reshape(-1)
        if kind != "canonical":
            arr = np.concatenate([arr, np.array([A.other_words(kind, c[1]) for c in groups[kind]], dtype=np.uint64).astype(np.uint32).reshape(-1)])
        records.append((1, A.cid, M.ACC_KIND[kind], len(groups[kind]), arr, accs.shape))
    for kind, got in zip(kinds, _run_host(host_runner, tmp_path, records)):
        for i, (c, w) in enumerate(zip(groups[kind], got)):
            out = A.from_words(w.tolist())
            assert A.affine(out) == c[2] and A.consistent(out) and A.closed(out), (curve, kind, i)


# ---- the table of documented bounds ------------------------------------------------------------------------------------------------
def test_documented_bounds_are_the_comments_own_and_hold_exactly():
    assert len(M.DOCUMENTED) >= 20
    for where, words, fields, derive in M.DOCUMENTED:
        fname, line = where.split(":")
        text = open(os.path.join(CSRC, fname)).read().split("\n")[int(line) - 1]
        assert words in text, "%s no longer says '%s': %s" % (where, words, text.strip())
        for f in fields:
            assert derive(M.GEO[f]), "%s: '%s' does not hold over %s" % (where, words, f)
