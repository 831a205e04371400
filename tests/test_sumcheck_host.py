"""CPU-side checks of the sumcheck round (no GPU needed): the two entries are public C ABI with the same arity in the header,
`_lib.SYMBOLS`, ark-hip-sys, ark_hip.hpp and the Rust mirror; the plan answers without a device and is monotone; every
argument error comes before any device is touched; and the big-integer model of tests/sumcheck_ref.py is consistent with
itself: its verifier accepts the honest prover, rejects a changed evaluation, and its periodic tables equal walked ones.
The kernels are checked on the GPU by tests/test_gpu_sumcheck.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import mle_ref
import pyref
import sumcheck_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_sumcheck_round_device": 11, "ark_hip_sumcheck_plan": 7}
LIMITS = {"ARK_HIP_SUMCHECK_MAX_TABLES": 8, "ARK_HIP_SUMCHECK_MAX_TERMS": 8, "ARK_HIP_SUMCHECK_MAX_DEGREE": 4}
ERR_ARG, ERR_NO_DEVICE = -1, -5
FR = 3                                               # BLS12_381_FR
P = pyref.MODULI["BLS12_381_FR"][0]


def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    L = _lib.lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity, name
        assert name not in hooks
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name
    for name, value in LIMITS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    doc = hdr[hdr.index("#define ARK_HIP_SUMCHECK_MAX_TABLES"):hdr.index("int ark_hip_sumcheck_round_device")]
    assert "NO in-place" in doc and "ARK_HIP_ERR_ARG" in doc


def test_rust_and_cpp_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
    rs = open(os.path.join(ROOT, "rust", "ark-hip", "src", "sumcheck.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    assert "sys::ark_hip_sumcheck_round_device(" in rs and "ark_hip_sumcheck_round_device(" in hpp
    assert "pub mod sumcheck;" in open(os.path.join(ROOT, "rust", "ark-hip", "src", "lib.rs")).read()
    for method in ("add_product", "round", "prove"):
        assert re.search(r"\bfn %s\b" % method, rs), method
        assert re.search(r"\b%s\(" % method, hpp[hpp.index("class ListOfProducts"):]), method
    import algebra_amd as A
    assert A.ListOfProducts is not None and callable(A.sumcheck_plan)


def _plan(num_vars, ntables=2, degree=2, fused=0):
    b, ppl, st = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    rc = _lib.lib().ark_hip_sumcheck_plan(num_vars, ntables, degree, fused, C.byref(b), C.byref(ppl), C.byref(st))
    assert rc == 0, (num_vars, ntables, degree, fused, rc)
    return b.value, ppl.value, st.value


def test_plan_answers_without_a_device_and_is_monotone():
    L = _lib.lib()
    for fused in (0, 1):
        prev = (0, 0, 0)
        for nv in range(1, 59):
            b, ppl, st = _plan(nv, fused=fused)
            m = nv - fused
            npairs = 1 << (m - 1) if m >= 1 else 1
            assert b >= 1 and ppl >= 1 and st in (1, 2) and st == (2 if b > 1 else 1), (nv, fused)
            if ppl < 0x7fffffff:                     # the int saturates there, from 2^49 pairs on
                assert b * 256 * ppl >= npairs and b * 256 * (ppl - 1) < npairs, (nv, fused, "the lanes cover the pairs, none idle a whole step")
            else:
                assert npairs >= b * 256 * 0x7fffffff
            assert b >= prev[0] and ppl >= prev[1] and st >= prev[2], (nv, fused, "monotone in size")
            prev = (b, ppl, st)
            for nt, deg in ((1, 1), (8, 4), (3, 3)):
                assert _plan(nv, nt, deg, fused) == (b, ppl, st), "tables and degree select the kernel, not the geometry"
        assert _plan(1, fused=fused)[2] == 1
        two = min(nv for nv in range(1, 59) if _plan(nv, fused=fused)[2] == 2)
        many = min(nv for nv in range(1, 59) if _plan(nv, fused=fused)[1] > 1)
        assert two <= 24 and many <= 24 and two < many, (two, many)
        assert _plan(two - 1, fused=fused)[2] == 1 and _plan(many - 1, fused=fused)[1] == 1
    assert _plan(12, fused=1) == _plan(11, fused=0)       # a fused round sums tables of half the length
    b, ppl, st = C.c_int(), C.c_int(), C.c_int()
    ok = (C.byref(b), C.byref(ppl), C.byref(st))
    assert L.ark_hip_sumcheck_plan(0, 2, 2, 0, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(0, 2, 2, 1, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(64, 2, 2, 0, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 0, 2, 0, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 9, 2, 0, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 2, 0, 0, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 2, 5, 0, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 2, 2, 0, None, ok[1], ok[2]) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 2, 2, 0, ok[0], None, ok[2]) == ERR_ARG
    assert L.ark_hip_sumcheck_plan(10, 2, 2, 0, ok[0], ok[1], None) == ERR_ARG


class Call:
    """one well-formed call of the round on pointers that are never dereferenced; `but` replaces arguments"""
    BASE = 1 << 32

    def __init__(self, nv=4, ntables=3, lens=(2, 3), tabs=(0, 1, 0, 1, 2), fused=False):
        self.nv, self.nt, self.lens, self.tabs, self.fused = nv, ntables, list(lens), list(tabs), fused
        step = 32 << nv                                   # a table's bytes: each begins where the one before ends
        self.src = [self.BASE + k * step for k in range(ntables)]
        self.dst = [self.BASE + (ntables + k) * step for k in range(ntables)]
        self.el = (C.c_uint64 * (4 * 16))()

    def run(self, field=FR, **but):
        host = C.cast(self.el, C.c_void_p)
        a = dict(d_tables=(C.c_void_p * len(self.src))(*self.src), ntables=self.nt, num_vars=self.nv,
                 term_len=(C.c_uint * len(self.lens))(*self.lens), term_tables=(C.c_uint * len(self.tabs))(*self.tabs), coeffs=host,
                 nterms=len(self.lens), r_prev=host if self.fused else None,
                 d_out_tables=(C.c_void_p * len(self.dst))(*self.dst) if self.fused else None, out_evals=host)
        a.update(but)
        return _lib.lib().ark_hip_sumcheck_round_device(field, a["d_tables"], a["ntables"], a["num_vars"], a["term_len"], a["term_tables"],
                                                        a["coeffs"], a["nterms"], a["r_prev"], a["d_out_tables"], a["out_evals"])


def test_argument_errors_come_before_any_device_use():
    L = _lib.lib()
    no_device = L.ark_hip_device_count() == 0
    for fused in (False, True):
        c = Call(fused=fused)
        if no_device:                                # the well-formed call: a loud refusal, no CPU fallback
            assert c.run() == ERR_NO_DEVICE
            assert Call(nv=1, fused=fused).run() == ERR_NO_DEVICE
            assert Call(nv=58, ntables=1, lens=(1,), tabs=(0,), fused=fused).run() == ERR_NO_DEVICE
        assert c.run(field=99) == ERR_ARG            # an unknown field
        assert c.run(field=0) == ERR_ARG             # a base field is not served
        for name in ("d_tables", "term_len", "term_tables", "coeffs", "out_evals"):
            assert c.run(**{name: None}) == ERR_ARG, name
        assert c.run(d_tables=(C.c_void_p * 3)(c.src[0], None, c.src[2])) == ERR_ARG
        for bad in (0, 9):
            assert c.run(ntables=bad) == ERR_ARG, ("ntables", bad)
            assert c.run(nterms=bad) == ERR_ARG, ("nterms", bad)
        assert c.run(term_len=(C.c_uint * 2)(0, 3)) == ERR_ARG
        assert c.run(term_len=(C.c_uint * 2)(2, 5)) == ERR_ARG
        assert c.run(term_tables=(C.c_uint * 5)(0, 1, 0, 1, 3)) == ERR_ARG      # a table index >= ntables
        assert c.run(term_tables=(C.c_uint * 5)(0, 1, 0, 1, 1 << 31)) == ERR_ARG
        assert c.run(num_vars=64) == ERR_ARG
        assert c.run(num_vars=59) == ERR_ARG         # 2^59 elements of 32 bytes: a size_t cannot count them
        assert c.run(num_vars=0) == ERR_ARG          # nothing to sum without r_prev, nothing to bind with it
    # the same input table twice is allowed
    c = Call()
    if no_device:
        assert c.run(d_tables=(C.c_void_p * 3)(c.src[0], c.src[0], c.src[2])) == ERR_NO_DEVICE
    # r_prev: output tables are needed, and none may overlap an input table or another output table
    c = Call(fused=True)
    n_in, n_out = 32 << c.nv, 16 << c.nv
    assert c.run(d_out_tables=None) == ERR_ARG
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], None, c.dst[2])) == ERR_ARG
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.src[0], c.dst[1], c.dst[2])) == ERR_ARG            # no in-place form
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], c.dst[1], c.src[0])) == ERR_ARG            # ... of another table either
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], c.src[2] + n_in - 32, c.dst[2])) == ERR_ARG   # the input's last element
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], c.src[2] - n_out + 32, c.dst[2])) == ERR_ARG  # the output's last element
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], c.dst[0], c.dst[2])) == ERR_ARG            # two outputs in one place
    assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], c.dst[1], c.dst[1] + n_out - 32)) == ERR_ARG
    if no_device:                                    # touching is not overlapping
        assert c.run(d_out_tables=(C.c_void_p * 3)(c.dst[0], c.dst[0] + n_out, c.dst[0] + 2 * n_out)) == ERR_NO_DEVICE


# ---- the model ---------------------------------------------------------------------------------------------------
def _shape(rng, nv):
    ntables = int(rng.integers(1, 5))
    tables = [[int.from_bytes(rng.bytes(40), "little") % P for _ in range(1 << nv)] for _ in range(ntables)]
    terms = []
    for _ in range(int(rng.integers(1, 4))):
        ix = [int(v) for v in rng.integers(0, ntables, size=int(rng.integers(1, 5)))]
        terms.append(((0, 1, P - 1, int.from_bytes(rng.bytes(40), "little") % P)[int(rng.integers(0, 4))], ix))
    return tables, terms


def _claim(tables, terms):
    return sum(S.pair_values([t[i] for t in tables], [t[i] for t in tables], terms, P)[0] for i in range(len(tables[0]))) % P


def test_round_sums_are_the_definition():
    # g(0) + g(1) is the sum over the whole cube; a degree-1 sum is the sum of the even and of the odd entries
    rng = np.random.default_rng(3)
    t = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(16)]
    assert S.round_sums([t], [(1, [0])], P) == [sum(t[0::2]) % P, sum(t[1::2]) % P]
    u = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(16)]
    g = S.round_sums([t, u], [(5, [0, 1, 0])], P)
    assert len(g) == 4 and (g[0] + g[1]) % P == 5 * sum(a * a * b for a, b in zip(t, u)) % P
    assert g[2] == 5 * sum((2 * t[2 * b + 1] - t[2 * b]) ** 2 * (2 * u[2 * b + 1] - u[2 * b]) for b in range(8)) % P
    assert S.interpolate([7, 12, 21], 5, P) == S.interpolate([7, 12, 21, 34], 5, P) == 72          # 7 + 3 x + 2 x^2 at 5
    assert S.interpolate([7, 12, 21], P - 1, P) == 6 and S.interpolate([4, 9], 10, P) == 54
    assert S.final_round([[3], [4]], [(2, [0, 1]), (1, [1])], P) == [2 * 12 + 4, 0, 0]


@pytest.mark.parametrize("nv", range(1, 7))
def test_the_verifier_accepts_the_honest_prover_and_rejects_a_changed_evaluation(nv):
    rng = np.random.default_rng(100 + nv)
    _, challenge = S.hash_challenge(P)
    for _ in range(4):
        tables, terms = _shape(rng, nv)
        rounds, point, finals, final_value = S.prove(tables, terms, challenge, P)
        claim = _claim(tables, terms)
        assert len(rounds) == nv and len(point) == nv
        assert finals == [mle_ref.evaluate(t, point, P) for t in tables]
        assert final_value == S.pair_values(finals, finals, terms, P)[0]
        assert S.verify_tables(claim, rounds, point, tables, terms, P)
        assert S.verify(claim, rounds, point, finals, terms, P)
        assert not S.verify_tables((claim + 1) % P, rounds, point, tables, terms, P)
        for i in range(nv):                          # one evaluation of one round changed, the point kept
            for t in range(len(rounds[i])):
                bad = [list(g) for g in rounds]
                bad[i][t] = (bad[i][t] + 1) % P
                assert not S.verify_tables(claim, bad, point, tables, terms, P), (i, t)


@pytest.mark.parametrize("nv", [1, 2, 5, 9, 10])
def test_periodic_tables_equal_walked_ones(nv):
    rng = np.random.default_rng(200 + nv)
    _, challenge = S.hash_challenge(P, b"periodic")
    tables = []
    for k in range(3):
        s = min(nv, (0, 3, 4)[k])
        base = [int.from_bytes(rng.bytes(40), "little") % P for _ in range(1 << s)]
        cells = {int(i): (0, P - 1, 12345)[q % 3] for q, i in enumerate(rng.integers(0, 1 << nv, size=5))}
        cells[0], cells[(1 << nv) - 1] = 1, 2
        tables.append(S.Periodic(nv, base, cells if k else None))
    walked = [t.expand() for t in tables]
    assert all(len(w) == 1 << nv for w in walked)
    terms = [(1, [0, 1]), (P - 1, [1, 1, 2]), (77, [2])]
    assert S.round_sums(tables, terms, P) == S.round_sums(walked, terms, P)
    mixed = [tables[0], walked[1], tables[2]]
    assert S.round_sums(mixed, terms, P) == S.round_sums(walked, terms, P)
    got, want = S.prove(tables, terms, challenge, P), S.prove(walked, terms, challenge, P)
    assert got == want
    assert S.verify_tables(_claim(walked, terms), got[0], got[1], walked, terms, P)
    r = 0xABCDEF
    for a, b in zip(S.bind(tables, r, P), S.bind(walked, r, P)):
        assert a.expand() == b
