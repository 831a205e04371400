"""CPU-side checks of the transcript and of the whole-proof sumcheck entry (no GPU needed): the host
entry ark_hip_transcript_challenge and the 512-bit reduction against the model of tests/transcript_ref.py (hashlib.shake_256
and Python integers) on all three scalar fields; every ARK_HIP_ERR_ARG case of the two new entries before any device is
touched; ark_hip_sumcheck_prove_plan; the names and arities in the header, `_lib.SYMBOLS`, ark-hip-sys and ark_hip.hpp.
The kernels are checked on the GPU by tests/test_gpu_sumcheck_device.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
import pyref
import sumcheck_ref as S
import transcript_ref as T
from test_sumcheck_host import _decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
NAMES = {"ark_hip_transcript_challenge": 5, "ark_hip_sumcheck_prove_device": 15, "ark_hip_sumcheck_prove_plan": 6}
HOOKS = {"ark_hip_test_transcript_reduce": 4, "ark_hip_test_transcript_challenge_device": 5}
TAIL_MAX = 14
ERR_ARG, ERR_NO_DEVICE = -1, -5
SEED = bytes(range(7, 39))


def reduce_vectors(p):
    """the 512-bit values the reduction is checked at, as 64 little-endian bytes"""
    rng = np.random.default_rng(512)
    top = (1 << 512) // p * p
    vals = [0, p - 1, p, p + 1, (1 << 256) - 1, 1 << 256, top, (1 << 512) - 1]
    vals += [int.from_bytes(rng.bytes(64), "little") for _ in range(200)]
    assert vals[6] % p == 0 and vals[6] < 1 << 512 <= vals[6] + p
    return [v.to_bytes(64, "little") for v in vals]


def challenge_cases(p, seed=2024):
    """(elements per call) of a transcript session: counts 0, 1, 3, 5 (one and two rate blocks), 4 (exactly 164 bytes), then
    a chain of 20 calls of mixed counts"""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 3, 5, 4] + [int(c) for c in rng.integers(0, 6, size=20)]
    return [[(0, 1, p - 1, int.from_bytes(rng.bytes(40), "little") % p)[min(int(rng.integers(0, 8)), 3)] for _ in range(k)] for k in counts]


@pytest.mark.parametrize("fname", FIELDS)
def test_host_challenge_is_the_model(fname):
    p = pyref.MODULI[fname][0]
    t, m = A.Transcript(fname, SEED), T.Transcript(p, SEED)
    assert t.state == SEED
    for i, els in enumerate(challenge_cases(p)):
        got = t.challenge(S.encode(els, p) if els else None)
        assert S.decode(got.reshape(1, 4), p) == [m.challenge(els)], (i, len(els))
        assert t.state == m.state, (i, len(els))
    # the message lengths named above: 36 bytes (no element), 164 bytes (4 elements: one block and 28 bytes), 196 (two blocks)
    assert [36 + 32 * k for k in (0, 4, 5)] == [36, 164, 196]
    # an empty list and None are the same call
    a, b = A.Transcript(fname, SEED), A.Transcript(fname, SEED)
    assert np.array_equal(a.challenge(None), b.challenge(np.zeros((0, 4), dtype=np.uint64))) and a.state == b.state


@pytest.mark.parametrize("fname", FIELDS)
def test_host_reduction_is_the_model(fname):
    p, fid = pyref.MODULI[fname][0], A.curves.field_id(fname)
    L = _lib.test_lib()
    out = np.zeros(4, dtype=np.uint64)
    for b in reduce_vectors(p):
        assert L.ark_hip_test_transcript_reduce(fid, b, 0, out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, T.reduce512(b, p)), int.from_bytes(b, "little")


def test_the_model_verifier_accepts_its_prover_and_rejects_another_point():
    p = pyref.MODULI["BLS12_381_FR"][0]
    rng = np.random.default_rng(5)
    tables = [[int.from_bytes(rng.bytes(40), "little") % p for _ in range(16)] for _ in range(3)]
    terms = [(1, [0, 1, 2]), (p - 1, [2])]
    tr = T.Transcript(p, SEED)
    rounds, point, finals, value = T.prove(tables, terms, tr, p)
    claim = (rounds[0][0] + rounds[0][1]) % p
    v = T.Transcript(p, SEED)
    assert T.verify(claim, rounds, point, finals, terms, v, p) and v.state == tr.state
    assert not T.verify(claim, rounds, point[:-1] + [(point[-1] + 1) % p], finals, terms, T.Transcript(p, SEED), p)
    assert not T.verify(claim, rounds, point, finals, terms, T.Transcript(p, bytes(32)), p)


def test_the_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    L, TL = _lib.lib(), _lib.test_lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity and name not in hooks, name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name
    for name, arity in HOOKS.items():
        assert hooks.get(name) == arity and name not in public, name
        assert name in _lib.TEST_SYMBOLS and len(_lib.TEST_SYMBOLS[name][1]) == arity, name
        assert hasattr(TL, name) and not hasattr(L, name), name
    assert re.search(r"#define\s+ARK_HIP_SUMCHECK_TAIL_MAX_VARS\s+%d\b" % TAIL_MAX, hdr)
    doc = hdr[hdr.index("int ark_hip_transcript_challenge") - 1200:hdr.index("int ark_hip_transcript_challenge")]
    assert "NOT checked" in doc and "SHAKE256" in doc


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
    for name in ("ark_hip_transcript_challenge(", "ark_hip_sumcheck_prove_device(", "ark_hip_sumcheck_prove_plan("):
        assert "sys::" + name in rs and name in hpp, name
    assert re.search(r"\bfn prove_device\b", rs) and re.search(r"\bstruct Transcript\b", rs)
    assert re.search(r"\bprove_device\(", hpp[hpp.index("class ListOfProducts"):]) and re.search(r"\bclass Transcript\b", hpp)
    assert A.Transcript is not None and callable(A.sumcheck_prove_plan)
    for cls in (A.ListOfProducts, A.GrandProduct, A.FractionalSum):
        assert callable(getattr(cls, "prove_device")), cls


def _plan(nv, nt=3, tail=-1):
    w, l, t = C.c_size_t(1 << 60), C.c_int(-7), C.c_int(-7)
    rc = _lib.lib().ark_hip_sumcheck_prove_plan(nv, nt, tail, C.byref(w), C.byref(l), C.byref(t))
    assert rc == 0, (nv, nt, tail, rc)
    return w.value, l.value, t.value


def test_prove_plan():
    L = _lib.lib()
    default = _plan(30)[2]
    assert 0 <= default <= TAIL_MAX
    for nv in range(1, 31):
        for nt in (1, 3, 8):
            w, launches, tf = _plan(nv, nt)
            # two alternating sets of bound tables: halves and quarters, as ListOfProducts.round sizes them
            assert w == nt * ((1 << max(nv - 1, 0)) + (1 << max(nv - 2, 0))), (nv, nt)
            assert tf == min(default, nv) and A.sumcheck_prove_plan(nv, nt) == (w, launches, tf)
        for tail in range(1, TAIL_MAX + 1):
            w, launches, tf = _plan(nv, 3, tail)
            assert tf == min(tail, nv), "tail_from is clamped to num_vars"
            # rounds above the tail: a round launch, a fold launch where the plan has two stages, a challenge launch; then the tail
            above = sum(A.sumcheck_plan(nv - i, 3, 3, False)[2] + 1 for i in range(nv - tf))
            assert launches == above + 1, (nv, tail)
            if nv <= tail:
                assert launches == 1, "at the seam the launches drop to the tail's one"
            else:
                assert launches >= 3
        w, launches, tf = _plan(nv, 3, 0)
        assert tf == 0 and launches == sum(A.sumcheck_plan(nv - i, 3, 3, False)[2] + 1 for i in range(nv)) + 2   # the m = 0 round, the gather
    assert _plan(TAIL_MAX + 1, 3, TAIL_MAX)[1] == A.sumcheck_plan(TAIL_MAX + 1, 3, 3, False)[2] + 2
    w, l, t = C.c_size_t(), C.c_int(), C.c_int()
    ok = (C.byref(w), C.byref(l), C.byref(t))
    assert L.ark_hip_sumcheck_prove_plan(0, 3, -1, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(59, 3, -1, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 0, -1, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 9, -1, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 3, -2, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 3, TAIL_MAX + 1, *ok) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 3, -1, None, ok[1], ok[2]) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 3, -1, ok[0], None, ok[2]) == ERR_ARG
    assert L.ark_hip_sumcheck_prove_plan(10, 3, -1, ok[0], ok[1], None) == ERR_ARG


def test_transcript_argument_errors():
    L = _lib.lib()
    st = (C.c_uint8 * 32)()
    el = (C.c_uint64 * 8)()
    out = (C.c_uint64 * 4)()
    stp, elp, outp = C.cast(st, C.c_void_p), C.cast(el, C.c_void_p), C.cast(out, C.c_void_p)
    assert L.ark_hip_transcript_challenge(3, stp, elp, 2, outp) == 0
    assert L.ark_hip_transcript_challenge(3, stp, None, 0, outp) == 0
    assert L.ark_hip_transcript_challenge(99, stp, elp, 2, outp) == ERR_ARG
    assert L.ark_hip_transcript_challenge(0, stp, elp, 2, outp) == ERR_ARG      # a base field is not served
    assert L.ark_hip_transcript_challenge(3, None, elp, 2, outp) == ERR_ARG
    assert L.ark_hip_transcript_challenge(3, stp, elp, 2, None) == ERR_ARG
    assert L.ark_hip_transcript_challenge(3, stp, None, 1, outp) == ERR_ARG
    with pytest.raises(ValueError):
        A.Transcript("BLS12_381_FR", b"short")


class Call:
    """one well-formed call of the whole-proof entry on pointers that are never dereferenced; `but` replaces arguments"""
    BASE = 1 << 32

    def __init__(self, nv=4, ntables=3, lens=(2, 3), tabs=(0, 1, 0, 1, 2)):
        self.nv, self.nt, self.lens, self.tabs = nv, ntables, list(lens), list(tabs)
        step = 32 << nv
        self.src = [self.BASE + k * step for k in range(ntables)]
        self.work = self.BASE + ntables * step
        self.work_bytes = 32 * _plan(nv, ntables)[0]
        self.el = (C.c_uint64 * (4 * 64))()
        self.st = (C.c_uint8 * 32)()

    def run(self, field=3, **but):
        host = C.cast(self.el, C.c_void_p)
        a = dict(d_tables=(C.c_void_p * len(self.src))(*self.src), ntables=self.nt, num_vars=self.nv,
                 term_len=(C.c_uint * len(self.lens))(*self.lens), term_tables=(C.c_uint * len(self.tabs))(*self.tabs), coeffs=host,
                 nterms=len(self.lens), state=C.cast(self.st, C.c_void_p), tail_vars=-1, d_work=self.work, out_rounds=host,
                 out_point=host, out_finals=host, out_value=host)
        a.update(but)
        return _lib.lib().ark_hip_sumcheck_prove_device(field, a["d_tables"], a["ntables"], a["num_vars"], a["term_len"], a["term_tables"],
                                                        a["coeffs"], a["nterms"], a["state"], a["tail_vars"], a["d_work"], a["out_rounds"],
                                                        a["out_point"], a["out_finals"], a["out_value"])


def test_prove_argument_errors_come_before_any_device_use():
    no_device = _lib.lib().ark_hip_device_count() == 0
    c = Call()
    if no_device:                                    # the well-formed call: a loud refusal, no CPU fallback
        assert c.run() == ERR_NO_DEVICE
        assert Call(nv=1).run() == ERR_NO_DEVICE
        for tail in (0, 1, TAIL_MAX):
            assert c.run(tail_vars=tail) == ERR_NO_DEVICE
        assert c.run(d_tables=(C.c_void_p * 3)(c.src[0], c.src[0], c.src[2])) == ERR_NO_DEVICE   # the same table twice is allowed
    # every argument error of the round entry
    assert c.run(field=99) == ERR_ARG
    assert c.run(field=0) == ERR_ARG
    for name in ("d_tables", "term_len", "term_tables", "coeffs"):
        assert c.run(**{name: None}) == ERR_ARG, name
    assert c.run(d_tables=(C.c_void_p * 3)(c.src[0], None, c.src[2])) == ERR_ARG
    for bad in (0, 9):
        assert c.run(ntables=bad) == ERR_ARG, ("ntables", bad)
        assert c.run(nterms=bad) == ERR_ARG, ("nterms", bad)
    assert c.run(term_len=(C.c_uint * 2)(0, 3)) == ERR_ARG
    assert c.run(term_len=(C.c_uint * 2)(2, 5)) == ERR_ARG
    assert c.run(term_tables=(C.c_uint * 5)(0, 1, 0, 1, 3)) == ERR_ARG
    assert c.run(term_tables=(C.c_uint * 5)(0, 1, 0, 1, 1 << 31)) == ERR_ARG
    for bad in (0, 59, 64):
        assert c.run(num_vars=bad) == ERR_ARG, ("num_vars", bad)
    # ... and this entry's own
    for name in ("state", "out_rounds", "out_point", "out_finals", "out_value", "d_work"):
        assert c.run(**{name: None}) == ERR_ARG, name
    for bad in (-2, TAIL_MAX + 1, 1 << 20):
        assert c.run(tail_vars=bad) == ERR_ARG, ("tail_vars", bad)
    # d_work may not overlap an input table: its first and its last element
    n_in = 32 << c.nv
    assert c.run(d_work=c.src[0]) == ERR_ARG
    assert c.run(d_work=c.src[2] + n_in - 32) == ERR_ARG
    assert c.run(d_work=c.src[0] - c.work_bytes + 32) == ERR_ARG
    if no_device:                                    # touching is not overlapping
        assert c.run(d_work=c.src[0] - c.work_bytes) == ERR_NO_DEVICE
