"""CPU-side checks of the gate expressions on device vectors (no GPU needed): the big-integer model of tests/gate_ref.py
against an independently written naive evaluation, the plan's invariants, every argument error of
ark_hip_fr_sum_of_products_device reported before any device is looked for, and the two entries as part of the public C ABI
(header, exports, Python / Rust / C++ mirrors).  The kernel itself is checked on the GPU by tests/test_gpu_gate.py."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import algebra_amd as A
import gate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_fr_sum_of_products_device": 11, "ark_hip_fr_sum_of_products_plan": 3}
ERR_ARG, ERR_NO_DEVICE = -1, -5
FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
MAX_COLUMNS, MAX_TERMS, MAX_DEGREE = 16, 16, 8
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_the_model_against_a_naive_evaluation(fname):
    f = R.Field(fname)
    rng = np.random.default_rng(25)
    for n, ncols, nterms in ((1, 1, 1), (2, 2, 3), (3, 1, 2), (5, 3, 4), (7, 16, 16), (12, 4, 5)):
        cols = [R.planted(f, n, 3 + 5 * k + n) for k in range(ncols)]
        rots = [0, 1, -1, n - 1, n, -n, n + 1, 4, 8, -3 * n - 2, 5 * n + 1, I64_MIN, I64_MAX]
        terms = []
        for j in range(nterms):
            ln = int(rng.integers(1, MAX_DEGREE, endpoint=True))
            factors = [(int(rng.integers(0, ncols)), rots[int(rng.integers(0, len(rots)))]) for _ in range(ln)]
            if j == 0:
                factors = [factors[0]] * ln                                   # one (column, rotation) repeated: a power
            coeff = (None, f.one, 0, f.enc(-1), R.rand_elems(f, 1, 40 + j)[0])[j % 5]
            terms.append((coeff, factors))
        for c0 in (None, R.rand_elems(f, 1, 77)[0]):
            assert R.sum_of_products(f, cols, n, terms, c0) == R.naive(f, cols, n, terms, c0), (n, ncols, nterms)
    assert R.sum_of_products(f, [[]], 0, [(None, [(0, 5)])]) == []


def test_the_model_on_a_hand_computed_case():
    f = R.Field("BLS12_381_FR")
    a, b = [f.enc(v) for v in (2, 3, 5, 7)], [f.enc(v) for v in (11, 13, 17, 19)]
    # 3 a[i] b[i+1] + a[i-1]^2 + 1
    got = R.sum_of_products(f, [a, b], 4, [(f.enc(3), [(0, 0), (1, 1)]), (None, [(0, -1), (0, 3)])], f.enc(1))
    assert got == [f.enc(v) for v in (3 * 2 * 13 + 49 + 1, 3 * 3 * 17 + 4 + 1, 3 * 5 * 19 + 9 + 1, 3 * 7 * 11 + 25 + 1)]
    assert R.sum_of_products(f, [a], 4, [(None, [(0, I64_MIN)])]) == a                # 2^63 is a multiple of 4
    assert R.sum_of_products(f, [a], 4, [(None, [(0, I64_MAX)])]) == a[3:] + a[:3]


# ---- the plan -----------------------------------------------------------------------------------------------------------
def _plan(n):
    b, r = C.c_int(), C.c_int()
    assert _lib.lib().ark_hip_fr_sum_of_products_plan(n, C.byref(b), C.byref(r)) == 0
    assert A.sum_of_products_plan(n) == (b.value, r.value)
    return b.value, r.value


def test_the_plan():
    assert _plan(0) == (0, 0)                                                 # n = 0 is defined: nothing is launched
    cap = _plan(1 << 40)[0]                                                   # the grid's cap
    assert cap >= 256 and _plan(1 << 41)[0] == cap
    seam = cap * 256
    for n in (1, 2, 255, 256, 257, 1000, 65536, seam - 1, seam, seam + 1, 2 * seam, 2 * seam + 1, 3 * seam, 1 << 30, 1 << 40):
        blocks, rpl = _plan(n)
        assert 1 <= blocks <= cap and blocks * 256 * rpl >= n, n
        assert blocks * 256 * (rpl - 1) < n, n                                # and no lane walks a row too many
        assert blocks == min(-(-n // 256), cap), n
        assert (rpl == 1) == (n <= seam), n
    assert _plan(seam)[1] == 1 and _plan(seam + 1)[1] == 2 and _plan(2 * seam)[1] == 2 and _plan(2 * seam + 1)[1] == 3
    assert _plan(1 << 58) == (cap, 0x7fffffff)                                # the count saturates
    L = _lib.lib()
    b = C.c_int()
    assert L.ark_hip_fr_sum_of_products_plan(5, None, C.byref(b)) == ERR_ARG
    assert L.ark_hip_fr_sum_of_products_plan(5, C.byref(b), None) == ERR_ARG


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_is_looked_for():
    """every violation of the contract is ARK_HIP_ERR_ARG with or without a GPU; without a GPU a well-formed call is
    ARK_HIP_ERR_NO_DEVICE.  The device pointers are fakes: no well-formed call is made when a GPU is present."""
    L = _lib.lib()
    entry = L.ark_hip_fr_sum_of_products_device
    F = 3                                            # BLS12_381_FR
    n = 1000
    BASE = 1 << 30
    ptrs = [BASE + k * (1 << 20) for k in range(MAX_COLUMNS + 1)]            # far apart: n * 32 bytes never overlap
    OUT = BASE + (1 << 28)
    one = np.zeros((MAX_TERMS + 1, 4), dtype=np.uint64)

    def call(field=F, cols=ptrs[:3], ncolumns=None, n=n, lens=(2, 1), tcols=(0, 1, 2), rots=(0, 0, 0), coeffs=one, nterms=None,
             c0=None, out=OUT, null=()):
        arr = (C.c_void_p * max(len(cols), 1))(*cols)
        ln = (C.c_uint * max(len(lens), 1))(*lens)
        tc = (C.c_uint * max(len(tcols), 1))(*tcols)
        rt = None if rots is None else (C.c_int64 * max(len(rots), 1))(*rots)
        return entry(field, None if "cols" in null else arr, len(cols) if ncolumns is None else ncolumns, n,
                     None if "lens" in null else ln, None if "tcols" in null else tc, rt,
                     None if "coeffs" in null else coeffs.ctypes.data_as(C.c_void_p), len(lens) if nterms is None else nterms,
                     None if c0 is None else c0.ctypes.data_as(C.c_void_p), None if out is None else C.c_void_p(out))

    ok = ERR_NO_DEVICE if L.ark_hip_device_count() == 0 else None            # None: the call would run -- not made

    def well_formed(**kw):
        if ok is not None:
            assert call(**kw) == ok, kw

    well_formed()
    well_formed(rots=None)
    well_formed(c0=one[0])
    assert call(field=99) == ERR_ARG and call(field=-1) == ERR_ARG            # unknown
    assert call(field=0) == ERR_ARG and call(field=2) == ERR_ARG              # base fields are not served
    for which in ("cols", "lens", "tcols", "coeffs"):
        assert call(null=(which,)) == ERR_ARG, which
    assert call(out=None) == ERR_ARG
    assert call(cols=[ptrs[0], 0, ptrs[2]]) == ERR_ARG                        # a null column with n > 0 ...
    assert call(cols=[ptrs[0], ptrs[1], 0]) == ERR_ARG
    if ok is not None:
        assert call(cols=[0, 0, 0], n=0) == ok                                # ... and with n = 0, where nothing is read
    assert call(ncolumns=0) == ERR_ARG and call(cols=ptrs[:MAX_COLUMNS + 1], ncolumns=MAX_COLUMNS + 1) == ERR_ARG
    well_formed(cols=ptrs[:MAX_COLUMNS])
    assert call(nterms=0) == ERR_ARG
    assert call(lens=[1] * (MAX_TERMS + 1), tcols=[0] * (MAX_TERMS + 1), rots=None) == ERR_ARG
    well_formed(lens=[1] * MAX_TERMS, tcols=[0] * MAX_TERMS, rots=None)
    assert call(lens=(0, 1), tcols=(0,), rots=None) == ERR_ARG and call(lens=(2, 0), tcols=(0, 1), rots=None) == ERR_ARG
    assert call(lens=(MAX_DEGREE + 1,), tcols=[0] * (MAX_DEGREE + 1), rots=None) == ERR_ARG
    well_formed(lens=(MAX_DEGREE,), tcols=[0] * MAX_DEGREE, rots=None)
    assert call(tcols=(0, 1, 3)) == ERR_ARG and call(tcols=(3, 1, 2)) == ERR_ARG and call(tcols=(0, 0xFFFFFFFF, 2)) == ERR_ARG
    assert call(n=(1 << 58) + 1) == ERR_ARG and call(n=1 << 63) == ERR_ARG
    assert call(n=0, field=99) == ERR_ARG and call(n=0, tcols=(0, 1, 3)) == ERR_ARG   # n = 0 still validates
    # aliasing: d_out may be a column read at rotation 0 mod n only
    well_formed(out=ptrs[1])
    well_formed(out=ptrs[1], rots=(5, n, 7))                                  # column 1 at rotation n: 0 after reduction
    well_formed(out=ptrs[1], rots=(5, -n, 7))
    well_formed(out=ptrs[1], rots=(5, I64_MIN + (1 << 63) % n, 7))
    assert call(out=ptrs[1], rots=(0, 1, 0)) == ERR_ARG
    assert call(out=ptrs[1], rots=(0, -1, 0)) == ERR_ARG and call(out=ptrs[1], rots=(0, n + 1, 0)) == ERR_ARG
    assert call(out=ptrs[1], rots=(0, I64_MIN, 0)) == ERR_ARG                  # 2^63 is not a multiple of 1000
    assert call(out=ptrs[1], rots=(0, I64_MAX, 0)) == ERR_ARG
    assert call(out=ptrs[0], lens=(2, 1), tcols=(0, 1, 0), rots=(0, 0, 4)) == ERR_ARG   # the second read of column 0 is rotated
    well_formed(out=ptrs[0], lens=(2, 1), tcols=(0, 1, 0), rots=(0, 3, 0))
    # the same pointer as two columns: the rotated one refuses, whichever index carries it
    assert call(cols=[ptrs[0], ptrs[0], ptrs[2]], out=ptrs[0], rots=(0, 2, 0)) == ERR_ARG
    assert call(cols=[ptrs[0], ptrs[0], ptrs[2]], out=ptrs[0], rots=(2, 0, 0)) == ERR_ARG
    well_formed(cols=[ptrs[0], ptrs[0], ptrs[2]], out=ptrs[0])
    # partial overlaps, from below and from above, by one element and by all but one; touching ranges are fine
    for k in range(3):
        for d in (32, -32, 32 * (n - 1), -32 * (n - 1), 16, -8):
            assert call(out=ptrs[k] + d) == ERR_ARG, (k, d)
            assert call(out=ptrs[k] + d, rots=None) == ERR_ARG, (k, d)
        well_formed(out=ptrs[k] + 32 * n)
        well_formed(out=ptrs[k] - 32 * n)
    assert call(cols=[ptrs[0], ptrs[1], ptrs[2]], out=ptrs[2] + 32, lens=(1,), tcols=(0,), rots=None) == ERR_ARG   # an unread column counts


# ---- the public interface ---------------------------------------------------------------------------------------------------
def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_two_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    block = hdr[hdr.index("gate expressions on device vectors"):hdr.index("dense multilinear extensions on device-resident")]
    assert hdr.index("int ark_hip_prefix_scan_plan(") < hdr.index("gate expressions on device vectors")   # after the prefix scans
    for name, value in (("COLUMNS", MAX_COLUMNS), ("TERMS", MAX_TERMS), ("DEGREE", MAX_DEGREE)):
        assert re.search(r"#define ARK_HIP_SOP_MAX_%s\s+%d\n" % (name, value), block), name
    emap = open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    exported = re.findall(r"global:\s*([^;]+);", emap)
    L = _lib.lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity, name
        assert name not in hooks and name + "(" in block, name
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pats in exported for pat in pats.split()), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert name not in _lib.TEST_SYMBOLS and hasattr(L, name), name


def test_the_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    for name, value in (("COLUMNS", MAX_COLUMNS), ("TERMS", MAX_TERMS), ("DEGREE", MAX_DEGREE)):
        assert "pub const ARK_HIP_SOP_MAX_%s: c_uint = %d;" % (name, value) in src, name
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    found = dict((n, len([a for a in args.split(",") if a.strip()]))
                 for n, args in re.findall(r"pub fn (ark_hip_\w+)\s*\(([^;]*?)\)\s*(?:->\s*[^;]+)?;", ext, flags=re.S))
    dev = open(os.path.join(ROOT, "rust", "ark-hip", "src", "device.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for name, arity in NAMES.items():
        assert found.get(name) == arity, name
        assert "sys::%s(" % name in dev, name
        assert name + "(" in hpp, name
    assert "pub struct SumOfProducts<" in dev and "class SumOfProducts {" in hpp
    for method in ("add_product", "set_constant", "evaluate"):
        assert hasattr(A.SumOfProducts, method)
        assert "pub fn %s(" % method in dev and " %s(" % method in hpp, method
    assert hasattr(A.DeviceVec, "rotate") and "pub fn rotate(" in dev and " rotate(" in hpp
    assert callable(A.sum_of_products_plan) and "pub fn sum_of_products_plan(" in dev and "sum_of_products_plan(" in hpp
    assert (A.gates.MAX_COLUMNS, A.gates.MAX_TERMS, A.gates.MAX_DEGREE) == (MAX_COLUMNS, MAX_TERMS, MAX_DEGREE)


class _FakeVec(A.DeviceVec):
    """a DeviceVec that owns nothing: the builder's checks need a length, a field and a pointer, not a device"""

    def __init__(self, field, length, ptr):
        self.field, self.len, self.cap, self.ptr = A.curves.field_id(field), length, length, C.c_void_p(ptr)

    def free(self):
        self.ptr = C.c_void_p(0)


def test_the_builder_refuses_without_a_device():
    f = "BLS12_381_FR"
    v = [_FakeVec(f, 8, 4096 * (k + 1)) for k in range(MAX_COLUMNS + 1)]
    s = A.SumOfProducts(f, 8)
    with pytest.raises(ValueError):
        s.evaluate()                                                          # no products
    with pytest.raises(ValueError):
        s.add_product([])
    with pytest.raises(ValueError):
        s.add_product([v[0]] * (MAX_DEGREE + 1))
    with pytest.raises(ValueError):
        s.add_product([_FakeVec(f, 9, 1 << 20)])                              # a length mismatch
    with pytest.raises(ValueError):
        s.add_product([_FakeVec("BN254_FR", 8, 1 << 20)])
    with pytest.raises(ValueError):
        s.add_product([(v[0], 1 << 63)])                                      # not an int64
    with pytest.raises(ValueError):
        s.add_product([(v[0], I64_MIN - 1)])
    with pytest.raises(TypeError):
        s.add_product([np.zeros((8, 4), dtype=np.uint64)])
    assert s.products == [] and s.columns == []                               # a refused product leaves nothing behind
    s.add_product([v[0], (v[1], I64_MIN), (v[0], I64_MAX)]).add_product([_FakeVec(f, 8, 4096)] * MAX_DEGREE)   # v[0]'s pointer again
    assert len(s.columns) == 2 and s.products[1][1] == [(0, 0)] * MAX_DEGREE
    for k in range(2, MAX_COLUMNS):
        s.add_product([v[k]])
    assert len(s.columns) == MAX_COLUMNS and len(s.products) == MAX_TERMS
    with pytest.raises(ValueError):
        s.add_product([v[0]])                                                 # a 17th product
    t = A.SumOfProducts(f, 8)
    t.add_product(v[:8])
    t.add_product(v[8:16])
    with pytest.raises(ValueError):
        t.add_product([v[0], v[16]])                                          # a 17th column
    assert len(t.columns) == MAX_COLUMNS and len(t.products) == 2
    with pytest.raises(ValueError):
        t.evaluate(out=_FakeVec(f, 9, 1 << 21))
    with pytest.raises(ValueError):
        A.SumOfProducts("BLS12_381_FQ", 8)
    with pytest.raises(ValueError):
        v[0].rotate(1, out=_FakeVec(f, 7, 1 << 21))
