"""CPU-side checks of the sparse matrices on the device (no GPU needed): the big-integer model of tests/csr_ref.py against a
naive dense product, the row plan's invariants on random and adversarial row_ptr, argument errors reported before any device
is touched, and the four entries as part of the public C ABI (header, exports, Python / Rust / C++ mirrors).  The kernels
themselves, and the argument errors of ark_hip_fr_csr_mul_device that need a live handle, are checked on the GPU by
tests/test_gpu_csr.py."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from algebra_amd import _lib
import algebra_amd as A
import csr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ark_hip_fr_csr_create": 9, "ark_hip_fr_csr_free": 1, "ark_hip_fr_csr_mul_device": 6, "ark_hip_csr_plan": 7}
ERR_ARG, ERR_NO_DEVICE = -1, -5
FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]


def random_csr(rng, rows, cols, max_len):
    lens = rng.integers(0, max_len, size=rows, endpoint=True) if cols else np.zeros(rows, dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    col_idx = rng.integers(0, max(cols, 1), size=int(row_ptr[-1])).astype(np.uint32)   # duplicates inside a row happen
    return row_ptr, col_idx


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_the_model_against_a_naive_dense_product(fname):
    f = R.Field(fname)
    rng = np.random.default_rng(5)
    for rows, cols in ((0, 0), (1, 1), (3, 1), (1, 4), (5, 7), (9, 6)):
        row_ptr, col_idx = random_csr(rng, rows, cols, 5)
        nnz = int(row_ptr[-1])
        vals = R.rand_elems(f, nnz, 11 + rows)
        for j, special in zip(range(nnz), (0, f.one, f.enc(-1), f.p - 1)):
            vals[j] = special
        x = R.rand_elems(f, cols, 13 + cols)
        d = R.dense(f, rows, cols, row_ptr, col_idx, vals)
        xv = [v * f.rinv % f.p for v in x]                                   # canonical values
        want = [f.enc(sum(d[r][c] * xv[c] for c in range(cols))) for r in range(rows)]
        assert R.mul(f, rows, row_ptr, col_idx, vals, x) == want
        # the transposition: the dense transpose, the same entries, ascending original rows inside every row of M^T
        t_ptr, t_idx, t_vals = R.transpose(rows, cols, row_ptr, col_idx, vals)
        dt = R.dense(f, cols, rows, t_ptr, t_idx, t_vals)
        assert dt == [[d[r][c] for r in range(rows)] for c in range(cols)]
        assert int(t_ptr[cols]) == nnz and sorted(t_vals) == sorted(vals)
        for c in range(cols):
            seg = [int(v) for v in t_idx[int(t_ptr[c]):int(t_ptr[c + 1])]]
            assert seg == sorted(seg), (c, seg)
        u = R.rand_elems(f, rows, 17 + rows)
        mv = R.mul(f, rows, row_ptr, col_idx, vals, x)
        mtu = R.mul(f, cols, t_ptr, t_idx, t_vals, u)
        assert R.inner(f, u, mv) == R.inner(f, mtu, x) == R.bilinear(f, rows, row_ptr, col_idx, vals, u, x)


def test_the_model_keeps_duplicates_in_their_order():
    f = R.Field("BLS12_381_FR")
    row_ptr, col_idx = np.array([0, 3, 4], dtype=np.uint32), np.array([1, 1, 0, 1], dtype=np.uint32)
    vals = [f.enc(2), f.enc(3), f.enc(5), f.enc(7)]
    assert R.mul(f, 2, row_ptr, col_idx, vals, [f.enc(10), f.enc(100)]) == [f.enc(550), f.enc(700)]
    t_ptr, t_idx, t_vals = R.transpose(2, 2, row_ptr, col_idx, vals)
    assert list(t_ptr) == [0, 1, 4] and list(t_idx) == [0, 0, 0, 1] and t_vals == [f.enc(5), f.enc(2), f.enc(3), f.enc(7)]


# ---- the plan -----------------------------------------------------------------------------------------------------------
def _plan(row_ptr):
    rp = np.ascontiguousarray(row_ptr, dtype=np.uint32)
    t, mr = C.c_int(), C.c_int()
    b, lr, lc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = _lib.lib().ark_hip_csr_plan(rp.size - 1, rp.ctypes.data_as(C.c_void_p), C.byref(t), C.byref(mr), C.byref(b), C.byref(lr), C.byref(lc))
    assert rc == 0
    return t.value, mr.value, b.value, lr.value, lc.value


def _check(lens):
    """the library's counts are those of the restated rule, whose blocks keep every invariant"""
    row_ptr = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint32)
    rows = len(lens)
    T, MR, blocks, long_rows, long_chunks = _plan(row_ptr)
    stream, longs, order = R.plan(rows, row_ptr, T, MR)
    assert R.check_plan(rows, row_ptr, T, MR, stream, longs, order) == (blocks, long_rows, long_chunks), lens[:8]
    assert long_chunks == sum(-(-int(n) // T) for n in lens if n > T)
    assert long_rows == sum(1 for n in lens if n > T)
    assert A.csr_plan(rows, row_ptr) == (T, MR, blocks, long_rows, long_chunks)
    return T, MR, blocks, long_rows, long_chunks


def test_plan_constants():
    T, MR, blocks, long_rows, long_chunks = _plan([0])
    assert 256 <= T <= 1 << 16 and T & (T - 1) == 0 and MR >= 256
    assert (blocks, long_rows, long_chunks) == (0, 0, 0)                     # rows = 0
    t, mr = C.c_int(), C.c_int()
    assert _lib.lib().ark_hip_csr_plan(0, None, C.byref(t), C.byref(mr), None, None, None) == 0 and (t.value, mr.value) == (T, MR)


def test_plan_invariants_on_adversarial_rows():
    T, MR = _plan([0])[:2]
    L = [0, 1, T - 1, T, T + 1, 3 * T + 5]
    assert _check([0] * (3 * MR + 7))[2:] == (4, 0, 0)                        # all rows empty: max_rows alone closes blocks
    assert _check([0] * (MR + 1) + [1] + [0] * (2 * MR))[3:] == (0, 0)        # runs of empty rows longer than max_rows
    assert _check([3 * T + 5])[2:] == (0, 1, 4)                               # one row holding everything
    assert _check([T])[2:] == (1, 0, 0) and _check([T + 1])[2:] == (0, 1, 2)
    assert _check([1] * T)[2:] == (1, 0, 0) and _check([1] * (T + 1))[2:] == (2, 0, 0)
    assert _check([T - 1, 1, 1])[2:] == (2, 0, 0) and _check([1, T, 1])[2:] == (3, 0, 0)
    assert _check([T + 1, T + 1])[2:] == (0, 2, 4)                            # two long rows in succession
    assert _check([1, T + 1, 1])[2:] == (2, 1, 2) and _check([T + 1, 1])[2:] == (1, 1, 2) and _check([1, T + 1])[2:] == (1, 1, 2)
    for a in L:                                                               # every ordered triple of the listed lengths
        for b in L:
            for c in L:
                _check([a, b, c])
    rng = np.random.default_rng(24)
    for _ in range(40):
        lens = list(rng.choice(L, size=int(rng.integers(1, 12))))
        for _ in range(int(rng.integers(0, 3))):                              # with runs of empty and of single-entry rows between
            at = int(rng.integers(0, len(lens) + 1))
            lens[at:at] = [int(rng.integers(0, 2))] * int(rng.integers(1, 2 * MR + 3))
        _check(lens)
    for _ in range(10):                                                       # R1CS-like: 1 to 4 per row
        _check(list(rng.integers(1, 4, size=int(rng.integers(1, 3 * T)), endpoint=True)))


def test_plan_argument_errors():
    L = _lib.lib()
    bad = [np.array(v, dtype=np.uint32) for v in ([1, 2, 3], [0, 5, 4, 6], [0, 2, 1])]
    for rp in bad:
        assert L.ark_hip_csr_plan(rp.size - 1, rp.ctypes.data_as(C.c_void_p), None, None, None, None, None) == ERR_ARG
    assert L.ark_hip_csr_plan(3, None, None, None, None, None, None) == ERR_ARG
    assert L.ark_hip_csr_plan(1 << 32, None, None, None, None, None, None) == ERR_ARG


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_create_argument_errors_come_before_any_device_use():
    """every violation of create's contract is ARK_HIP_ERR_ARG with or without a GPU and leaves *out untouched; without a GPU a
    well-formed call is ARK_HIP_ERR_NO_DEVICE.  No well-formed call is made when a GPU is present: nothing here uses one."""
    L = _lib.lib()
    F = 3                                            # BLS12_381_FR
    create = L.ark_hip_fr_csr_create
    rows, cols = 3, 4
    rp = np.array([0, 2, 2, 5], dtype=np.uint32)
    ci = np.array([0, 3, 1, 1, 2], dtype=np.uint32)
    va = np.zeros((5, 4), dtype=np.uint64)
    SENTINEL = 0x5A5A5A5A

    def call(field=F, rows=rows, cols=cols, rp=rp, ci=ci, va=va, nnz=5, flags=0, out=True):
        h = C.c_void_p(SENTINEL)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        rc = create(field, rows, cols, p(rp), p(ci), p(va), nnz, flags, C.byref(h) if out else None)
        assert h.value == SENTINEL
        return rc

    def arr(v):
        return np.array(v, dtype=np.uint32)
    assert call(field=99) == ERR_ARG and call(field=0) == ERR_ARG           # unknown; a base field is not served
    assert call(rp=arr([0, 3, 2, 5])) == ERR_ARG                            # non-monotone row_ptr
    assert call(rp=arr([1, 2, 2, 5])) == ERR_ARG                            # row_ptr[0] != 0
    assert call(rp=arr([0, 2, 2, 4])) == ERR_ARG and call(nnz=4) == ERR_ARG and call(nnz=6) == ERR_ARG   # row_ptr[rows] != nnz
    assert call(ci=arr([0, 4, 1, 1, 2])) == ERR_ARG                         # a column equal to cols
    assert call(cols=3) == ERR_ARG
    assert call(ci=arr([0, 3, 1, 1, 0xFFFFFFFF])) == ERR_ARG
    assert call(flags=2) == ERR_ARG and call(flags=3) == ERR_ARG and call(flags=1 << 31) == ERR_ARG   # unknown flag bits
    assert call(rp=None) == ERR_ARG and call(ci=None) == ERR_ARG and call(va=None) == ERR_ARG
    assert call(out=False) == ERR_ARG
    assert call(rows=1 << 32) == ERR_ARG and call(cols=1 << 32) == ERR_ARG and call(nnz=1 << 32) == ERR_ARG
    assert call(rows=0, cols=0, rp=None, ci=None, va=None, nnz=1) == ERR_ARG
    assert call(rows=2, cols=0, rp=arr([0, 0, 1]), ci=arr([0]), va=va[:1], nnz=1) == ERR_ARG   # cols = 0 admits no entry
    mul = L.ark_hip_fr_csr_mul_device
    x, y = C.c_void_p(1 << 20), C.c_void_p(2 << 20)
    for t in (0, 1, 2, -1):
        assert mul(None, t, x, 4, y, 3) == ERR_ARG                          # no handle
    assert L.ark_hip_fr_csr_free(None) == 0                                  # NULL is fine, with or without a device
    if L.ark_hip_device_count() == 0:                # well-formed calls: loud refusal, no CPU fallback
        assert call() == ERR_NO_DEVICE and call(flags=1) == ERR_NO_DEVICE
        assert call(rows=0, cols=0, rp=None, ci=None, va=None, nnz=0) == ERR_NO_DEVICE
        assert call(rows=0, cols=5, rp=arr([0]), ci=None, va=None, nnz=0) == ERR_NO_DEVICE
        assert call(rows=2, cols=0, rp=arr([0, 0, 0]), ci=None, va=None, nnz=0) == ERR_NO_DEVICE


# ---- the public interface ---------------------------------------------------------------------------------------------------
def _decls(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char\*)\s+(ark_hip_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_the_four_entries_are_public_c_abi():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    i, j = hdr.index("#ifdef ARK_HIP_TEST_HOOKS"), hdr.index("#endif /* ARK_HIP_TEST_HOOKS */")
    public, hooks = _decls(hdr[:i] + hdr[j:]), _decls(hdr[i:j])
    block = hdr[hdr.index("sparse constraint matrices on the device"):hdr.index("the sumcheck prover's round on device tables")]
    assert "typedef struct ark_hip_fr_csr ark_hip_fr_csr;" in block and "#define ARK_HIP_CSR_WITH_TRANSPOSE 1u" in block
    emap = open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    exported = re.findall(r"global:\s*([^;]+);", emap)
    L = _lib.lib()
    for name, arity in NAMES.items():
        assert public.get(name) == arity, name
        assert name not in hooks and name + "(" in block, name
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pats in exported for pat in pats.split()), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name


def test_the_mirrors_have_the_entries():
    src = open(os.path.join(ROOT, "rust", "ark-hip-sys", "src", "lib.rs")).read()
    assert "pub struct ark_hip_fr_csr {" in src and "pub const ARK_HIP_CSR_WITH_TRANSPOSE: c_uint = 1;" in src
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
    assert "pub struct CsrMatrix<" in dev and "class CsrMatrix {" in hpp
    for method in ("mul", "mul_t", "bilinear"):
        assert hasattr(A.CsrMatrix, method)
        assert "pub fn %s(" % method in dev and " %s(" % method in hpp, method
    assert hasattr(A.CsrMatrix, "free") and "void free()" in hpp and "impl<F: FftField> Drop for CsrMatrix<F>" in dev
    assert callable(A.csr_plan) and "pub fn csr_plan(" in dev and "inline CsrPlan csr_plan(" in hpp
