"""Child process of tests/test_gpu_fri.py: the device entries of ark_hip_xfp_* / ark_hip_fri_* behind a busy context stream, in
the pattern of tests/async_contract_child.py (these entries are outside tests/async_cases.py by name: none ends in _device).

    ARK_HIP_LIB=algebra_amd/libark_hip_test.so python tests/fri_async_child.py

The blocker: BLOCKER_CALLS batched transforms of BLOCKER_COLS Goldilocks columns of 2^20 words, queued on the context stream.
Every case: warm the call (table builds synchronise: they happen here), restore the outputs to their stale content, queue the
blocker, make the calls under test, overwrite the host copies of their challenges at once, ask ark_hip_test_context_busy (a case
whose blocker has already finished is INCONCLUSIVE and fails), wait, compare with the model.  The last case makes two folds with
different challenges and one wait."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import algebra_amd as A
import fri_ref as X
from algebra_amd import _lib

assert os.path.realpath(_lib.LIB_PATH) == os.path.realpath(_lib.TEST_LIB_PATH), "run with ARK_HIP_LIB=libark_hip_test.so"
T = _lib.test_lib()
L = _lib.lib()
assert T._handle == L._handle, "the mirror and the hooks must be one library instance"
BLOCKER_CALLS, BLOCKER_COLS, BLOCKER_LOG = 16, 32, 20
FAILURES = []
vp = C.c_void_p


def ok(rc, what):
    if rc != 0:
        print("%s failed with code %d: the child stops here" % (what, rc), flush=True)
        raise SystemExit(3)


def busy():
    b = C.c_int(-1)
    ok(T.ark_hip_test_context_busy(C.byref(b)), "ark_hip_test_context_busy")
    return b.value == 1


def sync():
    ok(L.ark_hip_synchronize(), "ark_hip_synchronize")


class Blocker:
    def __init__(self):
        self.dom = A.SmallRadix2EvaluationDomain.new("GOLDILOCKS", 1 << BLOCKER_LOG)
        self.mat = A.SmallDeviceMatrix("GOLDILOCKS", BLOCKER_COLS, 1 << BLOCKER_LOG)
        self.queue(2)     # tables and the ping buffer at their sizes
        sync()

    def queue(self, calls=BLOCKER_CALLS):
        for i in range(calls):
            self.mat.fft_in_place(self.dom, inverse=bool(i & 1))


def elem4(e):
    a = (C.c_uint64 * 4)()
    for k, v in enumerate(e):
        a[k] = int(v)
    return a


def cols(x, elems):
    return np.array([[e[k] for e in elems] for k in range(x.d)], dtype=np.uint64 if x.bytes == 8 else np.uint32)


def elems_of(arr):
    return [tuple(int(v) for v in arr[:, i]) for i in range(arr.shape[1])]


def case(name, x, blocker, calls, outputs):
    """calls: [(fn(host_constant) -> rc, constant, replacement)]; outputs: [(SmallExtVec, want elements)]"""
    stale = {id(v): v.to_host() for v, _ in outputs}
    for fn, const, _ in calls:      # warm-up with the same constants
        ok(fn(elem4(const)), name + " (warm-up)")
    sync()
    for v, _ in outputs:
        s = np.full_like(stale[id(v)], 0xA5)
        ok(L.ark_hip_memcpy_h2d(v._p, s.ctypes.data_as(vp), s.nbytes), "ark_hip_memcpy_h2d")
    blocker.queue()
    for fn, const, other in calls:
        host = elem4(const)
        ok(fn(host), name)
        for k in range(4):          # the host copy dies: another valid element
            host[k] = int(other[k]) if k < len(other) else 0
    was_busy = busy()
    sync()
    if not was_busy:
        FAILURES.append(name + ": inconclusive, the blocker had finished before the host side of the case was done")
    for v, want in outputs:
        if elems_of(v.to_host()) != want:
            FAILURES.append(name + ": an output differs from the model")
    print(name, "busy" if was_busy else "NOT busy", flush=True)


def main():
    blocker = Blocker()
    for fname in ("BABYBEAR", "GOLDILOCKS"):
        x = X.FIELDS[fname]
        rng = X.rng(7)
        k, a = 10, 2
        n = 1 << k
        dom = A.SmallRadix2EvaluationDomain.new(fname, n).get_coset(x.st(x.gen))
        layer = [x.random_element(rng) for _ in range(n)]
        plain = [x.plain(e) for e in layer]
        b1, b2, other = x.random_element(rng), x.random_element(rng), x.random_element(rng)
        vin = A.SmallExtVec.from_host(fname, cols(x, layer))
        out1, out2 = A.SmallExtVec(fname, n >> a), A.SmallExtVec(fname, n >> a)

        def fold_into(out):
            return lambda beta: L.ark_hip_fri_fold(x.sid, C.byref(dom._s), a, beta, vin._p, vin.stride, out._p, out.stride)

        w1 = [x.stored(e) for e in x.fold_eval(plain, k, x.gen, a, x.plain(b1))]
        w2 = [x.stored(e) for e in x.fold_eval(plain, k, x.gen, a, x.plain(b2))]
        case("fold " + fname, x, blocker, [(fold_into(out1), b1, other)], [(out1, w1)])
        case("two folds, one wait " + fname, x, blocker, [(fold_into(out1), b2, other), (fold_into(out2), b1, other)], [(out1, w2), (out2, w1)])
        src =A.SmallExtVec.from_host(fname, cols(x, layer))
        dst = A.SmallExtVec(fname, n)
        wc = [x.stored(x.mul(u, x.plain(b1))) for u in plain]
        case("vec_mul_const " + fname, x, blocker,
             [(lambda kk: L.ark_hip_xfp_vec_mul_const(x.sid, src._p, src.stride, kk, dst._p, dst.stride, n), b1, other)], [(dst, wc)])
        count = 5
        base = [[rng.randrange(x.p) for _ in range(n)] for _ in range(count)]
        mat = A.SmallDeviceMatrix.from_host(fname, np.array(base, dtype=src.matrix.vec.dtype))
        comb = A.SmallExtVec(fname, n)
        wcomb = [x.stored(e) for e in x.combine([[x.pl(v) for v in c] for c in base], x.plain(b2), 3)]
        case("combine_columns " + fname, x, blocker,
             [(lambda al: L.ark_hip_xfp_combine_columns(x.sid, mat.vec._p, count, mat.stride, n, al, 3, comb._p, comb.stride, 0), b2, other)],
             [(comb, wcomb)])
    sync()
    print("fri async: %d failed" % len(FAILURES), flush=True)
    for f in FAILURES:
        print("  " + f, flush=True)
    return 1 if FAILURES else 0


if __name__ == "__main__":
    sys.exit(main())
