"""Child process of tests/test_gpu_merkle.py::test_poisoned_scratch: the openings of a Merkle tree with the library's reused device
scratch POISONED in between (the protocol of tests/scratch_reuse_child.py).

    ARK_HIP_LIB=algebra_amd/libark_hip_test.so python tests/merkle_scratch_child.py

Per field: a large opening (300 indices: sizes the staging buffer), a small one (warm), poison every scratch buffer with the word 1,
then a small opening and a paths-only one against the model; afterwards no scratch buffer has moved, no byte of any buffer's slack
has changed, and the staging buffer was asked for exactly paths | rows | indices of the larger of the two."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import algebra_amd as A
import merkle_ref as R
from algebra_amd import _lib

WORD = 0x00000001
assert os.path.realpath(_lib.LIB_PATH) == os.path.realpath(_lib.TEST_LIB_PATH), "run with ARK_HIP_LIB=libark_hip_test.so"
T = _lib.test_lib()
assert T._handle == _lib.lib()._handle, "the mirror and the hooks must be one library instance"


def report():
    n = C.c_size_t(0)
    rc = T.ark_hip_test_scratch_report(WORD, None, 0, C.byref(n))
    assert rc in (0, -2) and n.value > 60, (rc, n.value)
    rows = (_lib.ScratchRow * n.value)()
    _lib.check(T.ark_hip_test_scratch_report(WORD, rows, n.value, C.byref(n)), "ark_hip_test_scratch_report")
    return {r.name.decode(): r for r in rows}


def staged_bytes(q, log, count, eb, rows=True):
    body = q * log * 32 + (q * count * eb if rows else 0)
    return ((body + 15) & ~15) + 8 * q


def opened(tree, model, cols, idx, rows=True):
    got_rows, paths = tree.open(idx, rows=rows)
    ok = all(paths[i].tobytes() == b"".join(R.path(model, ix)) for i, ix in enumerate(idx))
    if rows:
        ok = ok and all(got_rows[i].tolist() == [c[ix] for c in cols] for i, ix in enumerate(idx))
    return ok


LOG, COUNT = 9, 5
for field in ("BABYBEAR", "GOLDILOCKS", "KOALABEAR"):
    n, eb = 1 << LOG, R.elem_bytes(field)
    r = R.rng(160 + eb)
    cols = R.random_columns(field, r, COUNT, n)
    model = R.tree(field, cols)
    tree = A.SmallDeviceMatrix.from_host(field, np.array(cols, dtype=np.uint32 if eb == 4 else np.uint64)).commit()
    assert tree.root == model[0], field
    big = [r.randrange(n) for _ in range(300)]
    small = [n - 1, 0, 7, 7, n // 2]
    assert opened(tree, model, cols, big) and opened(tree, model, cols, small), (field, "warm")
    _lib.check(T.ark_hip_test_scratch_poison(WORD), "ark_hip_test_scratch_poison")
    assert opened(tree, model, cols, small), (field, "stale read: a small opening on poisoned scratch")
    assert opened(tree, model, cols, small[:3], rows=False), (field, "stale read: paths only on poisoned scratch")
    rows = report()
    bad = [(k, v.cap, v.asked, v.regrown, v.dirty_beyond, v.first_dirty_offset) for k, v in rows.items() if v.regrown or v.dirty_beyond]
    assert not bad, (field, "name, cap, asked, regrown, dirty_beyond, first_dirty_offset", bad)
    assert rows["merkle_stage"].asked == staged_bytes(len(small), LOG, COUNT, eb), (field, rows["merkle_stage"].asked)
    assert rows["merkle_stage"].cap >= staged_bytes(300, LOG, COUNT, eb)
    print("ok", field, flush=True)
