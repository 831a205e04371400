"""Child process of tests/test_gpu_smallfp_fft.py::test_poisoned_scratch: the small-field transforms with the library's reused
device scratch POISONED in between (the protocol of tests/scratch_reuse_child.py).

    ARK_HIP_LIB=algebra_amd/libark_hip_test.so python tests/smallfp_scratch_child.py

Per field: a 2^16 coset transform (two passes: sizes the ping buffer), poison every scratch buffer, then a 2^9 transform (one
workgroup) and a batch of 3 columns at the first two-pass size, both against the model; afterwards no scratch buffer has moved and
no byte of any buffer's slack has changed.  The twiddle and power tables are caches and keep their content."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import algebra_amd as A
import smallfp_ref as R
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


def run(f, log, count, coset=True):
    dt = np.uint64 if f.bytes == 8 else np.uint32
    m, d = f.domain_new(1 << log), A.SmallRadix2EvaluationDomain.new(f.name, 1 << log)
    if coset:
        m, d = f.get_coset(m, f.gen), d.get_coset(f.gen)
    rng = R.rng(log * 10 + count)
    cols = [f.random_elements(rng, 1 << log) for _ in range(count)]
    v = A.SmallDeviceVec.from_host(f.name, np.array(cols, dtype=dt).reshape(-1))
    d.fft_batch_in_place(v.ptr, count)
    got = v.to_host().reshape(count, 1 << log)
    return all(np.array_equal(got[j], np.array(f.transform(m, cols[j]), dtype=dt)) for j in range(count))


for f in R.FIELDS.values():
    two_pass = A.small_fft_plan(f.name, 0)[0] + 1
    assert run(f, 16, 1), (f.name, "2^16")
    assert run(f, 9, 1) and run(f, two_pass, 3), (f.name, "warm")
    _lib.check(T.ark_hip_test_scratch_poison(WORD), "ark_hip_test_scratch_poison")
    assert run(f, 9, 1), (f.name, "stale read: 2^9 on poisoned scratch")
    assert run(f, two_pass, 3), (f.name, "stale read: a batch on poisoned scratch")
    rows = report()
    bad = [(k, r.cap, r.asked, r.regrown, r.dirty_beyond, r.first_dirty_offset) for k, r in rows.items() if r.regrown or r.dirty_beyond]
    assert not bad, (f.name, "name, cap, asked, regrown, dirty_beyond, first_dirty_offset", bad)
    assert rows["sfp.sfp_ping"].asked == 3 * (1 << two_pass) * f.bytes, (f.name, rows["sfp.sfp_ping"].asked)
    print("ok", f.name, flush=True)
