"""The bucket reduction's full addition on 13 signed 30-bit digits (csrc/ec30s.cuh: xyzz_add_s; AccOps of csrc/msm.cuh where the
base field has the signed form: BLS12-381 G1) on the device.

The addition itself, lane by lane (ark_hip_test_s30_op, ops 12 and 13 of csrc/s30test_api.hpp): two stored points in, their
sum out in the reference's canonical form, which must be the oracle's bucket + bucket word for word -- 256 random pairs of sums
with denominators, P + P (the doubling), P + (-P), inf + P, P + inf, inf + inf, and operands whose coordinates are the stored
words 0, 1 and p - 1; with the second operand read from memory and taken from an accumulator of its own.

The kernels: MSM parity against the oracle at 2^10 and 2^12 pairs in a child process per level-0 kernel
(tests/reduce_s30_child.py; ARK_HIP_MSM_SPLIT_LEVEL is read once per process), the plan forced through both second stages, narrow
top windows, heavy runs, duplicate and opposite bases inside a bucket's first two entries and buckets of one, two and three
entries."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lazy30_add_model as AM
import reduce_s30_rows as R
from algebra_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_device(op, rows, out_words):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((rows.shape[0], out_words), dtype=np.int32)
    _lib.check(_lib.test_lib().ark_hip_test_s30_op(op, rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), rows.shape[0]),
               "test_s30_op")
    return out


@pytest.mark.parametrize("op", ["add_full", "add_full_acc"])
def test_full_addition_on_the_device_is_the_oracles(op):
    ps = R.pairs()
    assert len(ps) >= 256 + 21 + 54
    R.check_against_oracle(ps, run_device(AM.OPS[op], R.packed_rows(ps), AM.ADD_OUT))


@pytest.mark.parametrize("split", ["0", "1"])
def test_msm_parity_through_every_reduction_kernel(split):
    env = dict(os.environ, ARK_HIP_MSM_SPLIT_LEVEL=split)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reduce_s30_child.py")], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "reduce-s30 ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
