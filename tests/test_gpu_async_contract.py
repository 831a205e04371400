"""The asynchrony contract of include/ark_hip.h behind a busy context stream: with an MSM in flight on
lane 0, everything a `*_device` entry enqueues sits behind it, and the second lane is free to run ahead.  Then
  A  a producer that forgot mark_producer() hands the MSM on the second lane its STALE output;
  B  a host argument read after the call returned is seen with what the test wrote there since;
  C  two calls with different constants and nothing in between show a constant staged in memory the second call reuses;
  D  a "the call waits for it" result that was not waited for is still the sentinel at return.
The cases are tests/async_cases.py, the runner is tests/async_contract_child.py: one fresh process per group against
libark_hip_test.so (the hooks ark_hip_test_context_busy / _job_lane / _producer_marks), one after the other."""
import os
import subprocess
import sys

import pytest

import async_cases as AC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", AC.GROUPS)
def test_async_contract(group):
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "async_contract_child.py"), group], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "async contract %s:" % group in out.stdout, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
