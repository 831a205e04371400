"""What survives between calls: the library's device workspaces live as long as the process, only grow and are not cleared.
Every other GPU test starts from fresh (in practice zeroed) memory or repeats one shape, where a stale read returns the right
answer of the previous call and a write past the end of an array lands in slack nobody reads.  Here every scratch buffer
(csrc/scratch_list.hpp) is filled with a poison word between calls, and the slack behind what each call asked for is checked
afterwards: no call reads what it did not write, no kernel writes past what it asked for.

One child process (tests/scratch_reuse_child.py, which documents the protocol) per case, run against libark_hip_test.so through
ARK_HIP_LIB so that the Python mirror and the hooks are one library instance; MSM knobs are read once per process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("ARK_HIP_GFFT_SLAB_LOG", "ARK_HIP_POINTVEC_SLAB_LOG", "ARK_HIP_MSM_L0", "ARK_HIP_MSM_STAGE2", "ARK_HIP_MSM_GROUPS", "ARK_HIP_MSM_RUN_PARTS", "ARK_HIP_MSM_LAZY", "ARK_HIP_MSM_PROBE",
         "ARK_HIP_STREAM_PIECES")


def child(mode, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scratch_reuse_child.py"), mode], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and ("scratch-reuse ok " + mode) in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


def test_the_harness_fails_when_it_should():
    """ark_hip_test_scratch_selfcheck: a poisoned cell nothing wrote reads back as the poison; four bytes planted in the slack of
    one buffer (inside its capacity) are reported as that buffer's dirty_beyond == 4 and fail the children's own check."""
    out = child("selfcheck")
    assert "ok selfcheck: the planted overrun fails assert_clean" in out and "ok selfcheck\n" in out


@pytest.mark.parametrize("curve", ["bls12_381_g1", "bn254_g1", "bls12_377_g2"])
def test_msm_device_entry(curve):
    """uniform scalars at 2^12, 3000, 1 and 0 pairs, Montgomery scalars and the u8 / u16 / u64 entries at 2^12; each warm,
    poisoned, and poisoned after 2^16"""
    out = child("msm_" + curve)
    assert out.count("\nok ") + out.startswith("ok ") == 8, out


def test_msm_compaction_and_heavy_runs_at_2_19():
    """where the width probe runs: 60 % zero scalars (nzcnt / cscal / cidx) and one value for all scalars (hlist / hitems /
    hpart), after 2^20"""
    out = child("msm_large")
    assert "ok zeros 2^19" in out and "ok equal scalars 2^19" in out


def test_msm_other_entries():
    """prepared bases (hfinal), two jobs in flight (lane 1's workspace), the emulated sharded sum (comm_sums), the host-pointer
    entry with the cache off, and the streamed host entry in 5 pieces (ring_*, piece_buckets) after a one-piece call"""
    out = child("msm_entries")
    for case in ("prepared 4096", "two jobs 4096", "sharded 4 x 3000", "host 4096", "host streamed 12000 in 5 pieces"):
        assert "ok " + case in out, (case, out)


@pytest.mark.parametrize("l0,stage2", [("21", "1"), ("7", "0")])
def test_msm_rare_inputs_under_reduction_knobs(l0, stage2):
    """reduce_forms_child.rare's inputs at 2^12 (one occupied bucket, ragged last chunk, the largest digits)"""
    assert "ok rare x" in child("msm_rare", ARK_HIP_MSM_L0=l0, ARK_HIP_MSM_STAGE2=stage2, ARK_HIP_MSM_PROBE="0")


def test_msm_two_window_groups():
    child("msm_groups", ARK_HIP_MSM_GROUPS="2")


def test_msm_run_parts():
    child("msm_run_parts", ARK_HIP_MSM_RUN_PARTS="2")


def test_msm_saturated_kernels():
    child("msm_saturated", ARK_HIP_MSM_LAZY="0")


@pytest.mark.parametrize("field", ["bn254_fr", "bls12_381_fr", "bls12_377_fr"])
def test_fft(field):
    """2^10 forward, coset and inverse after 2^16; the host-pointer entry; degree-aware with 5 coefficients at 2^12; a batch of 3
    at 2^12; poly_mul 300 x 70 after 5000 x 5000; the smallest two- and three-pass plans (the ping buffer); fft_axis with G = 4"""
    out = child("fft_" + field)
    assert out.count("\nok ") + out.startswith("ok ") == 11, out


def test_polynomial_ops_and_mle():
    """evaluate / divide by x - z at T + 1 and 65 after T^2 + 1 (three scan levels), inner product at 4097 after 2^20, Lagrange
    coefficients at 2^10 after 2^14, MLE evaluate and fix_variables at 2^9 after 2^16"""
    out = child("poly")
    assert out.count("\nok ") + out.startswith("ok ") == 5, out


def test_point_arrays():
    """sw_mul and fold at 65 after 1000, the host-slice sw_mul, the host check and the host decompress at 65 rows with planted
    bad rows after 1000, normalize_batch and batch_mul host entries at 129 after 4097"""
    out = child("points")
    assert out.count("\nok ") + out.startswith("ok ") == 7, out


def test_point_vector_slabs():
    """sw_mul at 1000 with ARK_HIP_POINTVEC_SLAB_LOG at its smallest"""
    assert "ok sw_mul 1000" in child("points_slab", ARK_HIP_POINTVEC_SLAB_LOG="6")


def test_group_fft():
    """the coset inverse transform of 2^5 group elements after 2^8"""
    assert "ok group coset ifft 2^5" in child("gfft")


def test_group_fft_slabs():
    """2^8 group elements in slabs of 2^6 (ARK_HIP_GFFT_SLAB_LOG=6)"""
    assert "ok group coset ifft 2^8" in child("gfft_slab", ARK_HIP_GFFT_SLAB_LOG="6")
