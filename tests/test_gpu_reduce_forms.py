"""The bucket reduction in every form it can take: level-0 chunk length L0 any integer (ragged last chunk, per-window
bucket counts, T_w = A_w + L0 V_w on the host) x second stage in one kernel (bit-sliced over all pairs) or in two digits
(row and column sums, then the bit-sliced sums of those).  Each setting runs in a fresh child process
(tests/reduce_forms_child.py): ARK_HIP_MSM_SPLIT_LEVEL and other knobs of the library are read once per process.  The
expected value is always the oracle's."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L0S = (1, 3, 7, 16, 21, 32, 53)
FORMS = {"one_kernel": "0", "two_digit": "1"}


def child(mode, l0, form, **extra):
    env = dict(os.environ, ARK_HIP_MSM_L0=str(l0), ARK_HIP_MSM_STAGE2=FORMS[form], **extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reduce_forms_child.py"), mode], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "reduce-forms ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("l0", L0S)
def test_every_chunk_length_and_stage2_form_matches_the_oracle(l0, form):
    """BLS12-381 G1, BN254 G1, BLS12-377 G2 at 2^12, 2^16, 2^19 pairs.  2^(c-1) buckets per window are a power of two, so
    L0 = 3, 7, 21, 53 never divide them (ragged last chunk, m = ceil(2^(c-1) / L0) not a power of two: the low digit's
    D = 2^d does not divide m either)."""
    child("grid", l0, form)


@pytest.mark.parametrize("l0,form", [(21, "two_digit"), (7, "one_kernel")])
def test_two_window_groups_match_the_oracle(l0, form):
    """The same grid with two window groups forced (by default from 2^25 pairs): at 2^19 -- the smallest size that takes them
    -- the second group's sort runs on the side stream under the first group's accumulate kernel."""
    child("grid", l0, form, ARK_HIP_MSM_GROUPS="2")


@pytest.mark.parametrize("l0,form", [(3, "two_digit"), (7, "two_digit"), (16, "two_digit"), (21, "two_digit"), (3, "one_kernel"),
                                     (32, "one_kernel")])
def test_rare_branches(l0, form):
    """One occupied bucket (first, last, at a row boundary), equal sums and opposite sums meeting in a row and in a column
    (the full addition's doubling and identity branches inside the trees), the largest digits (the last bucket of a
    full, a narrow and the top window).  The width probe is off so that the plan is the one the inputs were built for."""
    child("rare", l0, form, ARK_HIP_MSM_PROBE="0")


@pytest.mark.parametrize("l0,form", [(21, "two_digit"), (7, "one_kernel"), (16, "two_digit")])
def test_sharded_sums_and_streamed_pieces_read_the_same_part_sums(l0, form):
    child("entries", l0, form)
