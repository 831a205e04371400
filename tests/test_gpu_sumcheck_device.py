"""The whole sumcheck proof in one wait (ark_hip_sumcheck_prove_device) and the transcript on the device.
Every proof is compared limb for limb -- rounds, point, final values, value and the transcript's end state -- with the
host-driven `prove` whose challenge callback is the `Transcript` host entry, and goes through the model's verifier
(tests/transcript_ref.py: hashlib.shake_256 and Python integers; tests/sumcheck_ref.py).  No tolerance anywhere.

`tail_vars` moves the seam between the round kernels (one launch chain per round) and the one-workgroup tail: the sizes below
are the smallest at which each seam exists."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
import fraction_sum_ref as FS
import grand_product_ref as GP
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S
import transcript_ref as T
from test_gpu_sumcheck import make_list, modulus, terms_of
from test_transcript_host import SEED, TAIL_MAX, challenge_cases, reduce_vectors

pytestmark = pytest.mark.gpu

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
MLE = A.DenseMultilinearExtension
ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def dev_table(fname, m, k):
    """table k of 2^m random elements with a zero, the residue p - 1 and the value -1 planted; uploaded once, never written.
    -> (device extension, Montgomery limbs)"""
    fid, p = O.FID[fname], modulus(fname)
    n = 1 << m
    a = O.gen_scalars(fid, 2300 + 16 * m + k, n, montgomery=True).copy()
    a[(k + 1) % n] = 0
    if n >= 4:
        a[(2 * k + 2) % n] = pyref.to_limbs(p - 1, 4)
        a[(n - 1 - k) % n] = pyref.to_mont(p - 1, p)
    a.setflags(write=False)
    return MLE.from_evaluations(fname, m, a), a


@functools.lru_cache(maxsize=None)
def canon(fname, m, k):
    return tuple(S.decode(dev_table(fname, m, k)[1], modulus(fname)))


def shape_terms(shape, fname):
    if shape == "eab":                                            # eq * a * b: three tables, one product, coefficient one
        return 3, [(1, [0, 1, 2])]
    if shape == "a":
        return 1, [(1, [0])]
    return terms_of(shape, fname)


def same_proof(got, want):
    return (len(got.rounds) == len(want.rounds) and all(np.array_equal(a, b) for a, b in zip(got.rounds, want.rounds)) and
            np.array_equal(got.point, want.point) and np.array_equal(got.final_evaluations, want.final_evaluations) and
            np.array_equal(got.final_value, want.final_value))


def check_proof(fname, m, shape, tail_vars):
    p = modulus(fname)
    nt, terms = shape_terms(shape, fname)
    mles = [dev_table(fname, m, k)[0] for k in range(nt)]
    plan = A.sumcheck_prove_plan(m, nt, tail_vars)
    lp, tr = make_list(fname, m, mles, terms), A.Transcript(fname, SEED)
    proof = lp.prove_device(tr, tail_vars)
    assert len(proof.rounds) == m and proof.point.shape == (m, 4) and proof.final_evaluations.shape == (nt, 4)
    # the host-driven prover, its challenges from the host entry
    host, th = make_list(fname, m, mles, terms), A.Transcript(fname, SEED)
    want = host.prove(lambda i, evals: th.challenge(evals))
    host.free()
    assert same_proof(proof, want), (fname, m, shape, tail_vars, plan)
    assert tr.state == th.state, "the end state"
    # the model's verifier, with its own transcript
    ints = [list(canon(fname, m, k)) for k in range(nt)]
    claim = sum(S.pair_values(row, row, terms, p)[0] for row in zip(*ints)) % p
    rounds, point, finals = [S.decode(g, p) for g in proof.rounds], S.decode(proof.point, p), S.decode(proof.final_evaluations, p)
    tv = T.Transcript(p, SEED)
    assert T.verify(claim, rounds, point, finals, terms, tv, p), "the model's verifier rejects"
    assert tv.state == tr.state
    assert finals == [mle_ref.evaluate(t, point, p) for t in ints]
    assert S.decode(proof.final_value.reshape(1, 4), p) == [S.pair_values(finals, finals, terms, p)[0]]
    for k in range(nt):
        assert np.array_equal(mles[k].to_evaluations(), dev_table(fname, m, k)[1]), "an input table changed"
    # again on the same list and the scratch the first left behind: prove_device keeps no state in the list
    tr2 = A.Transcript(fname, SEED)
    assert same_proof(lp.prove_device(tr2, tail_vars), proof) and tr2.state == tr.state
    lp.free()
    return proof


# ---- the transcript in a one-lane kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_device_reduction_is_the_model(fname):
    p, fid = modulus(fname), A.curves.field_id(fname)
    L = _lib.test_lib()
    out = np.zeros(4, dtype=np.uint64)
    for b in reduce_vectors(p):
        assert L.ark_hip_test_transcript_reduce(fid, b, 1, out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, T.reduce512(b, p)), int.from_bytes(b, "little")


@pytest.mark.parametrize("fname", FR)
def test_device_challenge_is_the_model(fname):
    p, fid = modulus(fname), A.curves.field_id(fname)
    L = _lib.test_lib()
    state, m = (C.c_uint8 * 32)(*SEED), T.Transcript(p, SEED)
    out = np.zeros(4, dtype=np.uint64)
    for i, els in enumerate(challenge_cases(p)):
        limbs = S.encode(els, p) if els else None
        assert L.ark_hip_test_transcript_challenge_device(fid, C.cast(state, C.c_void_p), None if limbs is None else limbs.ctypes.data_as(C.c_void_p),
                                                          len(els), out.ctypes.data_as(C.c_void_p)) == 0
        assert S.decode(out.reshape(1, 4), p) == [m.challenge(els)], (i, len(els))
        assert bytes(state) == m.state, (i, len(els))


# ---- whole proofs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("shape", ["a", "ab", "eab", "four", "eight_terms", "eight_tables"])
def test_term_shapes(fname, shape):
    """at 6 variables: the tail alone (default), round kernels handing over to the tail at 3, and no tail at all; the
    eight-table shape runs the NT = 8 kernels in every regime; coefficients 0, 1, p - 1 and random"""
    for tail in (None, 3, 0):
        check_proof(fname, 6, shape, tail)


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("m", [1, 2, 3])
def test_tail_only_with_idle_lanes(fname, m):
    """1, 2 and 4 pairs in a workgroup of 256 lanes; the m = 0 end inside the tail"""
    assert A.sumcheck_prove_plan(m, 4)[1:] == (1, m)
    check_proof(fname, m, "two_terms", None)
    check_proof(fname, m, "eight_tables", None)


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("t,above", [(t, d) for t in (1, 3, 9, 10) for d in (0, 1, 2)])
def test_the_seam_between_round_kernels_and_tail(fname, t, above):
    """tail_vars = t at nu = t, t + 1, t + 2: the hand-over right at, one above and two above the tail.  t = 9 is the last size
    one pass of 256 lanes covers, t = 10 the first where a lane walks two pairs."""
    m = t + above
    assert A.sumcheck_prove_plan(m, 4, t)[2] == t
    check_proof(fname, m, "two_terms" if (t + above) % 2 else "eab", t)


def test_eight_tables_where_a_tail_lane_walks_two_pairs():
    """the NT = 8 kernels at the large hand-over: round kernels with two reduction stages, then a tail from 10 variables"""
    check_proof("BLS12_381_FR", 11, "eight_tables", 10)
    check_proof("BN254_FR", 10, "eight_tables", 10)


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("m", [10, 11, 12])
def test_no_tail_where_the_reduction_gets_its_second_stage(fname, m):
    """round 0 (plain, over nu variables) has two stages from nu = 10, the binding rounds (over one variable less) from 11:
    every one of these proofs crosses from two stages to one"""
    assert A.sumcheck_plan(9, 2, 2)[2] == 1 and A.sumcheck_plan(10, 2, 2)[2] == 2
    assert A.sumcheck_plan(10, 2, 2, True)[2] == 1 and A.sumcheck_plan(11, 2, 2, True)[2] == 2
    assert A.sumcheck_prove_plan(m, 3, 0)[2] == 0
    check_proof(fname, m, "eab", 0)


@pytest.mark.parametrize("fname", FR)
def test_the_largest_tail(fname):
    assert A.sumcheck_prove_plan(TAIL_MAX + 1, 2, TAIL_MAX)[2] == TAIL_MAX
    check_proof(fname, TAIL_MAX + 1, "ab", TAIL_MAX)


@pytest.mark.parametrize("fname", FR)
def test_the_default_at_16_variables(fname):
    check_proof(fname, 16, "ab", None)


def test_a_small_proof_after_a_large_one():
    fname = "BLS12_381_FR"
    big = check_proof(fname, 14, "eab", 6)
    small = check_proof(fname, 4, "eab", 2)                        # on the scratch the large one left behind
    assert len(big.rounds) == 14 and len(small.rounds) == 4


def test_overlapping_work_is_refused_and_the_mirror_refuses_misuse():
    fname = "BLS12_381_FR"
    m, nt = 5, 2
    mles = [dev_table(fname, m, k)[0] for k in range(nt)]
    tabs = (C.c_void_p * nt)(*[t.evaluations.ptr.value for t in mles])
    lens, idx = (C.c_uint * 1)(2), (C.c_uint * 2)(0, 1)
    host = np.zeros((64, 4), dtype=np.uint64)
    hp = host.ctypes.data_as(C.c_void_p)
    state = (C.c_uint8 * 32)()
    work = A.DeviceVec(fname, A.sumcheck_prove_plan(m, nt)[0], _zero=False)

    def run(d_work):
        return _lib.lib().ark_hip_sumcheck_prove_device(A.curves.field_id(fname), tabs, nt, m, lens, idx, hp, 1, C.cast(state, C.c_void_p), -1,
                                                        d_work, hp, hp, hp, hp)
    assert run(work.ptr) == 0
    assert run(C.c_void_p(tabs[1])) == ERR_ARG
    assert run(C.c_void_p(tabs[0] + (32 << m) - 32)) == ERR_ARG
    assert run(None) == ERR_ARG
    lp = make_list(fname, m, mles, [(1, [0, 1])])
    with pytest.raises(ValueError):
        lp.prove_device(A.Transcript("BN254_FR", SEED))           # another field's transcript
    small = A.DeviceVec(fname, 4, _zero=False)
    with pytest.raises(ValueError):
        lp.prove_device(A.Transcript(fname, SEED), _work=small)   # a work vector that is too small
    lp.round()
    with pytest.raises(ValueError):
        lp.prove_device(A.Transcript(fname, SEED))                # rounds have been run
    for v in (work, small):
        v.free()
    lp.free()
    assert np.array_equal(mles[0].to_evaluations(), dev_table(fname, m, 0)[1])


# ---- the layered provers ----------------------------------------------------------------------------------------------
def model_challenge(tr):
    return lambda layer, rnd, values: tr.challenge(list(values))


def same_layers(got, want):
    assert len(got) == len(want)
    for (gs, gv), (ws, wv) in zip(got, want):
        assert (gs is None) == (ws is None) and np.array_equal(gv, wv)
        assert gs is None or same_proof(gs, ws)


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", [1, 2, 6, 11])
def test_grand_product_prove_device(fname, nv):
    p = modulus(fname)
    m, a = dev_table(fname, nv, 3)
    tr, th = A.Transcript(fname, SEED), A.Transcript(fname, SEED)
    proof = A.GrandProduct(m).prove_device(tr)
    want = A.GrandProduct(m).prove(lambda layer, rnd, values: th.challenge(values))
    assert np.array_equal(proof.product, want.product) and np.array_equal(proof.point, want.point) and tr.state == th.state
    same_layers(proof.layers, want.layers)
    product, layers, point = GP.decode_proof(proof, p)
    tv = T.Transcript(p, SEED)
    ok, vpoint, claim = GP.verify(nv, product, layers, model_challenge(tv), p)
    assert ok and vpoint == point and tv.state == tr.state
    assert product == GP.tree(list(canon(fname, nv, 3)), p)[0]
    assert claim == mle_ref.evaluate(list(canon(fname, nv, 3)), point, p)
    assert np.array_equal(m.to_evaluations(), a), "input changed"


@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("nv", [1, 2, 6, 11])
@pytest.mark.parametrize("has_num", [True, False])
def test_fractional_sum_prove_device(fname, nv, has_num):
    p = modulus(fname)
    den, d = dev_table(fname, nv, 5)
    num = dev_table(fname, nv, 4)[0] if has_num else None
    tr, th = A.Transcript(fname, SEED), A.Transcript(fname, SEED)
    proof = A.FractionalSum(num, den).prove_device(tr)
    want = A.FractionalSum(num, den).prove(lambda layer, rnd, values: th.challenge(values))
    assert np.array_equal(proof.root, want.root) and np.array_equal(proof.point, want.point) and tr.state == th.state
    same_layers(proof.layers, want.layers)
    root, layers, point = FS.decode_proof(proof, p)
    tv = T.Transcript(p, SEED)
    ok, vpoint, claim_n, claim_d = FS.verify(nv, has_num, root, layers, model_challenge(tv), p)
    assert ok and vpoint == point and tv.state == tr.state
    assert claim_d == mle_ref.evaluate(list(canon(fname, nv, 5)), point, p)
    if has_num:
        assert claim_n == mle_ref.evaluate(list(canon(fname, nv, 4)), point, p)
    assert np.array_equal(den.to_evaluations(), d), "denominators changed"


# ---- scratch ------------------------------------------------------------------------------------------------------------
def test_prove_device_on_poisoned_scratch():
    """tests/sumcheck_device_scratch_child.py: the proof at 12 variables with the tail from 8 warm, then with every scratch
    buffer poisoned (ark_hip_test_scratch_poison), then on poisoned scratch left behind by a larger call: the host-driven
    proof each time, nothing written past what was asked for"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sumcheck_device_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "sumcheck-device scratch ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
