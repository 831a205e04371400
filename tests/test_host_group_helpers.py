"""ark_hip_sw_sum and ark_hip_sw_into_affine on the host (no GPU): the multi-GPU combine, the ChunkedPippenger sum and the
normalisation half of the GPU tests compare through, on equal, opposite and identity operands and on representatives
with z != 1.  Expected values come from tests/pyref.py (Curve.add on Python integers), compared limb for limb."""
import numpy as np
import pytest

import algebra_amd as A
import oracle_lib as O
import point_fixtures as X


def _sum_expected(cname, pts):
    cv = X.curve(cname)
    acc = None
    for p in pts:
        acc = cv.add(acc, p)
    return cv.enc(acc)


def _check_sum(cname, pts, rows):
    """pts: pyref points (None = identity); rows: their Jacobian limbs, one row each (n may be 0)"""
    cid = O.CID[cname]
    got = A.sum_projective(cid, rows)
    assert np.array_equal(A.into_affine(cid, got), _sum_expected(cname, pts)), (cname, len(pts))


@pytest.mark.parametrize("cname", O.CURVES)
def test_sw_sum_on_equal_opposite_and_identity_operands(cname):
    cv = X.curve(cname)
    fw = cv.fw
    chain = X.affine_chain(cname, 52)
    lam = X.lambdas(cname, 60, 0x50 + O.CID[cname])
    row = lambda k, l: X.lift(cname, chain[k], lam[l])
    neg = lambda k, l: X.lift(cname, cv.neg(chain[k]), lam[l])
    ident = X.identity_rows(cname, 4, 9)
    Pp, Qq = chain[0], chain[1]
    _check_sum(cname, [], np.zeros((0, 3 * fw), dtype=np.uint64))                       # n = 0: the identity
    _check_sum(cname, [Pp], np.stack([row(0, 0)]))                                      # n = 1
    _check_sum(cname, [None], ident[1:2])                                               # n = 1, (x, y, 0)
    _check_sum(cname, [None, Pp, None, None, Qq, None],
               np.stack([ident[0], row(0, 0), ident[1], ident[2], row(1, 4), ident[3]]))   # identities first, inside, last
    _check_sum(cname, [None, None], ident[:2])
    _check_sum(cname, [Pp, Pp], np.stack([row(0, 0), row(0, 0)]))                       # doubling, the same limbs twice
    _check_sum(cname, [Pp, Pp], np.stack([row(0, 0), row(0, 3)]))                       # doubling, two representatives
    _check_sum(cname, [Pp, Pp, Pp], np.stack([row(0, 1), row(0, 2), row(0, 5)]))
    _check_sum(cname, [Pp, cv.neg(Pp)], np.stack([row(0, 0), neg(0, 0)]))
    _check_sum(cname, [Pp, cv.neg(Pp)], np.stack([row(0, 0), neg(0, 3)]))               # opposite, other representative
    _check_sum(cname, [Pp, cv.neg(Pp), Qq], np.stack([row(0, 0), neg(0, 6), row(1, 7)]))   # through the identity and on
    _check_sum(cname, [Qq, Pp, cv.neg(Pp)], np.stack([row(1, 8), row(0, 9), neg(0, 10)]))
    pts = list(chain[2:52])                                                             # 50 points, every kind of z
    _check_sum(cname, pts, np.stack([X.lift(cname, p, lam[10 + i]) for i, p in enumerate(pts)]))


@pytest.mark.parametrize("cname", O.CURVES)
def test_sw_into_affine_of_lifted_points(cname):
    cv = X.curve(cname)
    cid = O.CID[cname]
    F = cv.F
    chain = X.affine_chain(cname, 52)
    n = 40
    lam = X.lambdas(cname, n, 0x1A + cid)                    # random, 1, p - 1 (Fp2: also c0 = 0, c1 = 0) in turn
    one, minus_one = F.from_int(1), F.from_int(cv.p - 1)
    assert one in lam and minus_one in lam
    rows = np.stack([X.lift(cname, chain[i], lam[i]) for i in range(n)])
    exp = np.stack([cv.enc(chain[i]) for i in range(n)])
    ident = X.identity_rows(cname, 6, 77)                    # (1, 1, 0) and z = 0 with arbitrary x, y
    for k, at in enumerate((0, 7, 8, 21, 38, 39)):
        rows[at] = ident[k]
        exp[at] = 0
    assert np.array_equal(A.into_affine(cid, rows), exp)
    for i in (0, 1, 2, 7, 39):                               # one point per call (what the C++ / Rust wrappers do)
        assert np.array_equal(A.into_affine(cid, rows[i]), exp[i])
    assert A.into_affine(cid, np.zeros((0, 3 * cv.fw), dtype=np.uint64)).shape == (0, 2 * cv.fw)
    # z = 1 exactly as the oracle's generators come: affine limbs with the Montgomery one appended
    z1 = np.stack([np.concatenate([cv.enc(chain[i]), F.enc(one)]) for i in range(5)])
    assert np.array_equal(A.into_affine(cid, z1), np.stack([cv.enc(chain[i]) for i in range(5)]))


@pytest.mark.parametrize("B", [X.B_FR, X.B_FP2])
def test_zero_masks_cover_what_they_claim(B):
    """the pattern helper itself: whole lanes are whole, every pattern handed out plants a zero, and the sizes around the
    workgroup seam get all eight"""
    for n in (1, B - 1, B, B + 1, 128 * B - 1, 128 * B, 128 * B + 1, 256 * B + 1):
        m = X.zero_masks(n, B)
        lanes = X.lane_slots(n, B)
        L = len(lanes)
        assert m["none"].size == 0 and m["all"].size == n
        if L >= 5:
            assert tuple(m) == X.MASK_NAMES
            assert set(lanes[0]) | set(lanes[L - 1]) == set(m["lanes_0_and_last"].tolist())
            assert set(lanes[2][:-1]) | set(lanes[L - 2][:-1]) == set(m["lanes_2_and_Lm2_but_last_slot"].tolist())
            assert lanes[2][-1] not in m["lanes_2_and_Lm2_but_last_slot"] and lanes[1][0] not in m["lane_1_but_slot0"]
            assert len(m["lane_1_but_slot0"]) == len(lanes[1]) - 1
        if n > 128 * B:                                          # a second workgroup of 128 lanes, with ragged lanes in it
            assert L > 128 and X.has_full_lane(n, B) and len(lanes[L - 1]) < B
    assert X.has_full_lane(128 * B + 1, B) and not X.has_full_lane(B + 1, B)
