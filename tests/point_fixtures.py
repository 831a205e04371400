"""Inputs for the point-array tests (tests/test_gpu_point_arrays.py, tests/test_host_group_helpers.py), built with the
plain Python-integer arithmetic of tests/pyref.py: independent of the library and of the oracle.

    zero_masks(n, B)   where a lane-batched inversion (lane_batch_inverse, csrc/ec.cuh) is handed zeros
    affine_chain(...)  distinct affine points of a curve, by a Curve.add chain
    lift(...)          an affine point as a Jacobian representative (x l^2, y l^3, l) with a chosen l
"""
import functools

import numpy as np

import pyref as P

# Values per lane of the lane-batched inversion.  This MIRRORS csrc: fr_div_kernel instantiates lane_batch_inverse<F, 8>
# (devops.cuh), the point kernels LaneBatch<F>::B = 8 for a base field of at most 64 bytes (the G1 curves) and 4 for
# Fp2 (ec.cuh).  If LaneBatch changes, the masks below stop aiming at whole lanes, last slots and ragged lanes: change
# these constants with it.
B_FR = 8
B_G1 = 8
B_FP2 = 4


def lane_batch(cname):
    return B_FP2 if cname.endswith("G2") else B_G1


def lane_slots(n, B):
    """[lane t] -> the indices it owns, slot 0 first: t + j L for j < B, below n (L = ceil(n / B) lanes)."""
    L = -(-n // B)
    return [[t + j * L for j in range(B) if t + j * L < n] for t in range(L)]


MASK_NAMES = ("none", "all", "lanes_0_and_last", "slot0_of_odd_lanes", "last_slot_of_lanes_1_mod_3",
              "lanes_2_and_Lm2_but_last_slot", "lane_1_but_slot0", "random_half")


def zero_masks(n, B):
    """{name: sorted index array} of the zero patterns that FIT n values in lanes of B: a pattern that comes out empty
    (its lanes do not exist) or equal to an earlier one is not handed out, so every mask but "none" plants a zero and no
    two are the same.  What collapses at the small sizes (L = ceil(n / B) lanes):
      n <= B (one lane: n = 1, B - 1, B): "lanes_0_and_last" is "all"; no odd lane, no lane 1 or 2, so the four lane
        patterns are empty; "random_half" stays (at n = 1 it is "all" and dropped);
      n = B + 1 (two lanes, of ceil and floor of n / 2 values: consecutive indices belong to consecutive lanes):
        "lanes_0_and_last" is "all"; "last_slot_of_lanes_1_mod_3" is lane 1's last value; lane 2 does not exist and
        lane L - 2 is lane 0; "slot0_of_odd_lanes" is index 1 alone; with B = 4 lane 1 holds two values, so
        "lane_1_but_slot0" is its last value once more and dropped.
    At every larger size the tests use (five lanes and more) all eight are handed out."""
    lanes = lane_slots(n, B)
    L = len(lanes)
    assert sorted(i for s in lanes for i in s) == list(range(n)) and all(lanes)   # every index owned once, no empty lane
    rng = np.random.default_rng(0x5EED + 31 * n + B)
    cand = {
        "none": [],
        "all": list(range(n)),
        "lanes_0_and_last": lanes[0] + (lanes[L - 1] if L > 1 else []),
        "slot0_of_odd_lanes": [lanes[t][0] for t in range(1, L, 2)],
        "last_slot_of_lanes_1_mod_3": [lanes[t][-1] for t in range(1, L, 3)],
        "lanes_2_and_Lm2_but_last_slot": [i for t in sorted({2, L - 2}) if 0 <= t < L for i in lanes[t][:-1]],
        "lane_1_but_slot0": lanes[1][1:] if L > 1 else [],
        "random_half": sorted(int(i) for i in rng.permutation(n)[: (n + 1) // 2]),
    }
    assert tuple(cand) == MASK_NAMES
    if (B - 1) * L < n:   # lane 0 is a full lane: the whole-lane mask really zeroes B values of ONE lane
        assert len(lanes[0]) == B and set(lanes[0]) <= set(cand["lanes_0_and_last"])
        assert [i % L for i in lanes[0]] == [0] * B
    out, seen = {}, []
    for name, idx in cand.items():
        key = sorted(set(idx))
        assert len(key) == len(idx) and all(0 <= i < n for i in key), name
        if name != "none" and (not key or key in seen):
            continue
        seen.append(key)
        out[name] = np.array(key, dtype=np.int64)
    assert all(v.size for k, v in out.items() if k != "none")       # every mask handed out differs from the empty one
    return out


def has_full_lane(n, B):
    return (B - 1) * (-(-n // B)) < n


@functools.lru_cache(maxsize=None)
def curve(cname):
    return P.Curve(cname)


@functools.lru_cache(maxsize=None)
def generator(cname):
    """the curve's generator as a pyref point (the oracle's constant, decoded and checked against the curve equation)"""
    import oracle_lib as O
    g = curve(cname).dec(O.generator(O.CID[cname]))
    assert g is not None and curve(cname).on_curve(g)
    return g


@functools.lru_cache(maxsize=None)
def affine_chain(cname, n, start=3, step=5):
    """n distinct affine points [start + i step] G, i < n, by repeated Curve.add (never the identity: n step << r)"""
    cv = curve(cname)
    g = generator(cname)
    d = cv.mul(g, step)
    pts = [cv.mul(g, start)]
    for _ in range(n - 1):
        pts.append(cv.add(pts[-1], d))
    assert all(p is not None for p in pts)
    return tuple(pts)


def lambdas(cname, n, seed):
    """per point a non-zero l of the base field: random, 1, p - 1 in turn; over Fp2 also l with c0 = 0 and with c1 = 0"""
    cv = curve(cname)
    p = cv.p
    rng = np.random.default_rng(seed)
    rnd = lambda: 1 + int.from_bytes(rng.bytes(56), "little") % (p - 1)
    out = []
    for i in range(n):
        if cv.F.beta is None:
            out.append((rnd(), 1, p - 1)[i % 3])
        else:
            out.append(((rnd(), rnd()), (1, 0), (p - 1, 0), (0, rnd()), (rnd(), 0))[i % 5])
    return out


def lift(cname, pt, lam):
    """Jacobian limbs (x l^2 | y l^3 | l) of the affine point pt: z = l != 1, and into_affine gives pt back"""
    cv = curve(cname)
    F = cv.F
    l2 = F.mul(lam, lam)
    return np.concatenate([F.enc(F.mul(pt[0], l2)), F.enc(F.mul(pt[1], F.mul(l2, lam))), F.enc(lam)])


def identity_rows(cname, count, seed):
    """`count` Jacobian encodings of the identity: the canonical (1, 1, 0) and (x, y, 0) with arbitrary non-zero x, y
    (not on the curve: z = 0 alone makes the identity), alternating"""
    cv = curve(cname)
    F = cv.F
    rng = np.random.default_rng(seed)
    rnd = lambda: 1 + int.from_bytes(rng.bytes(56), "little") % (cv.p - 1)
    el = (lambda: rnd()) if F.beta is None else (lambda: (rnd(), rnd()))
    one = F.from_int(1)
    rows = []
    for k in range(count):
        x, y = (one, one) if k % 2 == 0 else (el(), el())
        rows.append(np.concatenate([F.enc(x), F.enc(y), F.enc(F.zero())]))
    return np.stack(rows) if rows else np.zeros((0, 3 * cv.fw), dtype=np.uint64)
