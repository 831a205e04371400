"""Input rows and the model's answers for the raw-digit hook ops that came with the unsigned gathered coordinate of the accumulate
kernel (csrc/s30test.cuh: ops 8 and 9, from_canonical_u and madd_entry, and op 0 on the unsigned operand class): shared by the
host-form test (tests/test_lazy30_diet_model_host.py) and the device test (tests/test_gpu_lazy30_diet.py)."""
import numpy as np

import lazy30_diet_model as D
import lazy30_model as M

HALF, L = M.HALF, M.L


def as_i32(rows):
    return (np.array(rows, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)


def slots(vecs):
    """digit / word vectors -> one row of 13-word slots"""
    out = []
    for v in vecs:
        out += list(v) + [0] * (L - len(v))
    return out


def raw_cases(points, seed=17):
    """op name -> (int32 input rows, int32 expected rows).  `points`: affine (x words, y words), canonical"""
    rng = np.random.default_rng(seed)
    cases = {}
    # the unsigned repack: 0, 1, p - 1, all ones below the top, random
    vals = [0, 1, M.P_INT - 1, M.P_INT >> 1, (1 << 380) - 1] + [int.from_bytes(rng.bytes(48), "little") % M.P_INT for _ in range(96)]
    cases["from_canonical_u"] = (as_i32([slots([M.to_words(v)]) for v in vals]), as_i32([D.from_canonical_u(M.to_words(v)) for v in vals]))
    # an unsigned operand with every digit at 2^30 - 1 (and the repack of p - 1, of random values) against normalised ones at +-2^29
    top = M.top_digit_bound(1)
    us = [[(1 << 30) - 1] * 12 + [(1 << 27) - 1], D.from_canonical_u(M.to_words(M.P_INT - 1))] + [D.from_canonical_u(M.to_words(v)) for v in vals[5:13]]
    ys = [[HALF] * 12 + [top], [-HALF] * 12 + [-top], [HALF if i & 1 else -HALF for i in range(12)] + [top],
          [-HALF if i & 1 else HALF for i in range(12)] + [-top], [HALF - 1] * 12 + [top], list(M.consts()["ONE"])] + M.random_digits(rng, 4)
    pairs = [(u, y) for u in us for y in ys]
    cases["mul"] = (as_i32([slots(p) for p in pairs]), as_i32([M.mul(*p) for p in pairs]))
    # the kernel's entry to the mixed addition over the branch chain, the base as +P and as -P: with the sign set the row carries the
    # NEGATED y, so both meet the same accumulator and must leave lazy30_model.madd's answer
    ins, outs = M.madd_rows(points)
    neg_y = lambda yw: M.to_words(M.P_INT - M.from_words(yw))
    srows, swant = [], []
    for row, want in zip(ins, outs):
        yw = row[5 * L + 1:5 * L + 13]
        srows += [list(row) + [0], list(row[:5 * L + 1]) + neg_y(yw) + [0, 1]]
        swant += [want, want]
    cases["madd_entry"] = (as_i32(srows), as_i32(swant))
    return cases


def compare(op, got, want):
    if op == "madd_entry":
        # an accumulator gone to infinity keeps whatever coordinates it had: only its flags are compared
        live = want[:, 4 * L] == 0
        assert np.array_equal(got[:, 4 * L:], want[:, 4 * L:]), op
        assert np.array_equal(got[live], want[live]), op
    else:
        assert np.array_equal(got, want), op
