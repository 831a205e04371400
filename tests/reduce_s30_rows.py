"""Inputs and the comparison of the full addition's raw hook (csrc/s30test_api.hpp: ADD_FULL, ADD_FULL_ACC), shared by the device
test (tests/test_gpu_reduce_s30.py) and the host twin's (tests/test_lazy30_add_host.py): stored points in, the oracle's
bucket + bucket out."""
import numpy as np

import lazy30_add_model as AM
import lazy30_model as M
import oracle_lib as O

CID = O.CID["BLS12_381_G1"]
FW = O.fe_words(CID)
L = M.L
A4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)
B4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)


def words(fe):
    """one coordinate (FW 64-bit words) -> 12 32-bit words"""
    return np.ascontiguousarray(fe, dtype=np.uint64).view(np.uint32).tolist()


def pairs():
    """(a, b) stored points as rows of 4 FW uint64 words"""
    fone = np.zeros(FW, dtype=np.uint64)
    r = O.field_const(O.curve_info(CID)[0], 1)
    fone[:r.size] = r
    inf = np.concatenate([fone, fone, np.zeros(2 * FW, dtype=np.uint64)])
    n = 64
    bases = O.gen_bases(CID, A4, B4, n)
    sums = []
    for i in range(n):                      # sums of one to four bases: denominators that are one and that are not
        acc = inf.copy()
        for j in range(1 + i % 4):
            acc = O.point_op(CID, "bkt_add_aff", acc, bases[(i + 7 * j) % n])
        sums.append(acc)
    rng = np.random.default_rng(23)
    out = [(sums[int(i)], sums[int(j)]) for i, j in zip(rng.integers(0, n, 256), rng.integers(0, n, 256))]
    neg = lambda p: np.concatenate([p[:FW], O.basefield_op(CID, "neg", p[FW:2 * FW]), p[2 * FW:]])
    for i in (0, 1, 2, 3, 5):
        out += [(sums[i], sums[i]), (sums[i], neg(sums[i])), (inf, sums[i]), (sums[i], inf)]
    out.append((inf, inf))
    # the same point under two denominators: G + 7 G' summed in the two orders is not available without a dlog; use P as a sum and
    # P as the oracle's doubling of nothing: (P + Q) - Q against P
    back = O.point_op(CID, "bkt_add_bkt", O.point_op(CID, "bkt_add_bkt", sums[0].copy(), sums[9]), neg(sums[9]))
    out += [(back, sums[0]), (sums[0], back), (back, neg(sums[0]))]
    # coordinates at the stored words 0, 1 and p - 1 (field values only: the addition is arithmetic)
    p = M.P_INT
    fe = lambda v: np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(FW)], dtype=np.uint64)
    edge = [fe(0), fe(1), fe(p - 1)]
    k = 0
    for x in edge:
        for y in edge:
            for zz in edge[1:]:             # zz = 0 is the identity, above
                a = np.concatenate([x, y, zz, edge[(k + 1) % 3]])
                b = np.concatenate([edge[(k + 2) % 3], edge[k % 3], edge[1 + k % 2], y])
                out += [(a, sums[k % n]), (sums[(k + 3) % n], a), (a, b)]
                k += 1
    return out


def packed_rows(ps):
    rows = [AM.pack_points([words(a[i * FW:(i + 1) * FW]) for i in range(4)], [words(b[i * FW:(i + 1) * FW]) for i in range(4)]) for a, b in ps]
    packed = np.array(rows, dtype=np.uint32).view(np.int32)
    assert packed.shape == (len(ps), AM.ADD_IN)
    return packed


def check_against_oracle(ps, out):
    """out: the hook's output rows (int32, 4 slots of 13 words) for the pairs ps"""
    got = np.ascontiguousarray(out, dtype=np.int32).view(np.uint32).reshape(len(ps), 4, L)
    assert not got[:, :, M.N32:].any()
    want = np.stack([O.point_op(CID, "bkt_add_bkt", a.copy(), b) for a, b in ps]).view(np.uint32).reshape(len(ps), 4, M.N32)
    inf_want = ~want[:, 2].any(axis=1)
    inf_got = ~got[:, 2, :M.N32].any(axis=1)
    assert np.array_equal(inf_got, inf_want), "infinity"
    assert int(inf_want.sum()) >= 7 and int((~inf_want).sum()) >= 256
    live = ~inf_want
    assert np.array_equal(got[live][:, :, :M.N32], want[live]), "!= oracle, canonical word for canonical word"
