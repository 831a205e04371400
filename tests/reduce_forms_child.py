"""Child process of tests/test_gpu_reduce_forms.py: one setting of the bucket reduction's knobs (ARK_HIP_MSM_L0,
ARK_HIP_MSM_STAGE2 -- in the environment this process was started with), every MSM checked against the oracle.
    python tests/reduce_forms_child.py grid | rare | entries
Inputs are the synthetic P_i = (a + i b)G of tools/synth.py, so the expected point is one scalar multiplication of the
oracle's: k G with k = sum_i s_i (a + idx_i b) mod r."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import algebra_amd as A
import oracle_lib as O
import synth as S
from algebra_amd import curves as cv

L0 = int(os.environ.get("ARK_HIP_MSM_L0", "0"))


def want_point(cid, k):
    return O.to_affine(cid, O.scalar_mul(cid, O.generator(cid), S.limbs4(k)))


def layout(c, bits):
    """(W, narrow) of the signed-digit windows: W windows of c bits, the top `narrow` one bit narrower (msm_window_layout)."""
    w = (bits + c - 1) // c
    deficit = w * c - bits
    if deficit > w or c < 3:
        return (bits + 1 + c - 1) // c, 0
    return w, deficit


def geometry(cid, n, r):
    """window offsets / widths of the plan for n pairs, and the second stage's two digits for this process's L0"""
    c, W = A.msm_plan(cid, n)
    Wl, narrow = layout(c, r.bit_length())
    assert Wl == W, (c, W, Wl)
    widths = [c - 1 if w >= W - narrow else c for w in range(W)]
    off = [sum(widths[:w]) for w in range(W)]
    mwin = 1 << (c - 1)
    l0 = min(L0, mwin)
    m = (mwin + l0 - 1) // l0
    nbits = max(0, (m - 1).bit_length())
    d = nbits // 2
    return dict(c=c, W=W, narrow=narrow, widths=widths, off=off, mwin=mwin, l0=l0, m=m, D=1 << d, rows=(m + (1 << d) - 1) >> d)


def to_limbs(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


def run_device(cid, bases_t, idx, vals, r):
    """MSM of the bases gathered by idx with the integer scalars vals, device resident, against k G"""
    ab = cv.affine_bytes(cid)
    gathered = bases_t.view(-1, ab)[torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()].contiguous().view(-1)
    sc = to_limbs(vals)
    d = torch.from_numpy(sc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    k = sum(v * (S.A0 + int(i) * S.B0) for v, i in zip(vals, idx)) % r
    got = A.into_affine(cid, A.msm_bigint(cid, gathered, d))
    return np.array_equal(got, want_point(cid, k))


def grid():
    # the three curve families (one lane per point on 28- and 29-bit limbs, a lane pair over Fp2) at three sizes
    for cname, logs in (("BLS12_381_G1", (12, 16, 19)), ("BN254_G1", (12, 16, 19)), ("BLS12_377_G2", (12, 16, 19))):
        cid = O.CID[cname]
        r = S.R[cv.scalar_field(cid)]
        bases = S.grow_bases(cid, 1 << max(logs), S.A0, S.B0, r)
        ab = cv.affine_bytes(cid)
        for logn in logs:
            n = 1 << logn
            sc = S.gen_scalars(n, 0x77 + logn, r)
            d = torch.from_numpy(sc.view(np.int64)).cuda()
            torch.cuda.synchronize()
            got = A.into_affine(cid, A.msm_bigint(cid, bases[: n * ab], d))
            assert np.array_equal(got, want_point(cid, S.dlog_of_msm(sc, S.A0, S.B0, r))), (cname, logn)
            print("ok", cname, logn, A.msm_plan(cid, n), flush=True)
        del bases
        torch.cuda.empty_cache()


def rare():
    # inputs a random vector never produces; every one checked against k G whatever branch it reaches
    for cname in ("BLS12_381_G1", "BLS12_377_G2"):
        cid = O.CID[cname]
        r = S.R[cv.scalar_field(cid)]
        n = 1 << 12
        g = geometry(cid, n, r)
        c, W, off, widths, l0, D, m = g["c"], g["W"], g["off"], g["widths"], g["l0"], g["D"], g["m"]
        bases = S.grow_bases(cid, n, S.A0, S.B0, r)
        rng = np.random.default_rng(0xB0 + L0)
        all_idx = list(range(n))
        narrow_half = 1 << (c - 2)                       # digits 1 .. narrow_half exist in every window without a carry
        # (a) all scalars equal: ONE occupied bucket per window -- the first, the last carry-free one, and the buckets on
        # both sides of a row boundary of the second stage (pair j = D h: buckets l0 D h - 1 and l0 D h)
        digits = [1, narrow_half - 1]
        edge = l0 * D * (1 if g["rows"] > 1 else 0)
        for k in (edge - 1, edge, edge + l0 - 1):
            if 0 <= k < narrow_half - 1:
                digits.append(k + 1)
        for dg in digits:
            s = sum(dg << off[w] for w in range(W - 1))  # (the top window stays empty: s < r / 2, no fold)
            assert run_device(cid, bases, all_idx, [s] * n, r), (cname, "one bucket", dg)
        # fillers for the cases below: window 0 holds nothing but the planted digits
        def fillers(count):
            return [(int(rng.integers(1, 1 << 62)) << off[1]) for _ in range(count)]
        # pairs j1, j2 of window 0 whose sums meet in a row (same h: adjacent lanes of the tree, and the same lane serially)
        # and in a column (same l)
        lps, slots = 1, (32 if cname.endswith("G2") else 64)     # lanes per row / column sum (msm_enqueue's rule)
        while lps < slots and lps * 8 < max(D, g["rows"]):
            lps *= 2
        meets = [(0, 1)]
        if lps < D:
            meets.append((0, lps))
        if g["rows"] > 1:
            meets.append((1, D + 1))
        for j1, j2 in meets:
            if j2 >= m or l0 * j2 + 1 >= (1 << (c - 1)):
                continue
            d1, d2 = l0 * j1 + 1, l0 * j2 + 1           # the first bucket of chunks j1 and j2, as digits
            # (b) the SAME point in both buckets: base 5 under two different digits -> P + P inside the sums
            idx = [5, 5] + all_idx[2:]
            vals = [d1, d2] + fillers(n - 2)
            assert run_device(cid, bases, idx, vals, r), (cname, "equal sums", j1, j2)
            # (c) P and -P: digit d1 and digit -d2 (the scalar 2^c - d2: window 0 recodes to -d2 and carries 1 upwards)
            vals = [d1, (1 << c) - d2] + fillers(n - 2)
            assert run_device(cid, bases, idx, vals, r), (cname, "opposite sums", j1, j2)
        # (d) the largest digit: raw = 2^(width - 1) recodes to -2^(width - 1), the LAST bucket of the window (the end of a
        # ragged last chunk when l0 does not divide the bucket count), in window 0, in a narrow window and -- through the
        # carry -- next to the top; and the largest digit the top window can hold below r / 2
        big = [(1 << (widths[0] - 1)) << off[0], (1 << (widths[W - 2] - 1)) << off[W - 2], ((r // 2) >> off[W - 1]) << off[W - 1]]
        vals = (big * n)[:n]
        assert run_device(cid, bases, all_idx, vals, r), (cname, "largest digits")
        vals = big + [int.from_bytes(rng.bytes(31), "little") % (r // 2) for _ in range(n - 3)]
        assert run_device(cid, bases, all_idx, vals, r), (cname, "largest digits among random ones")
        print("ok rare", cname, g, flush=True)
        del bases


def entries():
    # (e) the sharded part sums and the streamed pieces read the same [w][q] sums with the same L0 as the one-piece job
    from algebra_amd._lib import test_lib
    cid = O.CID["BLS12_381_G1"]
    r = S.R[cv.scalar_field(cid)]
    world, per = 4, 3000
    n = world * per
    bases_t = S.grow_bases(cid, n, S.A0, S.B0, r)
    ab = cv.affine_bytes(cid)
    sc = S.gen_scalars(n, 0xE5, r)
    want = want_point(cid, S.dlog_of_msm(sc, S.A0, S.B0, r))
    d = torch.from_numpy(sc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    one_piece = A.into_affine(cid, A.msm_bigint(cid, bases_t, d))
    assert np.array_equal(one_piece, want)
    db = [bases_t[k * per * ab:(k + 1) * per * ab].clone() for k in range(world)]
    ds = [d.view(-1)[k * per * 4:(k + 1) * per * 4].clone() for k in range(world)]
    torch.cuda.synchronize()
    pb = (C.c_void_p * world)(*[t.data_ptr() for t in db])
    ps = (C.c_void_p * world)(*[t.data_ptr() for t in ds])
    pn = (C.c_size_t * world)(*[per] * world)
    out = np.zeros(3 * O.fe_words(cid), dtype=np.uint64)
    path = C.c_int(0)
    rc = test_lib().ark_hip_test_msm_sharded_emulated(cid, world, pb, ps, pn, 0, out.ctypes.data_as(C.c_void_p), C.byref(path))
    assert rc == 0 and path.value == 1, (rc, path.value)
    assert np.array_equal(A.into_affine(cid, out), one_piece)
    print("ok sharded", flush=True)
    hb = bases_t.cpu().numpy().view(np.uint64).reshape(n, -1)
    A.base_cache_config(8 << 30, 0)
    A.base_cache_clear()
    for pieces in (2, 5):
        os.environ["ARK_HIP_STREAM_PIECES"] = str(pieces)
        for _ in range(2):      # bases streamed with the scalars, then found resident
            assert np.array_equal(A.into_affine(cid, A.msm_bigint(cid, hb, sc)), one_piece), pieces
    print("ok streamed", flush=True)


if __name__ == "__main__":
    {"grid": grid, "rare": rare, "entries": entries}[sys.argv[1]]()
    print("reduce-forms ok", flush=True)
