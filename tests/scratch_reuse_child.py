"""Child process of tests/test_gpu_scratch_reuse.py: calls of the library with its reused device scratch POISONED in between.

    ARK_HIP_LIB=algebra_amd/libark_hip_test.so python tests/scratch_reuse_child.py <mode>

The library keeps its device workspaces for the life of the process; they only grow and are not cleared.  Two rules keep that
sound: no call reads a cell it did not write itself, and no kernel writes past what its enqueue asked for.  Every case here
follows one protocol with the poison word 0x00000001 (as an index, offset or count it stays in bounds; as a limb it gives a
point that is neither on the curve nor the identity; as a flag it is a spurious error -- no scratch buffer holds 64-bit indices
or pointers: `part` and `hitems` are pairs of u32):
  1. warm:    run the call, compare with the oracle;
  2. poison:  fill every scratch buffer (whole capacity) and pinned staging area with the word, run the same call: the result
              equals the oracle's, no buffer moved (regrown == 0) and no byte of any buffer's slack [asked, cap) changed;
  3. shrink:  run a larger call of the same entry, poison, run the small call: the same two checks.
ARK_HIP_LIB makes the Python mirror (algebra_amd.*) and the hooks one library instance; the first assertion of every mode
proves it.  MSM knobs are read once per process, hence one process per knob setting.  Expected values come from the oracle:
MSMs of the synthetic bases P_i = (a + i b) G are k G with k = sum s_i (a + i b) mod r, one oracle scalar multiplication."""
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
from algebra_amd import _lib
from algebra_amd import curves as cv

WORD = 0x00000001
assert os.path.realpath(_lib.LIB_PATH) == os.path.realpath(_lib.TEST_LIB_PATH), "run with ARK_HIP_LIB=libark_hip_test.so"
T = _lib.test_lib()
assert T._handle == _lib.lib()._handle, "the mirror and the hooks must be one library instance"


def poison():
    _lib.check(T.ark_hip_test_scratch_poison(WORD), "ark_hip_test_scratch_poison")


def report():
    n = C.c_size_t(0)
    rc = T.ark_hip_test_scratch_report(WORD, None, 0, C.byref(n))
    assert rc in (0, -2) and n.value > 60, (rc, n.value)
    rows = (_lib.ScratchRow * n.value)()
    _lib.check(T.ark_hip_test_scratch_report(WORD, rows, n.value, C.byref(n)), "ark_hip_test_scratch_report")
    return {r.name.decode(): r for r in rows}


def assert_clean(case, reach=()):
    """after a poisoned run: no buffer moved, nothing written past what was asked for; `reach`: buffers the case is there for"""
    rows = report()
    bad = [(k, r.cap, r.asked, r.regrown, r.dirty_beyond, r.first_dirty_offset) for k, r in rows.items() if r.regrown or r.dirty_beyond]
    assert not bad, (case, "name, cap, asked, regrown, dirty_beyond, first_dirty_offset", bad)
    for name in reach:   # "prefix*": any of them (the FFT's ping buffers are one per stream, in the order of the stream handles)
        hit = [r for k, r in rows.items() if (k.startswith(name[:-1]) if name.endswith("*") else k == name)]
        assert hit and any(r.asked > 0 for r in hit), (case, "does not reach", name)
    return rows


def protocol(case, small, big=None, reach=(), warm=1):
    """small(), big(): run the call and return whether the result equals the oracle's.  warm: how many warm calls size every
    buffer the call can land in (2 for the host-pointer MSM entries, whose uploads alternate between two ring slots)"""
    for _ in range(warm):
        assert small(), (case, "warm")
    poison()
    assert small(), (case, "stale read: wrong result on poisoned scratch")
    assert_clean((case, "poisoned"), reach)
    if big is not None:
        assert big(), (case, "grower")
        poison()
        assert small(), (case, "stale read: wrong result on poisoned scratch after a larger call")
        assert_clean((case, "shrink"), reach)
    print("ok", case, flush=True)


def prove_one_instance(m):
    """the first assertion of every mode: after a poison (which resets the requests) one MSM of the Python mirror shows up in
    the hooks' report -- the mirror and the hooks are one library instance"""
    poison()
    assert m.uniform(1 << 10, 1)(), "warm-up MSM"
    assert report()["msm0.keys"].asked > 0, "the mirror's MSM did not run in the library the hooks look at"


# ---- MSM ---------------------------------------------------------------------------------------------------------------
def want_point(cid, k):
    return O.to_affine(cid, O.scalar_mul(cid, O.generator(cid), S.limbs4(k)))


def to_limbs(vals):
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64)


class Msm:
    """the synthetic base set of one curve on the device, and closures that run one MSM each against k G"""

    def __init__(self, cid, nmax):
        self.cid, self.r, self.ab = cid, S.R[cv.scalar_field(cid)], cv.affine_bytes(cid)
        self.bases = S.grow_bases(cid, nmax, S.A0, S.B0, self.r)
        self.nmax = nmax

    def dev(self, sc):
        d = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
        torch.cuda.synchronize()
        return d

    def eq(self, got, k):
        return np.array_equal(A.into_affine(self.cid, got), want_point(self.cid, k))

    def limbs(self, sc, montgomery=False):
        """device entry on canonical limbs [n, 4] (montgomery: the same values handed over as Montgomery residues)"""
        n = sc.shape[0]
        k = S.dlog_of_msm(sc, S.A0, S.B0, self.r) if n else 0
        give = to_limbs([S.scalar_int(row) * (1 << 256) % self.r for row in sc]) if montgomery else sc
        d = self.dev(give) if n else torch.zeros(0, dtype=torch.int64, device="cuda")
        fn = A.msm_unchecked if montgomery else A.msm_bigint
        return lambda: self.eq(fn(self.cid, self.bases[: n * self.ab], d), k)

    def uniform(self, n, seed, montgomery=False):
        return self.limbs(S.gen_scalars(n, seed, self.r) if n else np.zeros((0, 4), dtype=np.uint64), montgomery)

    def small(self, n, dtype, seed):
        vals = np.random.default_rng(seed).integers(0, np.iinfo(dtype).max, size=n, dtype=dtype, endpoint=True)
        k = sum(int(v) * (S.A0 + i * S.B0) for i, v in enumerate(vals)) % self.r
        d = torch.from_numpy(vals.view({1: np.uint8, 2: np.int16, 8: np.int64}[vals.itemsize])).cuda()
        torch.cuda.synchronize()
        fn = {1: A.msm_u8, 2: A.msm_u16, 8: A.msm_u64}[vals.itemsize]
        return lambda: self.eq(fn(self.cid, self.bases[: n * self.ab], d), k)

    def prepared(self, nb, seed):
        sc = S.gen_scalars(nb, seed, self.r)
        k = S.dlog_of_msm(sc, S.A0, S.B0, self.r)
        pb = A.PreparedBases(self.cid, self.bases[: nb * self.ab])
        d = self.dev(sc)
        return lambda: self.eq(pb.msm_bigint(d), k)

    def two_jobs(self, n, seed):
        scs = [S.gen_scalars(n, seed + j, self.r) for j in range(2)]
        ks = [S.dlog_of_msm(sc, S.A0, S.B0, self.r) for sc in scs]
        ds = [self.dev(sc) for sc in scs]

        def run():
            jobs = [A.msm_bigint_async(self.cid, self.bases[: n * self.ab], d) for d in ds]
            return all([self.eq(j.wait(), k) for j, k in zip(jobs, ks)])
        return run

    def sharded(self, world, per, seed):
        n = world * per
        sc = S.gen_scalars(n, seed, self.r)
        k = S.dlog_of_msm(sc, S.A0, S.B0, self.r)
        d = self.dev(sc)
        db = [self.bases[j * per * self.ab:(j + 1) * per * self.ab].clone() for j in range(world)]
        ds = [d.view(-1)[j * per * 4:(j + 1) * per * 4].clone() for j in range(world)]
        torch.cuda.synchronize()
        pb = (C.c_void_p * world)(*[t.data_ptr() for t in db])
        ps = (C.c_void_p * world)(*[t.data_ptr() for t in ds])
        pn = (C.c_size_t * world)(*[per] * world)

        def run():
            out = np.zeros(3 * O.fe_words(self.cid), dtype=np.uint64)
            path = C.c_int(0)
            rc = T.ark_hip_test_msm_sharded_emulated(self.cid, world, pb, ps, pn, 0, out.ctypes.data_as(C.c_void_p), C.byref(path))
            keep = (db, ds)  # noqa: F841 -- the shards stay alive with the closure
            return rc == 0 and path.value == 1 and self.eq(out, k)
        return run

    def host(self, n, seed, pieces=None):
        """the host-pointer entry (numpy in): bases and scalars are uploaded by the call"""
        sc = S.gen_scalars(n, seed, self.r)
        k = S.dlog_of_msm(sc, S.A0, S.B0, self.r)
        hb = self.bases[: n * self.ab].cpu().numpy().view(np.uint64).reshape(n, -1)

        def run():
            if pieces is None:
                os.environ.pop("ARK_HIP_STREAM_PIECES", None)
            else:
                os.environ["ARK_HIP_STREAM_PIECES"] = str(pieces)
            return self.eq(A.msm_bigint(self.cid, hb, sc), k)
        return run


def msm_curve(cname):
    """the device entry on one curve: uniform scalars at 2^12, 3000, 1 and 0 pairs, each also after 2^16; Montgomery scalars;
    the three small-scalar widths"""
    cid = O.CID[cname]
    m = Msm(cid, 1 << 16)
    prove_one_instance(m)
    big = m.uniform(1 << 16, 0x16)
    for n in (1 << 12, 3000, 1):
        protocol("%s uniform %d" % (cname, n), m.uniform(n, 0x20 + n % 97), big, reach=("msm0.keys", "msm0.buckets"))
    # 0 pairs: nothing is enqueued, and the poisoned pinned staging area must not reach the result (the identity)
    protocol("%s uniform 0" % cname, m.uniform(0, 0), big)
    protocol("%s montgomery 4096" % cname, m.uniform(1 << 12, 0x31, montgomery=True), big)
    for dt in (np.uint8, np.uint16, np.uint64):
        protocol("%s %s 4096" % (cname, np.dtype(dt).name), m.small(1 << 12, dt, 0x41), big)


def msm_large():
    """BLS12-381 G1 at 2^19, where the width probe runs: 60 % zeros (compaction) and one value for every scalar (heavy runs)"""
    cid = O.CID["BLS12_381_G1"]
    m = Msm(cid, 1 << 20)
    prove_one_instance(m)
    n = 1 << 19
    big = m.uniform(1 << 20, 0x20)
    sc = S.gen_scalars(n, 0x19, m.r)
    sc[np.random.default_rng(5).random(n) < 0.6] = 0
    protocol("zeros 2^19", m.limbs(sc), big, reach=("msm0.probe", "msm0.nzcnt", "msm0.cscal", "msm0.cidx"))
    one = S.gen_scalars(1, 0x77, m.r)
    protocol("equal scalars 2^19", m.limbs(np.repeat(one, n, axis=0)), big, reach=("msm0.probe", "msm0.hlist", "msm0.hitems", "msm0.hpart"))


def msm_entries():
    """BLS12-381 G1: prepared bases, two jobs in flight, the emulated sharded sum, the host-pointer entry plain and streamed"""
    cid = O.CID["BLS12_381_G1"]
    m = Msm(cid, 1 << 16)
    prove_one_instance(m)
    big = m.uniform(1 << 16, 0x16)
    protocol("prepared 4096", m.prepared(1 << 12, 0x51), m.prepared(1 << 16, 0x52), reach=("msm0.hfinal",))
    protocol("two jobs 4096", m.two_jobs(1 << 12, 0x61), m.two_jobs(1 << 16, 0x63), reach=("msm0.keys", "msm1.keys"))
    protocol("sharded 4 x 3000", m.sharded(4, 3000, 0xE5), big, reach=("comm_sums",))
    A.base_cache_config(0, 0)     # cache off: every host call uploads its bases
    A.base_cache_clear()
    protocol("host 4096", m.host(1 << 12, 0x71), m.host(1 << 16, 0x72), warm=2)
    protocol("host streamed 12000 in 5 pieces", m.host(12000, 0x73, pieces=5), m.host(1 << 16, 0x74, pieces=1),
             reach=("ring_s[0]", "ring_s[1]", "ring_b[0]", "ring_b[1]", "piece_buckets"), warm=2)
    os.environ.pop("ARK_HIP_STREAM_PIECES", None)


def msm_knob(logn, *reach):
    """one knob setting (in the environment): BLS12-381 G1, uniform scalars at 2^logn, after twice as many"""
    cid = O.CID["BLS12_381_G1"]
    n = 1 << logn
    m = Msm(cid, 2 * n)
    prove_one_instance(m)
    protocol("knob uniform 2^%d" % logn, m.uniform(n, 0x80 + logn), m.uniform(2 * n, 0x90 + logn), reach=reach)


def msm_rare():
    """reduce_forms_child.rare's inputs (one occupied bucket, equal and opposite sums, the largest digits: ragged last chunk)
    under this process's ARK_HIP_MSM_L0 / ARK_HIP_MSM_STAGE2: every input warm and poisoned, then every input poisoned again
    after a larger MSM."""
    import reduce_forms_child as RF
    plain = RF.run_device
    state = {"pass": 1, "count": 0}

    def wrapped(cid, bases_t, idx, vals, r):
        if state["pass"] == 1 and not plain(cid, bases_t, idx, vals, r):
            return False
        poison()
        ok = plain(cid, bases_t, idx, vals, r)
        assert_clean(("rare", cv.curve_name(cid), state["pass"], state["count"]))
        state["count"] += 1
        return ok

    prove_one_instance(Msm(O.CID["BLS12_381_G1"], 1 << 10))
    RF.run_device = wrapped
    RF.rare()
    first = state["count"]
    for cname in ("BLS12_381_G1", "BLS12_377_G2"):     # the growers: a larger MSM on each curve of the list
        assert Msm(O.CID[cname], 1 << 14).uniform(1 << 14, 0xA1)()
    state["pass"] = 2
    RF.rare()
    assert first >= 12 and state["count"] == 2 * first, state
    print("ok rare x", first, flush=True)


# ---- FFT ---------------------------------------------------------------------------------------------------------------
def fft_field(fname):
    fid = O.FID[fname]
    gen = O.field_const(fid, 3)

    def rand(n, seed):
        return O.gen_scalars(fid, seed, max(n, 1), montgomery=True)[:n]

    def dev(x):
        d = torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
        torch.cuda.synchronize()
        return d

    def back(t):
        return t.cpu().numpy().view(np.uint64).reshape(-1)

    def transform(log_n, coset, inverse, seed, host=False):
        n = 1 << log_n
        x = rand(n, seed)
        d = A.Radix2EvaluationDomain.new(fname, n)
        d = d.get_coset(gen) if coset else d
        want = O.fft(fid, x, log_n, gen if coset else None, inverse, 4)
        dx = x if host else dev(x)

        def run():
            y = (d.ifft if inverse else d.fft)(dx)
            return np.array_equal(y.reshape(-1) if host else back(y), want)
        return run

    prove_one_instance(Msm(O.CID["BLS12_381_G1"], 1 << 10))
    big = transform(16, True, False, 0x16)
    protocol("%s fft 2^10" % fname, transform(10, False, False, 2), big)
    protocol("%s coset fft 2^10" % fname, transform(10, True, False, 3), big)
    protocol("%s coset ifft 2^10" % fname, transform(10, True, True, 4), transform(16, True, True, 0x17))
    protocol("%s host fft 2^10" % fname, transform(10, False, False, 5, host=True), transform(16, False, False, 0x18, host=True),
             reach=("stage_a",))
    protocol("%s host coset ifft 2^12" % fname, transform(12, True, True, 6, host=True), transform(16, True, True, 0x19, host=True))

    # degree-aware: 5 coefficients on a domain of 2^12
    def degree_aware(log_n, rows, seed):
        x = rand(rows, seed)
        d = A.Radix2EvaluationDomain.new(fname, 1 << log_n)
        full = np.zeros((1 << log_n, 4), dtype=np.uint64)
        full[:rows] = x
        want = O.fft(fid, full, log_n, None, False, 4)
        dx = dev(x)
        return lambda: np.array_equal(back(d.fft(dx)), want)
    protocol("%s degree-aware 5 of 2^12" % fname, degree_aware(12, 5, 7), degree_aware(16, 9, 8))

    # a batch of 3: one ping buffer per stream
    def batch(log_n, seed):
        n = 1 << log_n
        xs = [rand(n, seed + j) for j in range(3)]
        d = A.Radix2EvaluationDomain.new(fname, n)
        wants = [O.fft(fid, x, log_n, None, False, 4) for x in xs]

        def run():
            ts = [dev(x) for x in xs]
            d.fft_batch_in_place(ts)
            return all(np.array_equal(back(t), w) for t, w in zip(ts, wants))
        return run
    protocol("%s batch of 3 at 2^12" % fname, batch(12, 0x30), batch(16, 0x40))

    # poly_mul 300 x 70 after 5000 x 5000: the expected product through the oracle's transforms on a domain that holds it
    def poly_mul(la, lb, seed):
        a, b = rand(la, seed), rand(lb, seed + 1)
        log_n = (la + lb - 2).bit_length()
        n = 1 << log_n
        pad = lambda v: np.concatenate([v, np.zeros((n - v.shape[0], 4), dtype=np.uint64)])   # noqa: E731
        fa, fb = O.fft(fid, pad(a), log_n, None, False, 4), O.fft(fid, pad(b), log_n, None, False, 4)
        want = O.fft(fid, O.field_op(fid, "mul", fa, fb.reshape(-1, 4)), log_n, None, True, 4).reshape(n, 4)[: la + lb - 1]
        return lambda: np.array_equal(A.poly_mul_host(fname, a, b), want)
    protocol("%s poly_mul 300 x 70" % fname, poly_mul(300, 70, 0x50), poly_mul(5000, 5000, 0x60), reach=("stage_a", "stage_b"))

    # the smallest size of the two- and of the three-pass plan (pyref.fft_plan restates the device planner): the ping buffer.
    # (The four-pass plan starts at 2^25: 1 GiB of data and an oracle transform of minutes -- not a test of seconds.)
    import pyref
    for passes in (2, 3):
        k = min(k for k in range(1, 25) if len(pyref.fft_plan(k)) == passes)
        protocol("%s fft 2^%d, the smallest %d-pass plan" % (fname, k, passes), transform(k, False, False, 0x70 + k),
                 transform(k + 1, False, False, 0x80 + k), reach=("fft.tmps*",))

    # fft_axis with G = 4: out[j][c] = sum_i root^(i j) in[i][c] along the slow axis of a [4][cols] device array
    p = pyref.MODULI[fname][0]
    root = O.domain(fid, 2)[0]
    rc = pyref.from_mont(root, p)

    def axis(cols, seed, checked=True):
        import mle_ref
        x = rand(4 * cols, seed)
        if checked:
            xi = mle_ref.ints(x)
            want = mle_ref.limbs([sum(pow(rc, i * j, p) * xi[i * cols + c] for i in range(4)) % p for j in range(4) for c in range(cols)])

        def run():
            t = dev(x)
            _lib.check(T.ark_hip_fft_axis_device(fid, t.data_ptr(), 4, cols, root.ctypes.data_as(C.c_void_p)), "ark_hip_fft_axis_device")
            _lib.check(T.ark_hip_synchronize(), "ark_hip_synchronize")
            return not checked or np.array_equal(back(t).reshape(-1, 4), want)
        return run
    protocol("%s fft_axis G = 4, 300 columns" % fname, axis(300, 0x91), axis(5000, 0x92, checked=False))


# ---- polynomial ops, MLE ---------------------------------------------------------------------------------------------------
def poly():
    """BLS12-381 Fr: evaluate and divide-by-linear at T + 1 and 65 after T^2 + 1 (three scan levels: poly_work), the inner product
    at 4097 after 2^20, the Lagrange coefficients at 2^10 after 2^14, MLE evaluate and fix_variables at 2^9 after 2^16.  The
    expected values are Python integers (Montgomery residues a R used as they are with the point in canonical form: the
    recurrences are linear in the coefficients); the growers only grow."""
    import mle_ref
    import pyref
    fname = "BLS12_381_FR"
    fid, p = O.FID[fname], pyref.MODULI[fname][0]
    rinv = pow(pyref.R_of(p), -1, p)
    prove_one_instance(Msm(O.CID["BLS12_381_G1"], 1 << 10))
    t, lv = C.c_int(), C.c_int()
    assert T.ark_hip_poly_scan_plan(0, C.byref(t), C.byref(lv)) == 0
    tile = t.value
    assert T.ark_hip_poly_scan_plan(tile * tile + 1, C.byref(t), C.byref(lv)) == 0 and lv.value == 3

    def rand(n, seed):
        return O.gen_scalars(fid, seed, max(n, 1), montgomery=True)[:n]

    z = rand(1, 9)[0]
    zc = pyref.from_mont(z, p)

    def eval_divide(n, seed, checked=True):
        a = rand(n, seed)
        dp = A.DeviceVec.from_host(fname, a)
        if checked:
            cm, q_want, acc = mle_ref.ints(a), [0] * (n - 1), 0
            for i in range(n - 1, -1, -1):
                if i < n - 1:
                    q_want[i] = acc
                acc = (cm[i] + zc * acc) % p
            q_want, r_want = mle_ref.limbs(q_want), pyref.to_limbs(acc, 4)

        def run():
            ev = dp.evaluate(z)
            q, rem = dp.divide_by_linear(z)
            got = q.to_host()
            q.free()
            return not checked or (np.array_equal(ev, r_want) and np.array_equal(rem, r_want) and np.array_equal(got, q_want))
        return run
    big = eval_divide(tile * tile + 1, 0x33, checked=False)
    protocol("evaluate and divide by x - z at T + 1", eval_divide(tile + 1, 0x31), big, reach=("poly_work",))
    protocol("evaluate and divide by x - z at 65", eval_divide(65, 0x32), big, reach=("poly_work",))

    def inner(n, seed, checked=True):
        a, b = rand(n, seed), rand(n, seed + 1)
        da, db = A.DeviceVec.from_host(fname, a), A.DeviceVec.from_host(fname, b)
        want = pyref.to_limbs(sum(x * y for x, y in zip(mle_ref.ints(a), mle_ref.ints(b))) * rinv % p, 4) if checked else None
        return lambda: not checked or np.array_equal(da.inner_product(db), want)
    protocol("inner product 4097", inner(4097, 0x41), inner(1 << 20, 0x43, checked=False), reach=("poly_work",))

    def lagrange(log_n, seed, checked=True):
        n = 1 << log_n
        d = A.Radix2EvaluationDomain.new(fname, n)
        tau = rand(1, seed)[0]
        if checked:   # L_i(tau) = (tau^n - 1) g^i / (n (tau - g^i))
            tc, g = pyref.from_mont(tau, p), pyref.from_mont(O.domain(fid, log_n)[0], p)
            zh, gi, want = (pow(tc, n, p) - 1) * pow(n, -1, p) % p, 1, []
            for _ in range(n):
                want.append(zh * gi * pow(tc - gi, -1, p) % p)
                gi = gi * g % p
            want = np.stack([pyref.to_mont(v, p) for v in want])

        def run():
            v = d.evaluate_all_lagrange_coefficients(tau)
            got = v.to_host()
            v.free()
            return not checked or np.array_equal(got, want)
        return run
    protocol("lagrange coefficients 2^10", lagrange(10, 0x51), lagrange(14, 0x52, checked=False))

    def mle(nv, seed, checked=True):
        table = rand(1 << nv, seed)
        point = rand(nv, seed + 1)
        m = A.DenseMultilinearExtension.from_evaluations(fname, nv, table)
        if checked:
            pc = [pyref.from_mont(x, p) for x in point]
            want_ev = pyref.to_limbs(mle_ref.evaluate(mle_ref.ints(table), pc, p), 4)
            want_fix = mle_ref.limbs(mle_ref.fix_variables(mle_ref.ints(table), pc[:3], p))

        def run():
            ev = m.evaluate(point)
            f = m.fix_variables(point[:3])
            got = f.to_evaluations()
            f.free()
            return not checked or (np.array_equal(ev, want_ev) and np.array_equal(np.asarray(got).reshape(-1, 4), want_fix))
        return run
    protocol("mle evaluate and fix_variables 2^9", mle(9, 0x61), mle(16, 0x63, checked=False))


# ---- point arrays -----------------------------------------------------------------------------------------------------------
def points():
    """BLS12-381 G1: sw_mul and fold on device vectors at 65 after 1000, the host-slice sw_mul, the host check at 65 rows with
    the planted bad rows after 1000 and the host decompress likewise (status bytes through stage_b, summary words through
    check_work), normalize_batch and
    batch_mul host entries at 129 after 4097.  P_i = (a + i b) G, so [k] P_i is one oracle multiple of the generator."""
    import check_fixtures as CF
    cname = "BLS12_381_G1"
    cid = O.CID[cname]
    fid = O.curve_info(cid)[1]
    r = S.R[cv.scalar_field(cid)]
    prove_one_instance(Msm(cid, 1 << 10))
    nmax = 4097
    xy = O.gen_bases(cid, S.limbs4(S.A0), S.limbs4(S.B0), nmax)
    assert np.array_equal(xy[2], want_point(cid, S.A0 + 2 * S.B0))
    ks = O.gen_scalars(fid, 0x5EED, nmax)
    kint = [S.scalar_int(row) for row in ks]
    dlog = lambda i: S.A0 + i * S.B0   # noqa: E731
    want_mul = np.stack([want_point(cid, kint[i] * dlog(i) % r) for i in range(129)])

    def affine_of(dev_points):
        got = dev_points.to_host()
        dev_points.free()
        return O.to_affine(cid, got)

    def sw_mul(n, checked=True):
        v = A.DevicePoints.from_host(cid, xy[:n])
        return lambda: (lambda got: not checked or np.array_equal(got, want_mul[:n]))(affine_of(v.mul(ks[:n], montgomery=False)))
    protocol("sw_mul 65", sw_mul(65), sw_mul(1000, checked=False), reach=("pointvec_work",))

    def fold(n, checked=True):
        lo, hi = A.DevicePoints.from_host(cid, xy[:n]), A.DevicePoints.from_host(cid, xy[n:2 * n])
        a, b = kint[0], kint[1]
        want = np.stack([want_point(cid, (a * dlog(i) + b * dlog(n + i)) % r) for i in range(n)]) if checked else None
        return lambda: (lambda got: not checked or np.array_equal(got, want))(affine_of(lo.fold(hi, ks[0], ks[1], montgomery=False)))
    protocol("fold 65", fold(65), fold(1000, checked=False), reach=("pointvec_work",))

    def sw_mul_host(n, checked=True):
        def run():
            out = np.zeros((n, 3 * O.fe_words(cid)), dtype=np.uint64)
            _lib.check(T.ark_hip_sw_mul(cid, xy[:n].ctypes.data_as(C.c_void_p), 0, ks[:n].ctypes.data_as(C.c_void_p), n, 0, n,
                                        out.ctypes.data_as(C.c_void_p)), "ark_hip_sw_mul")
            return not checked or np.array_equal(O.to_affine(cid, out), want_mul[:n])
        return run
    protocol("host-slice sw_mul 65", sw_mul_host(65), sw_mul_host(1000, checked=False), reach=("stage_a", "stage_b", "stage_c"))

    def check_host(n):
        rows, where = CF.plant(cname, n, CF.bad_rows(cname))
        st, summary = CF.expected(cname, rows, where, 3)

        def run():
            got = A.check_bases(cid, rows, return_status=True)
            return (np.array_equal(got.status, st) and [got.first_bad, got.not_reduced, got.off_curve, got.off_subgroup] == summary
                    and not got.ok)
        return run
    protocol("host check 65 with planted bad rows", check_host(65), check_host(1000), reach=("stage_a", "stage_b", "check_work"))

    import compress_fixtures as X

    def decompress_host(n):
        rows, where = X.plant(cname, n, X.bad_rows(cname, True))
        want_pts, want_st, want = X.expected(cname, rows, where, True)

        def run():
            pts, res = A.decompress_bases(cid, rows, validate=True, return_status=True)
            return (np.array_equal(pts, want_pts) and np.array_equal(res.status, want_st) and not res.ok
                    and [res.first_bad, res.bad_flags, res.not_reduced, res.no_root, res.off_subgroup] == want)
        return run
    protocol("host decompress 65 with planted bad rows", decompress_host(65), decompress_host(1000),
             reach=("stage_a", "stage_b", "stage_c", "check_work"))

    jac = A.DevicePoints.from_host(cid, xy[:nmax]).mul(ks[:nmax], montgomery=False).to_host()   # inputs with z != 1
    want_norm = O.to_affine(cid, jac[:129])

    def normalize(n, checked=True):
        return lambda: (lambda got: not checked or np.array_equal(got, want_norm[:n]))(A.normalize_batch(cid, jac[:n]))
    protocol("normalize_batch host 129", normalize(129), normalize(4097, checked=False), reach=("stage_a", "stage_b"))

    base = O.scalar_mul(cid, O.generator(cid), S.limbs4(7))
    want_bm = O.batch_mul(cid, base, ks[:129])

    def batch_mul(n, checked=True):
        return lambda: (lambda got: not checked or np.array_equal(got, want_bm[:n]))(A.batch_mul(cid, base, ks[:n], montgomery=False))
    protocol("batch_mul host 129", batch_mul(129), batch_mul(4097, checked=False))


# ---- transform over group elements -----------------------------------------------------------------------------------------
def gfft(log_n, log_big):
    """BLS12-381 G1, host entry: the coset inverse transform of P_i = [a + i b] G (one identity) is [IFFT_F(a + i b)_j] G -- the
    oracle's field transform and scalar multiplications; after a transform of 2^log_big points"""
    cname = "BLS12_381_G1"
    cid = O.CID[cname]
    bf, sf, _ = O.curve_info(cid)
    fw = O.fe_words(cid)
    r = S.R[cv.scalar_field(cid)]
    fname = cv.scalar_field(cid)
    prove_one_instance(Msm(cid, 1 << 10))
    gen = O.field_const(sf, 3)

    def case(k, checked=True):
        n = 1 << k
        pts = np.zeros((n, 3 * fw), dtype=np.uint64)
        pts[:, :2 * fw] = O.gen_bases(cid, S.limbs4(S.A0), S.limbs4(S.B0), n)
        one = O.field_const(bf, 1)
        pts[:, 2 * fw:2 * fw + one.size] = one
        scal = [(S.A0 + i * S.B0) % r for i in range(n)]
        pts[n - 1], scal[n - 1] = 0, 0
        d = A.Radix2EvaluationDomain.new(fname, n).get_coset(gen)
        if checked:
            mont = O.field_op(sf, "from_bigint", to_limbs(scal)).reshape(n, 4)
            canon = O.field_op(sf, "into_bigint", O.fft(sf, mont, k, gen, True, 2)).reshape(n, 4)
            want = np.stack([O.to_affine(cid, O.scalar_mul(cid, O.generator(cid), canon[j])) for j in range(n)])
        return lambda: (lambda got: not checked or np.array_equal(A.into_affine(cid, got), want))(d.fft_group_in_place(cname, pts.copy(), inverse=True))
    protocol("group coset ifft 2^%d" % log_n, case(log_n), case(log_big, checked=False), reach=("stage_a", "gfft_work", "gfft_scal"))


def points_slab():
    """sw_mul at 1000 with the smallest slab (ARK_HIP_POINTVEC_SLAB_LOG=6 in the environment): several launches share the tables"""
    cid = O.CID["BLS12_381_G1"]
    r = S.R[cv.scalar_field(cid)]
    assert os.environ.get("ARK_HIP_POINTVEC_SLAB_LOG") == "6"
    prove_one_instance(Msm(cid, 1 << 10))
    xy = O.gen_bases(cid, S.limbs4(S.A0), S.limbs4(S.B0), 2000)
    ks = O.gen_scalars(O.curve_info(cid)[1], 0x5EED, 2000)
    want = np.stack([want_point(cid, S.scalar_int(ks[i]) * (S.A0 + i * S.B0) % r) for i in range(1000)])

    def sw_mul(n, checked=True):
        v = A.DevicePoints.from_host(cid, xy[:n])

        def run():
            out = v.mul(ks[:n], montgomery=False)
            got = out.to_host()
            out.free()
            return not checked or np.array_equal(O.to_affine(cid, got), want[:n])
        return run
    protocol("sw_mul 1000 in slabs of 64 lanes", sw_mul(1000), sw_mul(2000, checked=False), reach=("pointvec_work",))


def selfcheck():
    """the harness fails when it should: an unwritten poisoned cell reads back as the poison, and four bytes planted in one
    buffer's slack (in bounds) are reported as exactly that -- no product kernel runs"""
    rc = T.ark_hip_test_scratch_selfcheck()
    assert rc == 0, ("ark_hip_test_scratch_selfcheck: failing step", rc)
    rows = report()
    dirty = {k: (r.dirty_beyond, r.first_dirty_offset, r.asked) for k, r in rows.items() if r.dirty_beyond}
    assert dirty == {"stage_c": (4, 1024 + 8, 1024)}, dirty
    assert not any(r.regrown for r in rows.values())
    try:
        assert_clean("selfcheck")
    except AssertionError:
        print("ok selfcheck: the planted overrun fails assert_clean", flush=True)
    else:
        raise AssertionError("assert_clean passed a planted overrun")
    poison()
    assert_clean("selfcheck, poisoned again")
    print("ok selfcheck", flush=True)


MODES = {
    "selfcheck": selfcheck,
    "msm_bls12_381_g1": lambda: msm_curve("BLS12_381_G1"),
    "msm_bn254_g1": lambda: msm_curve("BN254_G1"),
    "msm_bls12_377_g2": lambda: msm_curve("BLS12_377_G2"),
    "msm_large": msm_large,
    "msm_entries": msm_entries,
    "msm_rare": msm_rare,
    "msm_groups": lambda: msm_knob(19, "msm0.keys"),
    "msm_run_parts": lambda: msm_knob(16, "msm0.parts"),
    "msm_saturated": lambda: msm_knob(12, "msm0.keys"),
    "poly": poly,
    "points": points,
    "points_slab": points_slab,
    "gfft": lambda: gfft(5, 8),
    "gfft_slab": lambda: gfft(8, 9),
    "fft_bn254_fr": lambda: fft_field("BN254_FR"),
    "fft_bls12_381_fr": lambda: fft_field("BLS12_381_FR"),
    "fft_bls12_377_fr": lambda: fft_field("BLS12_377_FR"),
}

if __name__ == "__main__":
    MODES[sys.argv[1]]()
    print("scratch-reuse ok", sys.argv[1], flush=True)
