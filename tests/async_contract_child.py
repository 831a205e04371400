"""Child process of tests/test_gpu_async_contract.py: the cases of tests/async_cases.py behind a busy context stream.

    ARK_HIP_LIB=algebra_amd/libark_hip_test.so python tests/async_contract_child.py <group>      (A:<cases' group>, B, C or D)

The blocker: one asynchronous MSM of 2^BLOCKER_LOG BLS12-381 G1 points against a prepared base set, on lane 0 -- which is the
context stream.  Size: MEASURED 2^12 -- in three whole passes of the suite on an MI355X every case of every group was
conclusive (the blocker still running once the host side of the case was done) at 2^12, which is also the smallest set the
consumer of part A fits in (it takes up to 4096 scalars against the same prepared set), so nothing smaller can be tried;
single passes at 2^14, 2^16 and 2^18 were conclusive as well.  SHIPPED four times that, 2^14 (the margin is for host latency
on a shared machine).  ASYNC_CONTRACT_BLOCKER_LOG (12 .. 20) overrides it, for measuring only.

The arrangement of every case:
  1. upload the inputs, wait;  2. warm the call with the same shapes and constants (table builds and scratch growth
  synchronise: they must happen here);  3. restore the inputs, fill the outputs with their stale content;  4. enqueue the
  blocker;  5. make the call under test and do the part's host-side work;  6. ark_hip_test_context_busy: a case whose blocker
  has already finished is INCONCLUSIVE and fails;  7. wait, compare limb for limb with the reference.
Part A: the output goes straight to an MSM that must land on lane 1 and still see the result (the first case is the negative
control: with the producer marks off it must see the STALE vector).  Part B: every host argument is overwritten with other
valid values as soon as the call has returned, once in pageable and once in page-locked memory.  Part C: two calls with
different constants and nothing in between.  Part D: the waiting form -- the host value is compared AT RETURN; a call that
waits drains the context stream, so there the blocker is checked to be running right BEFORE the call.
A wrong result is counted and the child goes on; a HIP error code from any call ends the child there."""
import ctypes as C
import hashlib
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
import synth
import async_cases as AC
from algebra_amd import _lib
from algebra_amd import curves as cv

assert os.path.realpath(_lib.LIB_PATH) == os.path.realpath(_lib.TEST_LIB_PATH), "run with ARK_HIP_LIB=libark_hip_test.so"
T = _lib.test_lib()
L = _lib.lib()
assert T._handle == L._handle, "the mirror and the hooks must be one library instance"

BLOCKER_LOG = int(os.environ.get("ASYNC_CONTRACT_BLOCKER_LOG", "14"))
assert 12 <= BLOCKER_LOG <= 20, "the prepared set must hold the consumer's 2^12 scalars; the cap is 2^20"
vp = C.c_void_p
A4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)        # the bases P_i = (A0 + i B0) G of tools/synth.py, as oracle limbs
B4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)
SENTINEL = 0xA5
FAILURES = []


def ok(rc, what):
    if rc != 0:
        print("%s failed with code %d: the child stops here" % (what, rc), flush=True)
        raise SystemExit(3)


def busy():
    b = C.c_int(-1)
    ok(T.ark_hip_test_context_busy(C.byref(b)), "ark_hip_test_context_busy")
    return b.value == 1


def sync():
    ok(L.ark_hip_synchronize(), "ark_hip_synchronize")


def fail(case, what):
    FAILURES.append("%s: %s" % (case, what))
    print("FAIL", case, what, flush=True)


class Lane:
    """the prepared base set of one curve, the blocker's scalars, and the oracle's points of Fr vectors against it"""

    def __init__(self, fname):
        self.cname = AC.CURVE_OF[fname]
        self.cid = O.CID[self.cname]
        nb = 1 << BLOCKER_LOG
        r = synth.R[fname]
        bases = synth.grow_bases(self.cid, nb, synth.A0, synth.B0, r)
        self.pb = A.PreparedBases(self.cid, bases)
        del bases
        self.host_bases = O.gen_bases(self.cid, A4, B4, AC.N)
        self.other = torch.from_numpy(synth.gen_scalars(nb, 2, r).view(np.int64)).cuda()
        torch.cuda.synchronize()
        self.nb = nb
        self.points = {}
        ok(L.ark_hip_msm_prepared_device(self.pb._h, self.other.data_ptr(), nb, 0, np.zeros(18, dtype=np.uint64).ctypes.data_as(vp)),
           "blocker warm-up")                        # lane 0's workspace at its size
        j0 = self.blocker()                          # and lane 1's, at the largest consumer's: allocations happen here
        j1 = self.consumer(self.other.data_ptr(), AC.N)
        self.wait(j1)
        self.wait(j0)

    def blocker(self):
        h = vp()
        ok(L.ark_hip_msm_prepared_device_async(self.pb._h, self.other.data_ptr(), self.nb, 0, C.byref(h)), "the blocker")
        return h

    def consumer(self, addr, n):
        h = vp()
        ok(L.ark_hip_msm_prepared_device_async(self.pb._h, vp(addr), n, 1, C.byref(h)), "the consumer")
        return h

    def wait(self, h):
        out = np.zeros(cv.projective_words(self.cid), dtype=np.uint64)
        ok(L.ark_hip_msm_wait(h, out.ctypes.data_as(vp)), "ark_hip_msm_wait")
        return np.asarray(A.into_affine(self.cid, out)).reshape(-1)

    def oracle(self, scalars):
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        key = hashlib.sha256(s.tobytes()).digest()
        if key not in self.points:
            self.points[key] = O.to_affine(self.cid, O.msm(self.cid, self.host_bases[:s.shape[0]], s, O.SIGNED, 4, True)).reshape(-1)
        return self.points[key]


LANES = {}


def lane(fname):
    if fname not in LANES:
        LANES[fname] = Lane(fname)
    return LANES[fname]


class Run:
    """one case on the device: its buffers, its host arguments (pageable numpy, or page-locked from ark_hip_host_alloc), its handle"""

    def __init__(self, built, extra=(), pinned=False):
        self.b, self.pinned = built, pinned
        self.dev, self.d, self.h, self.locked = {}, {}, {}, []
        for src in (built,) + tuple(extra):
            for name, arr in src.dev.items():
                if name in self.dev:
                    assert name in src.outs or np.array_equal(self.dev[name], arr), name
                    continue
                self.dev[name] = np.ascontiguousarray(arr)
                p = vp(0)
                ok(L.ark_hip_malloc(max(self.dev[name].nbytes, 32), C.byref(p)), "ark_hip_malloc")
                self.d[name] = p.value
        for name in list(built.host) + list(built.ptrs):
            nbytes = built.host[name].nbytes if name in built.host else 8 * len(built.ptrs[name])
            dtype = built.host[name].dtype if name in built.host else np.uint64
            self.h[name] = self.host_array(nbytes, dtype)
        self.handle, self.drop = built.handle(L) if built.handle else (None, None)
        self.restore()

    def host_array(self, nbytes, dtype):
        if not self.pinned:
            return np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        p = vp(0)
        ok(L.ark_hip_host_alloc(max(nbytes, 8), C.byref(p)), "ark_hip_host_alloc")
        self.locked.append(p)
        return np.frombuffer((C.c_char * nbytes).from_address(p.value), dtype=dtype)

    def upload(self, name):
        a = self.dev[name]
        ok(L.ark_hip_memcpy_h2d(vp(self.d[name]), a.ctypes.data_as(vp), a.nbytes), "ark_hip_memcpy_h2d")

    def set_host(self, built):
        """the host arguments as `built` has them (the pointer arrays resolved against this run's device buffers)"""
        for name, arr in built.host.items():
            self.h[name].reshape(-1)[:] = np.ascontiguousarray(arr).reshape(-1)
        for name, names in built.ptrs.items():
            self.h[name][:] = np.array([self.d[k] for k in names], dtype=np.uint64)

    def restore(self):
        for name in self.dev:
            self.upload(name)                          # synchronous copies: the inputs and the stale outputs are in place
        self.set_host(self.b)

    def args(self, wait=None, **over):
        a = dict(self.d)
        a.update({k: v.ctypes.data for k, v in self.h.items()})
        a["wait"] = wait
        a["handle"] = self.handle
        a.update(over)
        return a

    def download(self, name):
        out = np.empty(self.dev[name].nbytes, dtype=np.uint8)
        ok(L.ark_hip_memcpy_d2h(out.ctypes.data_as(vp), vp(self.d[name]), out.nbytes), "ark_hip_memcpy_d2h")
        return out

    def outputs_match(self, case, built=None, rename=None):
        """every output limb for limb against the reference (the whole buffer: what the call does not write stays as it was)"""
        built = built or self.b
        good = True
        for o in built.outs:
            got, want = self.download((rename or {}).get(o, o)), built.expected(o)
            if built.compare:
                same = np.array_equal(built.compare(got.view(np.uint64)), built.compare(want.view(np.uint64)))
            else:
                same = np.array_equal(got, want)
            if not same:
                bad = np.nonzero(got != want)[0]
                stale_back = np.array_equal(got, np.ascontiguousarray(built.dev[o]).reshape(-1).view(np.uint8))
                fail(case, "output %s differs from the reference%s" % (o, " (it still holds the stale content)" if stale_back else
                                                                       " (first byte %d of %d)" % (bad[0] if bad.size else -1, got.size)))
                good = False
        return good

    def free(self):
        sync()
        if self.drop:
            ok(self.drop(), "the handle's free")
        for p in self.d.values():
            ok(L.ark_hip_free(vp(p)), "ark_hip_free")
        for p in self.locked:
            ok(L.ark_hip_host_free(p), "ark_hip_host_free")


def call(built, run, what, **kw):
    ok(built.call(L, run.args(**kw)), what)


# ---- part A -------------------------------------------------------------------------------------------------------------------
def part_a(case, control=False):
    name = "A%s %s" % (" negative control" if control else "", case.name)
    b = case.make(0)
    ln = lane(case.fname)
    run = Run(b)
    out, off, count = b.consume
    seg = slice(32 * off, 32 * (off + count))
    s_stale = np.ascontiguousarray(b.dev[out]).reshape(-1).view(np.uint8)[seg].view(np.uint64)
    s_right = b.expected(out)[seg].view(np.uint64)
    p_stale, p_right = ln.oracle(s_stale), ln.oracle(s_right)
    assert not np.array_equal(p_stale, p_right), (name, "the stale point and the right point must differ")
    addr = run.d[out] + 32 * off
    call(b, run, case.entry + " (warm-up)")
    ln.wait(ln.consumer(addr, count))
    sync()
    run.restore()
    j0 = ln.blocker()
    if control:
        ok(T.ark_hip_test_producer_marks(0), "ark_hip_test_producer_marks")
    call(b, run, case.entry)
    j1 = ln.consumer(addr, count)
    if control:
        ok(T.ark_hip_test_producer_marks(1), "ark_hip_test_producer_marks")
    which = C.c_int(-1)
    ok(T.ark_hip_test_job_lane(j1, C.byref(which)), "ark_hip_test_job_lane")
    was_busy = busy()
    got = ln.wait(j1)
    ln.wait(j0)
    sync()
    verdict = "the right point" if np.array_equal(got, p_right) else "the STALE point" if np.array_equal(got, p_stale) else "neither point"
    if which.value != 1:
        fail(name, "the consumer ran on lane %d, not on the second lane" % which.value)
    elif not was_busy:
        fail(name, "inconclusive: the blocker had finished before the host side of the case was done")
    elif control:
        if verdict != "the STALE point":
            fail(name, "the consumer saw %s with the producer marks off: the two streams were serialised here and part A "
                 "proves nothing on this machine" % verdict)
    elif verdict != "the right point":
        fail(name, "the MSM on the second lane returned %s" % verdict)
    run.outputs_match(name)
    run.free()


def group_a(group):
    cases = AC.cases_of("A", group)
    first = [c for c in AC.CASES if c.name == "add %s:%d" % (AC.FR, AC.N)][0]
    part_a(first, control=True)
    if FAILURES:
        return 1                                    # without a control that shows the stale point the rest proves nothing
    for c in cases:
        part_a(c)
    return len(cases) + 1


# ---- part B -------------------------------------------------------------------------------------------------------------------
def part_b(case, pinned):
    name = "B %s (%s host memory)" % (case.name, "page-locked" if pinned else "pageable")
    b, alt = case.make(0), case.make("B")
    ln = lane(AC.FR)
    run = Run(b, extra=(alt,), pinned=pinned)
    call(b, run, case.entry + " (warm-up)")
    sync()
    run.restore()
    j0 = ln.blocker()
    call(b, run, case.entry)
    run.set_host(alt)                               # the host arguments die: other valid values of the same shapes
    was_busy = busy()
    ln.wait(j0)
    sync()
    if not was_busy:
        fail(name, "inconclusive: the blocker had finished before the host side of the case was done")
    run.outputs_match(name)
    run.free()


def group_b():
    cases = AC.cases_of("B")
    for c in cases:
        for pinned in (False, True):
            part_b(c, pinned)
    return 2 * len(cases)


# ---- part C -------------------------------------------------------------------------------------------------------------------
def part_c(case):
    name = "C " + case.name
    b1, b2 = case.make(0), case.make("C")
    ln = lane(AC.FR)
    run1 = Run(b1)
    run2 = Run(b2)                                   # its own host arguments and its own outputs
    for b, run in ((b1, run1), (b2, run2)):          # both warmed: both constants' tables are built
        call(b, run, case.entry + " (warm-up)")
    sync()
    run1.restore()
    run2.restore()
    j0 = ln.blocker()
    call(b1, run1, case.entry + " (first call)")
    call(b2, run2, case.entry + " (second call)")
    was_busy = busy()
    ln.wait(j0)
    sync()
    if not was_busy:
        fail(name, "inconclusive: the blocker had finished before the host side of the case was done")
    run1.outputs_match(name + ", first call")
    run2.outputs_match(name + ", second call")
    run1.free()
    run2.free()


def group_c():
    cases = AC.cases_of("C")
    for c in cases:
        part_c(c)
    return len(cases)


# ---- part D -------------------------------------------------------------------------------------------------------------------
def part_d(case):
    name = "D " + case.name
    b = case.make(0)
    ln = lane(AC.FR)
    run = Run(b)
    nbytes, want = b.wait[0], b.wait[1]()
    host = np.full(nbytes, SENTINEL, dtype=np.uint8)
    call(b, run, case.entry + " (warm-up)", wait=host.ctypes.data)
    sync()
    run.restore()
    host[:] = SENTINEL
    assert host.tobytes() != want, name
    a = run.args(wait=host.ctypes.data)
    j0 = ln.blocker()
    was_busy = busy()                                # a call that waits drains the stream: the blocker must be running NOW
    rc = b.call(L, a)
    at_return = host.tobytes()                       # before any other library call
    ok(rc, case.entry)
    ln.wait(j0)
    sync()
    if not was_busy:
        fail(name, "inconclusive: the blocker had finished before the call was made")
    if at_return != want:
        fail(name, "the host result at return is %s" % ("still the sentinel: the call did not wait for it"
                                                        if at_return == bytes([SENTINEL]) * nbytes else "not the reference's"))
    run.outputs_match(name)
    run.free()


def group_d():
    cases = AC.cases_of("D")
    for c in cases:
        part_d(c)
    return len(cases)


def main():
    group = sys.argv[1]
    if group.startswith("A:"):
        ran = group_a(group[2:])
    else:
        ran = {"B": group_b, "C": group_c, "D": group_d}[group]()
    sync()
    for ln in LANES.values():
        ln.pb.free()
    print("async contract %s: %d cases, %d failed, blocker 2^%d" % (group, ran, len(FAILURES), BLOCKER_LOG), flush=True)
    for f in FAILURES:
        print("  " + f, flush=True)
    return 1 if FAILURES else 0


if __name__ == "__main__":
    sys.exit(main())
