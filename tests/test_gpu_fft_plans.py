"""Radix-2 FFT parity over every pass plan the device planner builds (csrc/fft.cuh, fft_run_device), up to each field's
two-adicity.  Every transform runs with the per-pass timing on and asserts the pass count the plan should have
(pyref.fft_plan, pinned in tests/test_fft_plans_host.py).  Every forced plan and knob case is chosen so that its pass
count differs from the default plan's, so a knob the planner silently drops cannot pass on the default plan.  (The timing
reports how many passes ran, not their stage counts: a plan of the same length in another order is not told apart.)

  * Three-pass plans and the two-pass 2^15 -- random input, every output limb for limb against the oracle: forward and
    coset forward; inverse and coset inverse exactly on the oracle's own outputs (they must give the input back);
    degree-aware lengths that leave one, two or three executed passes.
  * Four-pass plans (2^25 .. 2^28) against the closed form of a geometric input (pyref.geometric_fft) at sampled indices:
    the input is built on the device by doubling and only the sampled outputs are read back.
  * The per-call knobs (ARK_HIP_FFT_TILE_LOG, _KP, _BALANCED, _PLAN), the knobs read once per process (in a child process),
    the power-table cache's eviction, the batch entry, the carry-free kernel and the sharded decomposition at the new
    plan classes.

To see the file bite: index the two-factor coset tables' high factor with 16 bits in the saturated pass kernel
(`(spos >> PW_LO_BITS) & 0xffff`, and the same for `opos`, in csrc/fft.cuh).  test_four_pass_plans_closed_form then fails at
2^27 and 2^28, where those tables serve multi-pass transforms; the older FFT tests do not notice."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
import oracle_lib as O
import pyref as P
from algebra_amd._lib import check, lib

pytestmark = pytest.mark.gpu

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))


# ---- helpers ------------------------------------------------------------------------------------------------------
def planned(k, zlog=0, carry_free=False):
    """the plan pyref.fft_plan expects under the knobs set in this process's environment"""
    e = os.environ
    num = lambda name: int(e[name]) if name in e else None
    plan = [int(v) for v in e["ARK_HIP_FFT_PLAN"].split(",")] if "ARK_HIP_FFT_PLAN" in e else None
    return P.fft_plan(k, zlog, kp=num("ARK_HIP_FFT_KP"), tile_log=num("ARK_HIP_FFT_TILE_LOG"), plan=plan,
                      balanced="ARK_HIP_FFT_BALANCED" in e, ascending=e.get("ARK_HIP_FFT_ASCENDING", "1")[:1] != "0",
                      carry_free=carry_free)


_sentinels = {}


def _sentinel(k, carry_free=False):
    """a small transform whose pass count differs from the one about to be asserted: the count read afterwards is then
    known to come from the transform under test, not from an earlier one"""
    import torch
    if k not in _sentinels:
        _sentinels[k] = (A.Radix2EvaluationDomain.new("BN254_FR", 1 << k),
                         torch.zeros((1 << k, 4), dtype=torch.int64, device="cuda"))
    d, x = _sentinels[k]
    check(lib().ark_hip_fft_in_place_device(d.field, C.byref(d._s), x.data_ptr()), "sentinel fft")
    return len(planned(k, carry_free=carry_free))


def last_npass():
    out = (C.c_double * 10)()
    check(lib().ark_hip_fft_last_timing(out), "fft_last_timing")
    return int(out[1])


@contextlib.contextmanager
def pass_timing():
    check(lib().ark_hip_fft_set_timing(1), "fft_set_timing")
    try:
        yield
    finally:
        check(lib().ark_hip_fft_set_timing(0), "fft_set_timing")


def transform(dom, x, inverse=False, num_coeffs=None, npass=None, carry_free=False):
    """one transform in place on the CUDA tensor x (the library's device entries); asserts the executed pass count
    (default: what the planner restatement gives for this size and these knobs)"""
    import torch
    L = lib()
    k = dom.log_size_of_group()
    zlog = 0 if num_coeffs is None else P.degree_aware_zlog(k, num_coeffs)
    want = len(planned(k, zlog, carry_free)) if npass is None else npass
    torch.cuda.synchronize()
    with pass_timing():
        assert _sentinel(17 if want == 1 else 2, carry_free) != want
        sref = C.byref(dom._s)
        if inverse:
            rc = L.ark_hip_ifft_in_place_device(dom.field, sref, x.data_ptr())
        elif num_coeffs is not None:
            rc = L.ark_hip_fft_in_place_degree_aware_device(dom.field, sref, x.data_ptr(), num_coeffs)
        else:
            rc = L.ark_hip_fft_in_place_device(dom.field, sref, x.data_ptr())
        check(rc, "fft device entry")
        check(L.ark_hip_synchronize(), "synchronize")
        got = last_npass()
    assert got == want, ("executed passes", got, "planned", want, k, zlog)
    return x


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def rand_fr(fid, n, seed):
    return O.gen_scalars(fid, seed, n, montgomery=True)


def coset_gen(fid):
    return O.field_const(fid, 3)


def ints(fname, seed, count=3):
    p = P.MODULI[fname][0]
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(count)]


def geometric_device(fname, log_n, a, b, count=None, out=None):
    """x_i = a b^i (i < count) on the device, doubled up: x[m : 2m] = x[0 : m] * b^m; beyond `count` the buffer holds
    all-ones words (not field elements) that a degree-aware transform must never read"""
    import torch
    fid, p = O.FID[fname], P.MODULI[fname][0]
    n = 1 << log_n
    c = n if count is None else count
    x = out if out is not None else torch.empty((n, 4), dtype=torch.int64, device="cuda")
    if c < n:
        x[c:] = -1
    x[0] = torch.from_numpy(P.to_mont(a, p).view(np.int64))
    torch.cuda.synchronize()
    L = lib()
    m = 1
    while m < c:
        cnt = min(m, c - m)
        bm = P.to_mont(pow(b, m, p), p)
        check(L.ark_hip_fr_scale_device(fid, x.data_ptr(), bm.ctypes.data_as(C.c_void_p), x.data_ptr() + 32 * m, cnt),
              "fr_scale_device")
        m += cnt
    check(L.ark_hip_synchronize(), "synchronize")
    spots = [i for i in (0, 1, 2, 3, c // 2 + 1, c - 1) if i < c]
    got = to_host(x[spots])
    for i, g in zip(spots, got):
        assert P.from_mont(g, p) == a * pow(b, i, p) % p, ("geometric input", i)
    return x


def check_closed_form(fname, log_n, x, a, b, offset=1, inverse=False, num_coeffs=None, seed=0):
    import torch
    p = P.MODULI[fname][0]
    js = P.sample_indices(log_n, extra=300, seed=seed)
    got = to_host(x.index_select(0, torch.from_numpy(js).cuda()))
    exp = P.geometric_fft(fname, log_n, a, b, js, offset, inverse, num_coeffs)
    bad = [int(j) for j, g, e in zip(js, got, exp) if P.from_mont(g, p) != e]
    assert not bad, (fname, log_n, offset != 1, inverse, num_coeffs, "wrong outputs at", bad[:8], len(bad))


def oracle_rounds(fname, log_n, seed, lengths=()):
    """random input, full output against the oracle: forward and coset forward bit-exact; inverse and coset inverse of
    those (oracle-exact) outputs give the input back bit-exact; degree-aware forward of the first `c` coefficients,
    for each c in `lengths`, against the oracle's transform of the zero-extended input"""
    fid = O.FID[fname]
    n = 1 << log_n
    x = rand_fr(fid, n, seed)
    d = A.Radix2EvaluationDomain.new(fname, n)
    g = coset_gen(fid)
    dc = d.get_coset(g)
    for dom, off in ((d, None), (dc, g)):
        y = transform(dom, to_dev(x))
        assert np.array_equal(to_host(y), O.fft(fid, x, log_n, off, False, THREADS).reshape(n, 4)), (fname, log_n, off)
        assert np.array_equal(to_host(transform(dom, y, inverse=True)), x), (fname, log_n, off, "inverse")
        del y
    for c in lengths:
        xz = x.copy()
        xz[c:] = 0
        y = transform(d, to_dev(x), num_coeffs=c)   # the device buffer keeps the random tail: it must not be read
        assert np.array_equal(to_host(y), O.fft(fid, xz, log_n, None, False, THREADS).reshape(n, 4)), (fname, log_n, c)
        del y


def closed_form_rounds(fname, log_n, seed, coset=True, inverse=True, lengths=(), carry_free=False):
    """geometric input, sampled outputs against the closed form: forward, inverse, coset both ways, degree-aware"""
    import torch
    a, b, h = ints(fname, seed)
    p = P.MODULI[fname][0]
    n = 1 << log_n
    d = A.Radix2EvaluationDomain.new(fname, n)
    dc = d.get_coset(P.to_mont(h, p)) if coset else None
    x = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    try:
        for dom, off in ((d, 1), (dc, h)) if coset else ((d, 1),):
            for inv in (False, True) if inverse else (False,):
                geometric_device(fname, log_n, a, b, out=x)
                transform(dom, x, inverse=inv, carry_free=carry_free)
                check_closed_form(fname, log_n, x, a, b, off, inv, seed=seed)
        for c, off in lengths:
            dom = d if off == 1 else d.get_coset(P.to_mont(off, p))
            geometric_device(fname, log_n, a, b, count=c, out=x)
            transform(dom, x, num_coeffs=c, carry_free=carry_free)
            check_closed_form(fname, log_n, x, a, b, off, num_coeffs=c, seed=seed)
    finally:
        del x
        torch.cuda.empty_cache()


# ---- 2. default planner: three-pass plans and 2^15 against the oracle ----------------------------------------------
# degree-aware lengths: n >> zlog - 3 (the library zero-fills up to n >> zlog); the zlogs leave 1, 2 or 3 executed passes
@pytest.mark.parametrize("fname,log_n,lengths", [
    ("BLS12_381_FR", 15, [(1 << 8) - 3, (1 << 13) - 3]),             # (7, 8); kx = 8: one pass into the ping buffer
    ("BN254_FR", 18, [(1 << 8) - 3, (1 << 16) - 3]),                 # (6, 6, 6); kx = 8 / 16
    ("BN254_FR", 21, [(1 << 8) - 3, (1 << 15) - 3, (1 << 17) - 3]),  # (6, 7, 8): sorted from 8, 7, 6
    ("BLS12_381_FR", 21, [(1 << 9) - 3]),
    ("BLS12_377_FR", 21, [(1 << 19) - 3]),
    ("BLS12_377_FR", 23, [(1 << 15) - 3]),                           # (7, 8, 8); kx = 15
    ("BLS12_381_FR", 24, [(1 << 8) - 3]),                            # (8, 8, 8); kx = 8
])
def test_default_plans_against_oracle(fname, log_n, lengths):
    oracle_rounds(fname, log_n, 1500 + log_n, lengths)


@pytest.mark.parametrize("fname,log_n", [("BLS12_377_FR", 11), ("BN254_FR", 13), ("BLS12_381_FR", 14),
                                         ("BLS12_377_FR", 16), ("BLS12_381_FR", 17), ("BN254_FR", 19),
                                         ("BLS12_377_FR", 20), ("BN254_FR", 22)])
def test_remaining_default_plans_against_oracle(fname, log_n):
    # with the sizes above and below, every default plan from 2^11 to 2^28 runs with its pass count asserted
    oracle_rounds(fname, log_n, 1600 + log_n)


@pytest.mark.parametrize("fname,log_n,lengths", [
    ("BLS12_377_FR", 23, [((1 << 21) - 3, 1)]),
    ("BLS12_381_FR", 24, [((1 << 21) - 3, 1), ((1 << 15) - 3, 5)]),   # kx = 21 (three passes), 15 (two), coset
])
def test_default_plans_degree_aware_closed_form(fname, log_n, lengths):
    closed_form_rounds(fname, log_n, 2400 + log_n, coset=False, inverse=False, lengths=lengths)


# ---- 3. four-pass plans and the two-adicity edge against the closed form ------------------------------------------
@pytest.mark.parametrize("fname,log_n,lengths", [
    ("BLS12_381_FR", 25, []),
    ("BLS12_377_FR", 25, []),
    ("BLS12_381_FR", 26, [((1 << 24) - 3, 1), ((1 << 16) - 5, 7)]),          # kx = 24 (8, 8, 8), 16 (8, 8) on a coset
    ("BLS12_381_FR", 27, [((1 << 25) - 3, 1), ((1 << 25) - 1, 11)]),        # kx = 25: four passes, two-factor coset
    ("BN254_FR", 28, [((1 << 26) - 3, 1), ((1 << 8) - 1, 13)]),             # two-adicity of BN254 Fr
])
def test_four_pass_plans_closed_form(fname, log_n, lengths):
    closed_form_rounds(fname, log_n, 2500 + log_n, lengths=lengths)


def test_bn254_domain_past_two_adicity_is_refused():
    # the domain is refused at construction, so no transform of 2^29 BN254 elements can be asked for
    assert A.Radix2EvaluationDomain.new("BN254_FR", 1 << 28).log_size_of_group() == 28
    assert A.Radix2EvaluationDomain.new("BN254_FR", 1 << 29) is None
    assert A.Radix2EvaluationDomain.new("BN254_FR", (1 << 28) + 1) is None


# ---- 5. per-call knobs ----------------------------------------------------------------------------------------------
def knob_rounds(fname, log_n, seed, lengths=()):
    if log_n <= 22:
        oracle_rounds(fname, log_n, seed, lengths)
    else:
        closed_form_rounds(fname, log_n, seed, lengths=[(c, 1) for c in lengths])


@pytest.mark.parametrize("tile_log", [11, 12])
@pytest.mark.parametrize("log_n", [11, 12, 16, 17, 22, 25])
def test_tile_log_knob(monkeypatch, tile_log, log_n):
    monkeypatch.setenv("ARK_HIP_FFT_TILE_LOG", str(tile_log))
    fname = FR[log_n % 3]
    # degree-aware: kx = 11 (with 4096-element tiles one pass of 11 stages), kx = 20
    lengths = {16: [(1 << 11) - 3], 22: [(1 << 20) - 3]}.get(log_n, [])
    knob_rounds(fname, log_n, 3000 + 10 * log_n + tile_log, lengths)


@pytest.mark.parametrize("kp", [5, 6, 7])
@pytest.mark.parametrize("log_n", [16, 20])
def test_stages_per_pass_knob(monkeypatch, kp, log_n):
    monkeypatch.setenv("ARK_HIP_FFT_KP", str(kp))
    knob_rounds("BLS12_381_FR", log_n, 3100 + 10 * log_n + kp, [(1 << (log_n - 4)) - 3])


@pytest.mark.parametrize("fname,log_n", [("BN254_FR", 20), ("BLS12_377_FR", 21)])
def test_balanced_knob(monkeypatch, fname, log_n):
    monkeypatch.setenv("ARK_HIP_FFT_BALANCED", "1")
    knob_rounds(fname, log_n, 3200 + log_n)


# every forced plan has a pass count the default plan (for the same tile size) does not have: a plan the device dropped
# would fail the pass count; middle passes leave at least two bits for their columns
@pytest.mark.parametrize("log_n,plan,tile_log", [
    (13, "1,1,11", 12),          # one-stage passes, an 11-stage pass on the 4096-element tile
    (14, "1,1,12", 12),          # a 12-stage pass on the 4096-element tile
    (16, "1,4,11", 11),          # an 11-stage pass on the 2048-element tile
    (13, "7,1,5", None),         # odd first, longest first
    (14, "1,3,10", None),        # one-stage pass; a 10-stage pass last on the default tile
    (15, "10,3,2", None),        # a 10-stage pass first
    (14, "9,3,2", None),         # a 9-stage pass first
    (15, "1,9,5", None),         # a 9-stage middle pass
    (16, "1,9,6", None),
    (15, "1,1,1,1,1,10", None),  # six passes: four ping-buffer to ping-buffer
    (16, "3,3,3,3,4", None),     # five passes
    (16, "2,2,2,2,2,2,2,2", None),   # eight passes: the most the planner reads
    (15, "3,5,7", None),         # odd counts, ascending
])
def test_forced_plans(monkeypatch, log_n, plan, tile_log):
    monkeypatch.setenv("ARK_HIP_FFT_PLAN", plan)
    if tile_log:
        monkeypatch.setenv("ARK_HIP_FFT_TILE_LOG", str(tile_log))
    kps = [int(v) for v in plan.split(",")]
    assert planned(log_n) == kps   # the plan is one the device honours (else the default would run)
    assert len(kps) != len(P.fft_plan(log_n, tile_log=tile_log))   # and the pass count tells it from the default
    fname = FR[log_n % 3]
    fid = O.FID[fname]
    n = 1 << log_n
    x = rand_fr(fid, n, 3300 + log_n)
    d = A.Radix2EvaluationDomain.new(fname, n)
    g = coset_gen(fid)
    dc = d.get_coset(g)
    for dom, off in ((d, None), (dc, g)):
        for inv in (False, True):
            y = to_host(transform(dom, to_dev(x), inverse=inv, npass=len(kps)))
            assert np.array_equal(y, O.fft(fid, x, log_n, off, inv, THREADS).reshape(n, 4)), (plan, off, inv)
    # one stage too many: the plan does not add up and is dropped, the default plan runs (after eight counts nothing
    # more is read, so the eight-pass plan still holds)
    monkeypatch.setenv("ARK_HIP_FFT_PLAN", plan + ",1")
    assert planned(log_n) == (kps if len(kps) == 8 else P.fft_plan(log_n, tile_log=tile_log))
    y = to_host(transform(d, to_dev(x)))
    assert np.array_equal(y, O.fft(fid, x, log_n, None, False, THREADS).reshape(n, 4))


# ---- 6. knobs read once per process ---------------------------------------------------------------------------------
def once_per_process_child():
    """run in a child process whose environment turns the expanded power tables, the compact twiddle table and the
    short-first pass order off"""
    for fname, log_n in (("BLS12_381_FR", 12), ("BN254_FR", 17), ("BLS12_377_FR", 21)):
        oracle_rounds(fname, log_n, 4000 + log_n)
    closed_form_rounds("BLS12_381_FR", 25, 4025, lengths=[((1 << 25) - 3, 1)])


def test_knobs_read_once_per_process():
    env = dict(os.environ, ARK_HIP_FFT_FULL_POWERS="0", ARK_HIP_FFT_COMPACT="0", ARK_HIP_FFT_ASCENDING="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_fft_plans as T\nT.once_per_process_child()\nprint('once-per-process ok')\n"
            % (os.path.dirname(here), here))
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(here), env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "once-per-process ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


# ---- 7. cache and side entries at the new plan classes ------------------------------------------------------------
@pytest.mark.parametrize("fname,log_n", [("BLS12_377_FR", 12), ("BLS12_381_FR", 16)])
def test_power_cache_eviction_by_count(fname, log_n):
    """70 distinct coset offsets (the cache holds 62 and then starts over), then the first one again"""
    fid = O.FID[fname]
    n = 1 << log_n
    x = rand_fr(fid, n, 5000 + log_n)
    d = A.Radix2EvaluationDomain.new(fname, n)
    offs = rand_fr(fid, 70, 5100 + log_n)
    for i, off in enumerate(list(offs) + [offs[0]]):
        dc = d.get_coset(off)
        inv = i % 5 == 4   # an inverse takes a second entry (h^-1 with size_inv)
        y = to_host(transform(dc, to_dev(x), inverse=inv))
        assert np.array_equal(y, O.fft(fid, x, log_n, off, inv, THREADS).reshape(n, 4)), (i, inv)


def test_power_cache_eviction_by_budget():
    """2^26 expanded power tables are 2 GiB each: a fifth distinct offset passes the 8 GiB budget"""
    import torch
    fname, log_n = "BLS12_381_FR", 26
    p = P.MODULI[fname][0]
    a, b = ints(fname, 5200, 2)
    hs = ints(fname, 5201, 5)
    d = A.Radix2EvaluationDomain.new(fname, 1 << log_n)
    x = torch.empty((1 << log_n, 4), dtype=torch.int64, device="cuda")
    for i, h in enumerate(hs + hs[:1]):
        geometric_device(fname, log_n, a, b, out=x)
        transform(d.get_coset(P.to_mont(h, p)), x)
        check_closed_form(fname, log_n, x, a, b, h, seed=i)
    del x
    torch.cuda.empty_cache()


def test_batch_entry_four_pass():
    """fft_batch_in_place at 2^25 with two polynomials: two streams, each with its own ping buffer"""
    import torch
    fname, log_n = "BLS12_381_FR", 25
    d = A.Radix2EvaluationDomain.new(fname, 1 << log_n)
    abs_ = [ints(fname, 5300 + i, 2) for i in range(2)]
    xs = [geometric_device(fname, log_n, a, b) for a, b in abs_]
    for inv in (False, True):
        if inv:
            xs = [geometric_device(fname, log_n, a, b, out=x) for (a, b), x in zip(abs_, xs)]
        with pass_timing():
            assert _sentinel(2) == 1
            d.fft_batch_in_place(xs, inverse=inv)
            assert last_npass() == 4   # the transform on the context stream is timed
        for i, ((a, b), x) in enumerate(zip(abs_, xs)):
            check_closed_form(fname, log_n, x, a, b, inverse=inv, seed=i)
    del xs
    torch.cuda.empty_cache()


def test_carry_free_kernel_four_pass(monkeypatch):
    """the carry-free kernel ignores the tile knob: with 4096-element tiles requested the saturated kernel would run 2^25
    in three passes (8, 8, 9) and a degree-aware kx = 22 in two (11, 11); the carry-free one runs four and three"""
    monkeypatch.setenv("ARK_HIP_FFT_TILE_LOG", "12")
    assert len(P.fft_plan(25, tile_log=12)) == 3 and len(P.fft_plan(25, tile_log=12, carry_free=True)) == 4
    assert len(P.fft_plan(25, 3, tile_log=12)) == 2 and len(P.fft_plan(25, 3, tile_log=12, carry_free=True)) == 3
    check(lib().ark_hip_fft_set_kernel(1), "fft_set_kernel")
    try:
        closed_form_rounds("BN254_FR", 25, 5400, lengths=[((1 << 22) - 3, 1)], carry_free=True)
    finally:
        check(lib().ark_hip_fft_set_kernel(-1), "fft_set_kernel")


def test_sharded_decomposition_three_pass_local():
    """2^22 over 4 ranks: local transforms of 2^20 (6, 6, 8).  (The sharded entries do not report pass timings, so no pass
    count is asserted here; the 2^20 default plan's count is asserted in test_remaining_default_plans_against_oracle.)"""
    import test_gpu_dist_fft as D
    D._emulated("BLS12_381_FR", 22, 4, None)
