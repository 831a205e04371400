"""Every pointwise entry of the one-word fields (ark_hip_sfp_{add,sub,mul,neg,scale,inverse,from_canonical,into_canonical}_device)
on the GPU against Python integers: the lengths around a wave, a block and the vector width, edge values crossed with each other,
the result aliasing either input, unaligned pointers, and guard regions on both sides of the output."""
import ctypes as C

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
import smallfp_ref as R

pytestmark = pytest.mark.gpu
FIELDS = list(R.FIELDS)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1000, (1 << 16) + 1)
GUARD = 8


def dtype(f):
    return np.uint64 if f.bytes == 8 else np.uint32


def inputs(f, n, seed):
    """two vectors: the edge values crossed with each other in front, random behind"""
    rng = R.rng(seed)
    e = f.edge_values()
    cross = [(a, b) for a in e for b in e]
    a = [cross[i][0] if i < len(cross) else rng.randrange(f.p) for i in range(n)]
    b = [cross[i][1] if i < len(cross) else rng.randrange(f.p) for i in range(n)]
    return a, b


class Arena:
    """one device allocation holding guard | a | guard | b | guard | r | guard, every guard 0xFF bytes; `shift` moves the vectors
    off 16-byte alignment"""

    def __init__(self, f, n, a, b, shift=0):
        self.f, self.n, self.dt = f, n, dtype(f)
        self.slot = (n + 2 * GUARD + 4 + 3) // 4 * 4   # every slot starts 16-byte aligned: shift 0 takes the vector path
        fill = np.iinfo(self.dt).max
        self.host = np.full(3 * self.slot, fill, dtype=self.dt)
        self.off = [k * self.slot + GUARD + shift for k in range(3)]
        self.host[self.off[0]:self.off[0] + n] = a
        self.host[self.off[1]:self.off[1] + n] = b
        self.vec = A.SmallDeviceVec.from_host(f.name, self.host)

    def ptr(self, k):
        return C.c_void_p(self.vec.ptr + self.off[k] * self.f.bytes)

    def result(self, k, touched):
        """slot k's vector after the call; everything outside slot k's n elements must be as uploaded"""
        out = self.vec.to_host()
        mask = np.ones(out.size, dtype=bool)
        mask[self.off[k]:self.off[k] + self.n] = False
        assert np.array_equal(out[mask], self.host[mask]), (self.f.name, self.n, touched, "wrote outside its output")
        return out[self.off[k]:self.off[k] + self.n]


def call(f, op, arena, dst, k=None):
    L = _lib.lib()
    n = arena.n
    if op in ("add", "sub", "mul"):
        rc = getattr(L, "ark_hip_sfp_%s_device" % op)(f.sid, arena.ptr(0), arena.ptr(1), arena.ptr(dst), n)
    elif op == "scale":
        rc = L.ark_hip_sfp_scale_device(f.sid, arena.ptr(0), k, arena.ptr(dst), n)
    else:
        rc = getattr(L, "ark_hip_sfp_%s_device" % op)(f.sid, arena.ptr(0), arena.ptr(dst), n)
    assert rc == 0, (f.name, op, n, rc)


def model(f, op, a, b, k=None):
    if op == "add":
        return [f.add(x, y) for x, y in zip(a, b)]
    if op == "sub":
        return [f.sub(x, y) for x, y in zip(a, b)]
    if op == "mul":
        return [f.mul(x, y) for x, y in zip(a, b)]
    if op == "neg":
        return [(f.p - x) % f.p for x in a]
    if op == "scale":
        return [f.mul(x, k) for x in a]
    if op == "inverse":
        return [f.inv(x) for x in a]
    raise AssertionError(op)


@pytest.mark.parametrize("op", ["add", "sub", "mul", "neg", "scale"])
@pytest.mark.parametrize("name", FIELDS)
def test_pointwise_ops(name, op):
    f = R.FIELDS[name]
    for n in LENGTHS:
        a, b = inputs(f, n, 31 + n)
        for k in ((f.p - 1, f.r, 0) if op == "scale" else (None,)):
            want = np.array(model(f, op, a, b, k), dtype=dtype(f))
            # r apart from the inputs, r = a, r = b (binary ops), and all three off 16-byte alignment
            for dst, shift in ((2, 0), (0, 0), (1, 0), (2, 1), (0, 1)):
                if dst == 1 and op not in ("add", "sub", "mul"):
                    continue
                arena = Arena(f, n, a, b, shift)
                call(f, op, arena, dst, k)
                got = arena.result(dst, (op, dst, shift))
                assert np.array_equal(got, want), (name, op, n, dst, shift, np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("name", FIELDS)
def test_inverse_keeps_zeros_and_inverts_the_rest(name):
    f = R.FIELDS[name]
    one = f.r
    for n in LENGTHS:
        a, _ = inputs(f, n, 57 + n)
        for i in (0, 1, 62, 63, 64, 65, 127, 128, 255, 256, n - 2, n - 1):   # zeros at both ends and around wave boundaries
            if 0 <= i < n:
                a[i] = 0
        want = np.array(model(f, "inverse", a, a), dtype=dtype(f))   # pow(x, p - 2) in Montgomery form; zero for zero
        for dst, shift in ((2, 0), (0, 0), (2, 1)):
            arena = Arena(f, n, a, a, shift)
            call(f, "inverse", arena, dst)
            got = arena.result(dst, ("inverse", dst, shift))
            assert np.array_equal(got, want), (name, n, dst, shift, np.nonzero(got != want)[0][:8])
            for x, y in zip(a[:300], got[:300].tolist()):
                assert (y == 0) if x == 0 else (f.mul(x, y) == one), (name, n, x, y)


@pytest.mark.parametrize("name", FIELDS)
def test_canonical_conversions(name):
    f = R.FIELDS[name]
    dt = dtype(f)
    top = int(np.iinfo(dt).max)
    for n in LENGTHS:
        rng = R.rng(91 + n)
        raw = [0, 1, f.p - 1, f.p, f.p + 1, top, top - 1, 2 * f.p if 2 * f.p <= top else top, 1 << 31, (1 << 32) - 1]
        x = [(raw[i] if i < len(raw) else rng.randrange(top + 1)) for i in range(n)]   # the word's whole range, values >= p too
        for shift in (0, 1):
            arena = Arena(f, n, x, x, shift)
            call(f, "from_canonical", arena, 2)
            mont = arena.result(2, ("from_canonical", shift))
            assert np.array_equal(mont, np.array([f.to_mont(v) for v in x], dtype=dt)), (name, n, shift)
            arena2 = Arena(f, n, mont, mont, shift)
            call(f, "into_canonical", arena2, 0)   # in place
            back = arena2.result(0, ("into_canonical", shift))
            assert np.array_equal(back, np.array([v % f.p for v in x], dtype=dt)), (name, n, shift)


@pytest.mark.parametrize("name", FIELDS)
def test_device_vec_mirror(name):
    f = R.FIELDS[name]
    dt = dtype(f)
    a, b = inputs(f, 1000, 5)
    va, vb = A.SmallDeviceVec.from_host(name, np.array(a, dtype=dt)), A.SmallDeviceVec.from_host(name, np.array(b, dtype=dt))
    vc = va.clone()
    vc += vb
    vc *= vb
    vc -= va
    vc.scale(f.gen).negate()
    want = [(f.p - f.mul(f.sub(f.mul(f.add(x, y), y), x), f.gen)) % f.p for x, y in zip(a, b)]
    assert vc.to_host().tolist() == want
    vd = vc.clone().batch_inverse()
    vd *= vc
    assert vd.to_host().tolist() == [f.r if w else 0 for w in want]
    assert va.to_host().tolist() == a and vb.to_host().tolist() == b and len(va) == 1000
    # evaluate_over_domain / interpolate: 100 coefficients over the coset of 2^8
    m = f.get_coset(f.domain_new(256), f.gen)
    d = A.SmallRadix2EvaluationDomain.new(name, 256).get_coset(f.gen)
    coeffs = A.SmallDeviceVec.from_host(name, np.array(a[:100], dtype=dt))
    ev = coeffs.evaluate_over_domain(d)
    assert ev.to_host().tolist() == f.transform(m, a[:100])
    assert ev.interpolate(d).to_host().tolist() == a[:100] + [0] * 156
