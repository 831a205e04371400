"""The transforms over the one-word fields (ark_hip_sfp_fft_batch_device / _fft_in_place) on the GPU against the big-integer model
of tests/smallfp_ref.py: every size from 2^0 to two stages past the plan's first two-pass size, forward and inverse, plain and
coset; batches with gaps and guards; zero-padded inputs; one 2^20 transform against Horner; the low-degree extension end to end;
the host-slice entry; poisoned scratch (a child process).  Seams (one workgroup / two passes / three passes, tile and segment
boundaries) come from ark_hip_sfp_fft_plan."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
import smallfp_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(R.FIELDS)


def dtype(f):
    return np.uint64 if f.bytes == 8 else np.uint32


@functools.lru_cache(maxsize=None)
def domains(name, log, coset):
    """(model domain, device domain) of 2^log elements, plain or on the coset of the field's generator"""
    f = R.FIELDS[name]
    m, d = f.domain_new(1 << log), A.SmallRadix2EvaluationDomain.new(name, 1 << log)
    if coset:
        m, d = f.get_coset(m, f.gen), d.get_coset(f.gen)
    return m, d


@functools.lru_cache(maxsize=None)
def planted_input(name, log):
    """random elements with 0, 1 and p - 1 at index 0, at the last index and on both sides of every segment and tile boundary"""
    f = R.FIELDS[name]
    _, tile, seg, _ = A.small_fft_plan(name, log)
    n = 1 << log
    x = f.random_elements(R.rng(1000 + log), n)
    special = (0, 1, f.p - 1)
    x[0], x[n - 1] = special[log % 3], special[(log + 1) % 3]
    for c, b in enumerate(range(1 << seg, n, 1 << seg)):
        x[b - 1], x[b] = special[c % 3], special[(c + 1) % 3]
    for b in range(1 << tile, n, 1 << tile):
        x[b - 1], x[b] = f.p - 1, f.p - 1
    return tuple(x)


@functools.lru_cache(maxsize=None)
def expected(name, log, coset, inverse):
    f = R.FIELDS[name]
    return f.transform(domains(name, log, coset)[0], list(planted_input(name, log)), inverse)


def device_transform(name, dom, x, inverse=False, num_coeffs=None):
    f = R.FIELDS[name]
    v = A.SmallDeviceVec.from_host(name, np.array(x, dtype=dtype(f)))
    dom.fft_batch_in_place(v.ptr, 1, num_coeffs=num_coeffs, inverse=inverse)
    return v.to_host()


def top_log(name):
    """two stages past the first size the plan gives two passes"""
    single = A.small_fft_plan(name, 0)[0]
    assert len(A.small_fft_plan(name, single + 1)[3]) == 2 and len(A.small_fft_plan(name, single)[3]) == 1
    return single + 3


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("name", FIELDS)
def test_every_size_against_the_model(name, coset, inverse):
    f = R.FIELDS[name]
    for log in range(top_log(name) + 1):
        got = device_transform(name, domains(name, log, coset)[1], planted_input(name, log), inverse)
        want = np.array(expected(name, log, coset, inverse), dtype=dtype(f))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, log, A.small_fft_plan(name, log), "first mismatches at", bad[:8], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("name", FIELDS)
def test_three_passes_against_the_model(name):
    """the smallest size with three passes, beyond the sizes of the sweep above: coset, both directions"""
    f = R.FIELDS[name]
    log = next(l for l in range(f.two_adicity + 1) if len(A.small_fft_plan(name, l)[3]) == 3)
    m, d = domains(name, log, True)
    x = list(planted_input(name, log))
    y = f.fft_fast(m, x)
    got = device_transform(name, d, x)
    assert np.array_equal(got, np.array(y, dtype=dtype(f))), (name, log)
    back = device_transform(name, d, got, inverse=True)
    assert np.array_equal(back, np.array(x, dtype=dtype(f))), (name, log)


@pytest.mark.parametrize("name", FIELDS)
def test_inverse_of_forward_is_the_input(name):
    f = R.FIELDS[name]
    for log in (0, 1, 5, top_log(name) - 3, top_log(name) - 2, top_log(name)):
        for coset in (False, True):
            d = domains(name, log, coset)[1]
            x = np.array(planted_input(name, log), dtype=dtype(f))
            assert np.array_equal(device_transform(name, d, device_transform(name, d, x), inverse=True), x), (name, log, coset)


@pytest.mark.parametrize("name", FIELDS)
def test_batches_write_their_columns_and_nothing_else(name):
    f = R.FIELDS[name]
    dt = dtype(f)
    guard = 64
    for log in (5, top_log(name) - 2):
        n = 1 << log
        d = domains(name, log, True)[1]
        rng = np.random.default_rng(77 + log)
        for count in (1, 2, 3, 65):
            cols = rng.integers(0, f.p, size=(count, n), dtype=np.uint64).astype(dt)
            singles = {inv: [device_transform(name, d, cols[j], inverse=inv) for j in range(min(count, 3))] + [None] * (count - 3)
                       for inv in (False, True)}
            for inv in (False, True):
                singles[inv][-1] = device_transform(name, d, cols[-1], inverse=inv)
            for stride in (n, n + 5):
                for inv in (False, True):
                    buf = np.full(count * stride + guard, np.iinfo(dt).max, dtype=dt)
                    for j in range(count):
                        buf[j * stride:j * stride + n] = cols[j]
                    v = A.SmallDeviceVec.from_host(name, buf)
                    d.fft_batch_in_place(v.ptr, count, stride=stride, inverse=inv)
                    out = v.to_host()
                    assert np.all(out[count * stride:] == np.iinfo(dt).max), (name, log, count, stride, "guard")
                    body = out[:count * stride].reshape(count, stride)
                    assert np.all(body[:, n:] == np.iinfo(dt).max), (name, log, count, stride, "gaps")
                    if count == 65:   # every column of the largest batch, through one more batch with the other stride
                        w = A.SmallDeviceVec.from_host(name, np.ascontiguousarray(cols).reshape(-1))
                        d.fft_batch_in_place(w.ptr, count, stride=n, inverse=inv)
                        assert np.array_equal(body[:, :n], w.to_host().reshape(count, n)), (name, log, stride, inv)
                    for j, s in enumerate(singles[inv]):
                        if s is not None:
                            assert np.array_equal(body[j, :n], s), (name, log, count, stride, inv, j)
    d.fft_batch_in_place(v.ptr, 0)   # count = 0: nothing happens
    assert np.array_equal(v.to_host(), out)


@pytest.mark.parametrize("name", FIELDS)
def test_a_launch_beyond_the_wide_workgroups(name):
    """A pass runs 1024 threads per workgroup while its launch has at most 512 workgroups and 512 beyond.  300 columns of the first
    two-pass size are 600 workgroups per pass: the same columns in chunks of 60 (120 workgroups) go through the other kernels and
    must give the same, and four columns are compared with the model."""
    f = R.FIELDS[name]
    dt = dtype(f)
    log = top_log(name) - 2
    n = 1 << log
    stages = A.small_fft_plan(name, log)[3]
    assert len(stages) == 2 and 300 * 2 > 512 >= 60 * 2
    m, d = domains(name, log, True)
    cols = np.random.default_rng(300).integers(0, f.p, size=(300, n), dtype=np.uint64).astype(dt)
    for inverse in (False, True):
        whole = A.SmallDeviceVec.from_host(name, cols.reshape(-1))
        d.fft_batch_in_place(whole.ptr, 300, inverse=inverse)
        got = whole.to_host().reshape(300, n)
        for c in range(0, 300, 60):
            part = A.SmallDeviceVec.from_host(name, cols[c:c + 60].reshape(-1))
            d.fft_batch_in_place(part.ptr, 60, inverse=inverse)
            assert np.array_equal(got[c:c + 60], part.to_host().reshape(60, n)), (name, inverse, c)
        for j in (0, 1, 150, 299):
            assert np.array_equal(got[j], np.array(f.transform(m, cols[j].tolist(), inverse), dtype=dt)), (name, inverse, j)


@pytest.mark.parametrize("name", FIELDS)
def test_num_coeffs_reads_a_zero_padded_prefix(name):
    f = R.FIELDS[name]
    dt = dtype(f)
    for log in (4, 10, top_log(name) - 2):
        n = 1 << log
        for coset in (False, True):
            m, d = domains(name, log, coset)
            x = list(planted_input(name, log))
            for nc in sorted({1, 2, n // 4 - 1, n // 4, n // 4 + 1, n - 1, n}):
                if nc < 1:
                    continue
                garbage = x[:nc] + [f.p - 1 - (i % 7) for i in range(n - nc)]   # what lies behind num_coeffs must not be read
                got = device_transform(name, d, garbage, num_coeffs=nc)
                want = np.array(f.transform(m, x[:nc]), dtype=dt)
                assert np.array_equal(got, want), (name, log, coset, nc)


@pytest.mark.parametrize("name", FIELDS)
def test_2_20_against_horner(name):
    f = R.FIELDS[name]
    log = 20
    n = 1 << log
    m, d = domains(name, log, True)
    rng = np.random.default_rng(2020)
    x = rng.integers(0, f.p, size=n, dtype=np.uint64).astype(dtype(f))
    got = device_transform(name, d, x)
    plain = [c * f.rinv % f.p for c in x.tolist()]
    prng = R.rng(2021)
    for j in [0, n - 1] + [prng.randrange(n) for _ in range(4)]:
        point = f.from_mont(f.domain_element(m, j))
        acc = 0
        for c in reversed(plain):
            acc = (acc * point + c) % f.p
        assert int(got[j]) == f.to_mont(acc), (name, j)
    assert np.array_equal(device_transform(name, d, got, inverse=True), x)


@pytest.mark.parametrize("name", FIELDS)
def test_low_degree_extension(name):
    """8 columns of 2^10 evaluations to the coset of 2^12.  Every output is checked against Horner: on the 31-bit fields with exact
    uint64 arithmetic on all 4096 points at once; on Goldilocks (no exact 64-bit product in numpy) every output against the model's
    transform of the interpolated coefficients and every 16th output of every column against Horner."""
    f = R.FIELDS[name]
    dt = dtype(f)
    small_m, small_d = domains(name, 10, False)
    big_m, big_d = domains(name, 12, True)
    rng = np.random.default_rng(1012)
    evals = rng.integers(0, f.p, size=(8, 1 << 10), dtype=np.uint64).astype(dt)
    mat = A.SmallDeviceMatrix.from_host(name, evals, stride=1 << 12)
    mat.low_degree_extend(small_d, big_d)
    out = mat.to_host()
    points_plain = [f.from_mont(f.domain_element(big_m, j)) for j in range(1 << 12)]
    for col in range(8):
        coeffs = f.fft_fast(small_m, evals[col].tolist(), inverse=True)
        plain = [f.from_mont(c) for c in coeffs]
        if f.bytes == 4:
            pts, acc = np.array(points_plain, dtype=np.uint64), np.zeros(1 << 12, dtype=np.uint64)
            for c in reversed(plain):
                acc = (acc * pts + np.uint64(c)) % np.uint64(f.p)       # < 2^62 + 2^31: exact
            want = (acc * np.uint64(f.r) % np.uint64(f.p)).astype(dt)
            assert np.array_equal(out[col], want), (name, col)
        else:
            assert np.array_equal(out[col], np.array(f.fft_fast(big_m, coeffs), dtype=dt)), (name, col)
            for j in range(0, 1 << 12, 16):
                acc = 0
                for c in reversed(plain):
                    acc = (acc * points_plain[j] + c) % f.p
                assert int(out[col][j]) == f.to_mont(acc), (name, col, j)
    assert f.fft_fast(small_m, coeffs) == evals[7].tolist()   # the model's interpolation reproduces what it was given


@pytest.mark.parametrize("name", FIELDS)
def test_host_slice_entry(name):
    f = R.FIELDS[name]
    for log in (0, 3, 10, top_log(name) - 2):
        for coset in (False, True):
            m, d = domains(name, log, coset)
            x = np.array(planted_input(name, log), dtype=dtype(f))
            assert np.array_equal(d.fft(x), np.array(expected(name, log, coset, False), dtype=dtype(f))), (name, log, coset)
            assert np.array_equal(d.ifft(x), np.array(expected(name, log, coset, True), dtype=dtype(f))), (name, log, coset)
    short = x[:5]
    assert np.array_equal(d.fft(short), np.array(f.transform(m, short.tolist()), dtype=dtype(f)))


def test_poisoned_scratch():
    """DESIGN.md section 16 through ark_hip_test_scratch_poison: a 2^16 transform, poison, then a 2^9 transform and a batch, for
    every field, in a fresh child process against libark_hip_test.so"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "smallfp_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.count("\nok ") + out.stdout.startswith("ok ") == 3, (out.stdout[-2000:], out.stderr[-4000:])
