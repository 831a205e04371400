"""Host-side checks of the one-word fields (no GPU): the model of tests/smallfp_ref.py against the literals of the reference's three
SmallFp instances and against itself, and the host entries of the library (ark_hip_sfp_info / _pow / _radix2_domain_new /
_get_coset / _fft_plan and every argument error) against the model."""
import ctypes as C
import os
import re

import pytest

import algebra_amd as A
from algebra_amd import _lib, smallfp
import smallfp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(R.FIELDS)
ERR_ARG, ERR_SIZE, ERR_NO_DEVICE = -1, -2, -5

# field: (p, two-adicity, R mod p, g^((p-1)/2^s) plain, the same as stored)
LITERALS = {
    "GOLDILOCKS": (18446744069414584321, 32, 4294967295, 1753635133440165772, 15733474329512464024),
    "BABYBEAR": (2013265921, 27, 268435454, 440564289, 1476048622),
    "KOALABEAR": (2130706433, 24, 33554430, 1791270792, 331895189),
}


@pytest.mark.parametrize("name", FIELDS)
def test_model_constants_are_the_reference_literals(name):
    f = R.FIELDS[name]
    assert (f.p, f.two_adicity, f.r, f.root_plain, f.root) == LITERALS[name]
    assert f.k_bits == (64 if name == "GOLDILOCKS" else 32) and f.R == 1 << f.k_bits
    assert f.gen_plain == {"GOLDILOCKS": 7, "BABYBEAR": 31, "KOALABEAR": 3}[name]
    assert pow(f.root_plain, 1 << f.two_adicity, f.p) == 1 and pow(f.root_plain, 1 << (f.two_adicity - 1), f.p) == f.p - 1
    assert f.p * f.nprime % f.R == f.R - 1


@pytest.mark.parametrize("name", FIELDS)
def test_model_step_sequences_equal_the_plain_formula(name):
    f = R.FIELDS[name]
    rng = R.rng(11)
    edges = f.edge_values()
    assert {0, 1, 2, f.p - 1, f.p - 2, f.r} <= set(edges)
    pairs = [(a, b) for a in edges for b in edges] + [(rng.randrange(f.p), rng.randrange(f.p)) for _ in range(20000)]
    pairs += [(a, rng.randrange(f.p)) for a in edges for _ in range(50)]
    for a, b in pairs:
        want = f.mul(a, b)
        assert f.mul_steps(a, b) == want, (a, b)
        assert f.mul_generic_steps(a, b) == want, (a, b)


@pytest.mark.parametrize("name", FIELDS)
def test_model_fast_transform_equals_the_naive_dft(name):
    f = R.FIELDS[name]
    rng = R.rng(12)
    for log in range(9):
        plain = f.domain_new(1 << log)
        for dom in (plain, f.get_coset(plain, f.gen)):
            x = f.random_elements(rng, 1 << log)
            for inverse in (False, True):
                assert f.fft_fast(dom, x, inverse) == f.dft_naive(dom, x, inverse), (log, inverse)
            assert f.fft_fast(dom, f.fft_fast(dom, x), True) == x
            if log:   # a short input is its zero extension, and the value at the j-th domain element is Horner's
                short = x[:(1 << log) - 1]
                y = f.fft_fast(dom, short)
                assert y == f.dft_naive(dom, short + [0])
                assert y[1] == f.horner(short, f.domain_element(dom, 1))


@pytest.mark.parametrize("name", FIELDS)
def test_info_and_pow(name):
    f = R.FIELDS[name]
    info = A.small_field_info(name)
    assert info == dict(bytes=f.bytes, p=f.p, k_bits=f.k_bits, r=f.r, r2=f.r2, generator=f.gen, two_adicity=f.two_adicity,
                        two_adic_root=f.root)
    assert smallfp.SMALL_FIELDS[name] == (f.sid, f.bytes, f.p)
    rng = R.rng(13)
    for a in f.edge_values() + f.random_elements(rng, 50):
        for e in (0, 1, 2, 3, f.p - 2, f.p - 1, (1 << 64) - 1, rng.randrange(1 << 64)):
            assert A.small_field_pow(name, a, e) == f.pow(a, e), (a, e)
    for a, b in [(a, b) for a in f.edge_values() for b in f.edge_values()]:   # the library's multiply on the edge values
        assert A.small_field_pow(name, f.mul(a, b), 2) == f.mul(f.mul(a, a), f.mul(b, b))


@pytest.mark.parametrize("name", FIELDS)
def test_domain_new_and_coset_for_every_log_size(name):
    f = R.FIELDS[name]
    rng = R.rng(14)
    for log in range(f.two_adicity + 1):
        for num in {1 << log, (1 << log) - 1 if log > 1 else 1 << log}:
            d = A.SmallRadix2EvaluationDomain.new(name, num)
            want = f.domain_new(num)
            assert d is not None and {k: getattr(d._s, k) for k in R.DOMAIN_KEYS} == want, (log, num)
        assert d.size() == 1 << log and d.log_size_of_group() == log
        assert f.pow(d.group_gen(), 1 << log) == f.r and (log == 0 or f.pow(d.group_gen(), 1 << (log - 1)) == f.p - f.r)
        for offset in (f.gen, f.r, f.p - 1, rng.randrange(1, f.p)):
            c = d.get_coset(offset)
            assert {k: getattr(c._s, k) for k in R.DOMAIN_KEYS} == f.get_coset(want, offset), (log, offset)
    assert A.SmallRadix2EvaluationDomain.new(name, 0).size() == 1
    assert A.SmallRadix2EvaluationDomain.new(name, (1 << f.two_adicity) + 1) is None
    s = _lib.SmallRadix2DomainStruct()
    assert _lib.lib().ark_hip_sfp_radix2_domain_new(f.sid, (1 << f.two_adicity) + 1, C.byref(s)) == ERR_SIZE
    assert d.get_coset(0) is None


@pytest.mark.parametrize("name", FIELDS)
def test_plan_invariants_for_every_log_size(name):
    f = R.FIELDS[name]
    single0, tile0, seg0, _ = A.small_fft_plan(name, 0)
    assert (1 << tile0) * f.bytes == 32 << 10 and (1 << seg0) * f.bytes == 128 and single0 <= tile0
    seen_passes = set()
    for log in range(f.two_adicity + 1):
        single, tile, seg, stages = A.small_fft_plan(name, log)
        assert (single, tile, seg) == (single0, tile0, seg0)
        assert sum(stages) == log and 1 <= len(stages) <= 4, (log, stages)
        if log <= single:
            assert stages == [log]
        else:   # every pass shares its tile with 2^seg neighbours of the other dimension
            assert len(stages) >= 2 and all(1 <= s <= tile - seg for s in stages), (log, stages)
            assert len(stages) == -(-log // (tile - seg)), "the fewest passes"
        seen_passes.add(len(stages))
    assert {1, 2, 3} <= seen_passes
    out = (C.c_int * 8)()
    assert _lib.lib().ark_hip_sfp_fft_plan(f.sid, f.two_adicity + 1, out) == ERR_SIZE


def test_argument_errors_come_before_any_device():
    """every ARK_HIP_ERR_ARG the header lists, with no GPU in reach (this test runs on a CPU-only host too: a call that got past
    its argument checks would answer ARK_HIP_ERR_NO_DEVICE there, or touch the fake pointer on a GPU host)"""
    L = _lib.lib()
    u64 = C.c_uint64()
    out8, plan8 = (C.c_uint64 * 8)(), (C.c_int * 8)()
    dom = _lib.SmallRadix2DomainStruct()
    fake = C.c_void_p(0x1000)
    for bad in (-1, 3, 5, 99):   # the scalar-field ids of the four-limb family are no small-field ids
        assert L.ark_hip_sfp_info(bad, out8) == ERR_ARG
        assert L.ark_hip_sfp_pow(bad, 1, 1, C.byref(u64)) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_new(bad, 4, C.byref(dom)) == ERR_ARG
        assert L.ark_hip_sfp_fft_plan(bad, 4, plan8) == ERR_ARG
        assert L.ark_hip_sfp_add_device(bad, fake, fake, fake, 4) == ERR_ARG
        assert L.ark_hip_sfp_neg_device(bad, fake, fake, 4) == ERR_ARG
        assert L.ark_hip_sfp_scale_device(bad, fake, 1, fake, 4) == ERR_ARG
    for name in FIELDS:
        f = R.FIELDS[name]
        sid = f.sid
        assert L.ark_hip_sfp_info(sid, None) == ERR_ARG
        assert L.ark_hip_sfp_pow(sid, 1, 1, None) == ERR_ARG
        assert L.ark_hip_sfp_pow(sid, f.p, 1, C.byref(u64)) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_new(sid, 4, None) == ERR_ARG
        assert L.ark_hip_sfp_fft_plan(sid, 4, None) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_new(sid, 16, C.byref(dom)) == 0
        cos = _lib.SmallRadix2DomainStruct()
        assert L.ark_hip_sfp_radix2_domain_get_coset(sid, None, f.gen, C.byref(cos)) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_get_coset(sid, C.byref(dom), f.gen, None) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_get_coset(sid, C.byref(dom), 0, C.byref(cos)) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_get_coset(sid, C.byref(dom), f.p, C.byref(cos)) == ERR_ARG
        # transforms: null pointers, stride < size, num_coeffs out of range, inverse with a short input, a size that is not
        # 2^log_size_of_group
        assert L.ark_hip_sfp_fft_batch_device(sid, None, fake, 1, 16, 16, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(dom), None, 1, 16, 16, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(dom), fake, 1, 15, 16, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(dom), fake, 1, 16, 0, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(dom), fake, 1, 16, 17, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(dom), fake, 1, 16, 8, 1) == ERR_ARG
        assert L.ark_hip_sfp_fft_in_place(sid, None, fake, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_in_place(sid, C.byref(dom), None, 0) == ERR_ARG
        broken = _lib.SmallRadix2DomainStruct.from_buffer_copy(dom)
        broken.size = 24
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(broken), fake, 1, 32, 16, 0) == ERR_ARG
        assert L.ark_hip_sfp_fft_in_place(sid, C.byref(broken), fake, 0) == ERR_ARG
        assert L.ark_hip_sfp_radix2_domain_get_coset(sid, C.byref(broken), f.gen, C.byref(cos)) == ERR_ARG
        broken = _lib.SmallRadix2DomainStruct.from_buffer_copy(dom)
        broken.log_size_of_group, broken.size = 40, 1 << 40
        assert L.ark_hip_sfp_fft_batch_device(sid, C.byref(broken), fake, 1, 1 << 40, 16, 0) == ERR_ARG
        # pointwise: null pointers with n > 0, a scale factor >= p
        assert L.ark_hip_sfp_add_device(sid, None, fake, fake, 4) == ERR_ARG
        assert L.ark_hip_sfp_sub_device(sid, fake, None, fake, 4) == ERR_ARG
        assert L.ark_hip_sfp_mul_device(sid, fake, fake, None, 4) == ERR_ARG
        for fn in (L.ark_hip_sfp_neg_device, L.ark_hip_sfp_inverse_device, L.ark_hip_sfp_from_canonical_device,
                   L.ark_hip_sfp_into_canonical_device):
            assert fn(sid, None, fake, 4) == ERR_ARG and fn(sid, fake, None, 4) == ERR_ARG
        assert L.ark_hip_sfp_scale_device(sid, None, 1, fake, 4) == ERR_ARG
        assert L.ark_hip_sfp_scale_device(sid, fake, f.p, fake, 4) == ERR_ARG
    # the four-limb family keeps refusing ids it does not serve: nothing of this family leaks into `field` arguments
    big = _lib.Radix2DomainStruct()
    for fid in (0, 2, 4, 6, 7):
        assert L.ark_hip_radix2_domain_new(fid, 16, C.byref(big)) == ERR_ARG


def test_without_a_gpu_the_device_entries_say_so():
    L = _lib.lib()
    if L.ark_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    dom = _lib.SmallRadix2DomainStruct()
    assert L.ark_hip_sfp_radix2_domain_new(0, 16, C.byref(dom)) == 0
    fake = C.c_void_p(0x1000)
    assert L.ark_hip_sfp_fft_batch_device(0, C.byref(dom), fake, 1, 16, 16, 0) == ERR_NO_DEVICE
    assert L.ark_hip_sfp_add_device(0, fake, fake, fake, 4) == ERR_NO_DEVICE


def test_header_bindings_and_mirrors_name_the_same_entries():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    declared = set(re.findall(r"\b(ark_hip_sfp_[a-z0-9_]+)\s*\(", hdr))
    bound = {s for s in _lib.SYMBOLS if s.startswith("ark_hip_sfp_")}
    assert declared == bound and len(declared) == 15, declared ^ bound
    py = open(os.path.join(ROOT, "algebra_amd", "smallfp.py")).read()
    cpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for mirror, text in (("smallfp.py", py), ("ark_hip.hpp", cpp)):
        used = set(re.findall(r"\b(ark_hip_sfp_[a-z0-9_]+)\s*\(", text))
        assert used == declared, (mirror, used ^ declared)
    for cls in ("SmallRadix2EvaluationDomain", "SmallDeviceVec"):
        assert ("class " + cls) in py and ("class " + cls) in cpp, cls
    for ident in ("ARK_HIP_SFP_GOLDILOCKS = 0", "ARK_HIP_SFP_BABYBEAR = 1", "ARK_HIP_SFP_KOALABEAR = 2"):
        assert ident in hdr
    fields = [n for n, _ in _lib.SmallRadix2DomainStruct._fields_]
    assert fields == ["size", "log_size_of_group", "_pad"] + list(R.DOMAIN_KEYS[2:])
    assert C.sizeof(_lib.SmallRadix2DomainStruct) == 72
