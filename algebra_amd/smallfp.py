"""Host mirror of the reference's one-word fields (ff/src/fields/models/small_fp/: SmallFp<P>) behind the ark_hip_sfp_* entries:
Goldilocks (uint64), BabyBear and KoalaBear (uint32), the three instances of test-curves/src/smallfp.rs.

An element is SmallFp::value, the canonical Montgomery residue x * R mod p in the field's own word (R = 2^64, and 2^32 for both
31-bit fields); vectors are numpy arrays of that word, single elements Python integers.  SmallRadix2EvaluationDomain mirrors
Radix2EvaluationDomain<SmallFp<P>>, SmallDeviceVec a resident Vec<SmallFp<P>>, SmallDeviceMatrix a batch of columns.  This module
holds no arithmetic: everything runs in libark_hip.so.
"""
import ctypes as C

import numpy as np

from ._lib import SmallRadix2DomainStruct, check, lib

# name -> (id, word bytes, modulus)
SMALL_FIELDS = {
    "GOLDILOCKS": (0, 8, 2**64 - 2**32 + 1),
    "BABYBEAR": (1, 4, 2**31 - 2**27 + 1),
    "KOALABEAR": (2, 4, 2**31 - 2**24 + 1),
}


def small_field_id(field):
    if isinstance(field, str):
        return SMALL_FIELDS[field][0]
    if field not in (0, 1, 2):
        raise ValueError("unknown small field %r" % (field,))
    return int(field)


def small_field_dtype(field):
    return np.dtype(np.uint64 if small_field_id(field) == 0 else np.uint32)


def small_field_info(field):
    """ark_hip_sfp_info as a dict; the generator and the two-adic root as stored."""
    out = (C.c_uint64 * 8)()
    check(lib().ark_hip_sfp_info(small_field_id(field), out), "ark_hip_sfp_info")
    keys = ("bytes", "p", "k_bits", "r", "r2", "generator", "two_adicity", "two_adic_root")
    return dict(zip(keys, (int(v) for v in out)))


def small_field_pow(field, base, exp):
    out = C.c_uint64()
    check(lib().ark_hip_sfp_pow(small_field_id(field), base, exp, C.byref(out)), "ark_hip_sfp_pow")
    return int(out.value)


def small_fft_plan(field, log_n):
    """ark_hip_sfp_fft_plan: (largest one-workgroup log n, tile log, segment log, [stages of every pass]); host only."""
    out = (C.c_int * 8)()
    check(lib().ark_hip_sfp_fft_plan(small_field_id(field), log_n, out), "ark_hip_sfp_fft_plan")
    return int(out[0]), int(out[1]), int(out[2]), [int(out[4 + i]) for i in range(int(out[3]))]


def _host(field, x):
    a = np.ascontiguousarray(x, dtype=small_field_dtype(field))
    if a.ndim != 1:
        raise ValueError("a vector of field words is one-dimensional")
    return a


class SmallRadix2EvaluationDomain:
    def __init__(self, field, struct):
        self.field = small_field_id(field)
        self._s = struct

    @classmethod
    def new(cls, field, num_coeffs):
        """Radix2EvaluationDomain::new (radix2/mod.rs:55-83); None beyond the field's two-adicity, as the reference."""
        s = SmallRadix2DomainStruct()
        rc = lib().ark_hip_sfp_radix2_domain_new(small_field_id(field), num_coeffs, C.byref(s))
        if rc == -2:
            return None
        check(rc, "ark_hip_sfp_radix2_domain_new")
        return cls(field, s)

    def get_coset(self, offset):
        """get_coset (radix2/mod.rs:85-92); None for a zero offset."""
        if offset == 0:
            return None
        s = SmallRadix2DomainStruct()
        check(lib().ark_hip_sfp_radix2_domain_get_coset(self.field, C.byref(self._s), offset, C.byref(s)),
              "ark_hip_sfp_radix2_domain_get_coset")
        return SmallRadix2EvaluationDomain(self.field, s)

    def size(self):
        return int(self._s.size)

    def log_size_of_group(self):
        return int(self._s.log_size_of_group)

    def size_as_field_element(self):
        return int(self._s.size_as_field_element)

    def size_inv(self):
        return int(self._s.size_inv)

    def group_gen(self):
        return int(self._s.group_gen)

    def group_gen_inv(self):
        return int(self._s.group_gen_inv)

    def coset_offset(self):
        return int(self._s.offset)

    def coset_offset_inv(self):
        return int(self._s.offset_inv)

    def coset_offset_pow_size(self):
        return int(self._s.offset_pow_size)

    def _padded(self, x):
        a = _host(self.field, x)
        if a.size > self.size():
            raise ValueError("more coefficients than the domain holds")
        out = np.zeros(self.size(), dtype=a.dtype)
        out[:a.size] = a
        return out

    def fft(self, coeffs):
        """EvaluationDomain::fft on a host array: zero-extended to the domain, one upload and one download."""
        out = self._padded(coeffs)
        check(lib().ark_hip_sfp_fft_in_place(self.field, C.byref(self._s), out.ctypes.data_as(C.c_void_p), 0),
              "ark_hip_sfp_fft_in_place")
        return out

    def ifft(self, evals):
        out = self._padded(evals)
        check(lib().ark_hip_sfp_fft_in_place(self.field, C.byref(self._s), out.ctypes.data_as(C.c_void_p), 1),
              "ark_hip_sfp_fft_in_place")
        return out

    def fft_batch_in_place(self, d_data, count, stride=None, num_coeffs=None, inverse=False):
        """ark_hip_sfp_fft_batch_device on a raw device pointer: count columns, `stride` elements apart."""
        stride = self.size() if stride is None else stride
        num_coeffs = self.size() if num_coeffs is None else num_coeffs
        check(lib().ark_hip_sfp_fft_batch_device(self.field, C.byref(self._s), d_data, count, stride, num_coeffs, 1 if inverse else 0),
              "ark_hip_sfp_fft_batch_device")


class SmallDeviceVec:
    """A vector of field words resident on the device."""

    def __init__(self, field, length):
        self.field = small_field_id(field)
        self.dtype = small_field_dtype(field)
        self.len = int(length)
        self._p = C.c_void_p()
        check(lib().ark_hip_malloc(max(self.nbytes, 16), C.byref(self._p)), "ark_hip_malloc")

    @property
    def nbytes(self):
        return self.len * self.dtype.itemsize

    @property
    def ptr(self):
        return self._p.value

    @classmethod
    def from_host(cls, field, x):
        a = _host(field, x)
        v = cls(field, a.size)
        if a.size:
            check(lib().ark_hip_memcpy_h2d(v._p, a.ctypes.data_as(C.c_void_p), a.nbytes), "ark_hip_memcpy_h2d")
        return v

    @classmethod
    def zeros(cls, field, length):
        v = cls(field, length)
        if v.len:
            check(lib().ark_hip_memset_device(v._p, 0, v.nbytes), "ark_hip_memset_device")
        return v

    def to_host(self):
        out = np.empty(self.len, dtype=self.dtype)
        if self.len:
            check(lib().ark_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self._p, self.nbytes), "ark_hip_memcpy_d2h")
        return out

    def clone(self):
        v = SmallDeviceVec(self.field, self.len)
        if self.len:
            check(lib().ark_hip_memcpy_d2d(v._p, self._p, self.nbytes), "ark_hip_memcpy_d2d")
        return v

    def free(self):
        if self._p:
            lib().ark_hip_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __len__(self):
        return self.len

    def _same(self, o):
        if o.field != self.field or o.len != self.len:
            raise ValueError("vectors of one field and one length are combined")

    def __iadd__(self, o):
        self._same(o)
        check(lib().ark_hip_sfp_add_device(self.field, self._p, o._p, self._p, self.len), "ark_hip_sfp_add_device")
        return self

    def __isub__(self, o):
        self._same(o)
        check(lib().ark_hip_sfp_sub_device(self.field, self._p, o._p, self._p, self.len), "ark_hip_sfp_sub_device")
        return self

    def __imul__(self, o):
        self._same(o)
        check(lib().ark_hip_sfp_mul_device(self.field, self._p, o._p, self._p, self.len), "ark_hip_sfp_mul_device")
        return self

    def scale(self, k):
        check(lib().ark_hip_sfp_scale_device(self.field, self._p, k, self._p, self.len), "ark_hip_sfp_scale_device")
        return self

    def negate(self):
        check(lib().ark_hip_sfp_neg_device(self.field, self._p, self._p, self.len), "ark_hip_sfp_neg_device")
        return self

    def batch_inverse(self):
        """ark_ff::batch_inversion: every non-zero element inverted, zeros left alone."""
        check(lib().ark_hip_sfp_inverse_device(self.field, self._p, self._p, self.len), "ark_hip_sfp_inverse_device")
        return self

    def from_canonical(self):
        check(lib().ark_hip_sfp_from_canonical_device(self.field, self._p, self._p, self.len), "ark_hip_sfp_from_canonical_device")
        return self

    def into_canonical(self):
        check(lib().ark_hip_sfp_into_canonical_device(self.field, self._p, self._p, self.len), "ark_hip_sfp_into_canonical_device")
        return self

    def commit(self, wait=True):
        """MerkleTree.commit_small of this vector as one column (merkle.py)"""
        from .merkle import MerkleTree
        return MerkleTree.commit_small(self, wait=wait)

    def evaluate_over_domain(self, domain):
        """DensePolynomial::evaluate_over_domain: a new vector of domain.size() evaluations of these coefficients."""
        if self.len == 0 or self.len > domain.size() or domain.field != self.field:
            raise ValueError("1 .. domain.size() coefficients of the domain's field")
        out = SmallDeviceVec(self.field, domain.size())
        check(lib().ark_hip_memcpy_d2d(out._p, self._p, self.nbytes), "ark_hip_memcpy_d2d")
        domain.fft_batch_in_place(out._p, 1, num_coeffs=self.len)
        return out

    def interpolate(self, domain):
        """Evaluations::interpolate: a new vector of the domain.size() coefficients."""
        if self.len != domain.size() or domain.field != self.field:
            raise ValueError("one evaluation per element of the domain")
        out = self.clone()
        domain.fft_batch_in_place(out._p, 1, inverse=True)
        return out


class SmallDeviceMatrix:
    """count columns of field words, column j at element offset j * stride of one device allocation."""

    def __init__(self, field, count, stride):
        self.field = small_field_id(field)
        self.count, self.stride = int(count), int(stride)
        self.vec = SmallDeviceVec.zeros(field, self.count * self.stride)

    @classmethod
    def from_host(cls, field, columns, stride=None):
        cols = np.ascontiguousarray(columns, dtype=small_field_dtype(field))
        if cols.ndim != 2:
            raise ValueError("columns as a [count, length] array")
        m = cls(field, cols.shape[0], cols.shape[1] if stride is None else stride)
        flat = np.zeros((m.count, m.stride), dtype=cols.dtype)
        flat[:, :cols.shape[1]] = cols
        m.vec.free()
        m.vec = SmallDeviceVec.from_host(field, flat.reshape(-1))
        return m

    def to_host(self, length=None):
        a = self.vec.to_host().reshape(self.count, self.stride)
        return a if length is None else a[:, :length].copy()

    def commit(self, n=None, wait=True):
        """MerkleTree.commit_small over the first n elements of every column (merkle.py); n = None: the whole stride"""
        from .merkle import MerkleTree
        return MerkleTree.commit_small(self, n=n, wait=wait)

    def fft_in_place(self, domain, num_coeffs=None, inverse=False):
        domain.fft_batch_in_place(self.vec._p, self.count, self.stride, num_coeffs, inverse)
        return self

    def low_degree_extend(self, domain, coset_domain):
        """Columns of evaluations over `domain` -> their evaluations over the larger `coset_domain`, in place: a batched inverse
        transform, then a batched forward transform that reads domain.size() coefficients per column."""
        if coset_domain.size() > self.stride or domain.size() > coset_domain.size():
            raise ValueError("the stride holds the larger domain")
        self.fft_in_place(domain, inverse=True)
        return self.fft_in_place(coset_domain, num_coeffs=domain.size())
