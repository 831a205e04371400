"""Point vectors kept on the device: `out[i] = [k_i] P_i`, `P += Q`, `P -= Q`, `[a] Lo + [b] Hi`.

The reference has no batch form: callers map `Projective *= ScalarField` (ec/src/models/short_weierstrass/group.rs:556-570 ->
mul_bigint -> SWCurveConfig::mul_projective / mul_affine, short_weierstrass/mod.rs:101-109 -> double_and_add(_affine),
ec/src/scalar_mul/mod.rs:29-60) and `Projective += Projective` (group.rs:450-538) over a vector with rayon.  `DevicePoints` runs
them where the points live (ark_hip_sw_mul_device / _add_device / _fold_device: one lane per point, csrc/pointvec.cuh): an SRS
update `P_i <- [tau^i] P_i`, a round of an inner-product argument `G' = [u^-1] G_lo + [u] G_hi`, a random linear combination of
commitment vectors -- without downloading the points."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib
from .poly import DeviceVec

FORM_AFFINE, FORM_PROJECTIVE = 0, 1


def _scalar4(k):
    return np.ascontiguousarray(k, dtype=np.uint64).reshape(4)


class DevicePoints:
    """A vector of points of one curve owned by the library's allocator on the current GPU -- the Python mirror of
    `ark_hip::DevicePoints` (Rust: rust/ark-hip/src/points.rs, C++: include/ark_hip.hpp).  Affine (x | y, identity (0, 0)) as
    uploaded bases are, or Projective (Jacobian x | y | z, identity z = 0) as every operation's result is.  numpy in
    (`from_host`), numpy out (`to_host`); asynchronous on the library's stream in between, `to_host` and `msm` wait."""

    def __init__(self, curve, length, affine=False):
        self.curve = cv.curve_id(curve)
        self.len = int(length)
        self.affine = bool(affine)
        self.ptr = C.c_void_p(0)
        if self.len:
            check(lib().ark_hip_malloc(self.len * self._stride(), C.byref(self.ptr)), "ark_hip_malloc")

    def _words(self, affine=None):
        affine = self.affine if affine is None else affine
        return cv.affine_words(self.curve) if affine else cv.projective_words(self.curve)

    def _stride(self, affine=None):
        return 8 * self._words(affine)

    @property
    def form(self):
        return FORM_AFFINE if self.affine else FORM_PROJECTIVE

    def data_ptr(self):
        return self.ptr.value or 0

    @classmethod
    def from_host(cls, curve, points, affine=True):
        cid = cv.curve_id(curve)
        words = cv.affine_words(cid) if affine else cv.projective_words(cid)
        a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
        v = cls(cid, a.shape[0], affine)
        if v.len:
            check(lib().ark_hip_memcpy_h2d(v.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes), "ark_hip_memcpy_h2d")
        return v

    def to_host(self):
        out = np.empty((self.len, self._words()), dtype=np.uint64)
        if self.len:
            check(lib().ark_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes), "ark_hip_memcpy_d2h")
        return out

    def clone(self):
        v = DevicePoints(self.curve, self.len, self.affine)
        if self.len:
            check(lib().ark_hip_memcpy_d2d(v.ptr, self.ptr, self.len * self._stride()), "ark_hip_memcpy_d2d")
        return v

    def free(self):
        if self.ptr and self.ptr.value:
            check(lib().ark_hip_free(self.ptr), "ark_hip_free")
            self.ptr = C.c_void_p(0)
            self.len = 0

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def __len__(self):
        return self.len

    def _out(self, in_place):
        """where a Projective result goes: this vector (Projective only: an Affine element is shorter) or a new one"""
        if in_place:
            if self.affine:
                raise ValueError("an Affine vector cannot take a Projective result in place")
            return self
        return DevicePoints(self.curve, self.len, affine=False)

    def mul(self, scalars, montgomery=True, in_place=False):
        """out[i] = [k_i] P_i.  scalars: a DeviceVec of len(self) Fr elements (it never leaves the device), a host array
        [len(self), 4], or ONE scalar (4 words) shared by every point.  montgomery: Fr elements in Montgomery form; False:
        canonical BigInt<4>, every 256-bit value multiplied exactly.  Returns a Projective vector (self with in_place)."""
        keep = None
        if isinstance(scalars, DeviceVec):
            if cv.field_id(cv.scalar_field(self.curve)) != scalars.field:
                raise ValueError("scalars of another field")
            ns, sp = len(scalars), scalars.ptr
        else:
            a = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            keep = DeviceVec.from_host(cv.scalar_field(self.curve), a)
            ns, sp = a.shape[0], keep.ptr
        if ns != 1 and ns != self.len:
            raise ValueError("one scalar, or one per point")
        out = self._out(in_place)
        if self.len:
            check(lib().ark_hip_sw_mul_device(self.curve, self.ptr, self.form, sp, ns, int(montgomery), self.len, out.ptr),
                  "ark_hip_sw_mul_device")
        if keep is not None:
            keep.free()   # ark_hip_free waits for the stream
        return out

    def _same(self, other):
        if other.curve != self.curve or other.len != self.len:
            raise ValueError("vectors of unequal length or curve")
        if self.affine or other.affine:
            raise ValueError("elementwise addition takes Projective vectors")

    def __iadd__(self, other):
        self._same(other)
        if self.len:
            check(lib().ark_hip_sw_add_device(self.curve, self.ptr, other.ptr, 0, self.len, self.ptr), "ark_hip_sw_add_device")
        return self

    def __isub__(self, other):
        self._same(other)
        if self.len:
            check(lib().ark_hip_sw_add_device(self.curve, self.ptr, other.ptr, 1, self.len, self.ptr), "ark_hip_sw_add_device")
        return self

    def fold(self, hi, a, b, montgomery=True, in_place=False):
        """out[i] = [a] self[i] + [b] hi[i] on one joint doubling chain; both vectors in the same form.  Returns a
        Projective vector (self with in_place)."""
        if hi.curve != self.curve or hi.len != self.len or hi.affine != self.affine:
            raise ValueError("vectors of unequal length, curve or form")
        a, b = _scalar4(a), _scalar4(b)
        out = self._out(in_place)
        if self.len:
            check(lib().ark_hip_sw_fold_device(self.curve, self.ptr, hi.ptr, self.form, a.ctypes.data_as(C.c_void_p),
                                               b.ctypes.data_as(C.c_void_p), int(montgomery), self.len, out.ptr),
                  "ark_hip_sw_fold_device")
        return out

    def normalize(self):
        """CurveGroup::normalize_batch (group.rs:302-319) on the device: a new Affine vector, the form the MSM entries take
        their bases in (`msm`, or `data_ptr()` for ark_hip_msm_sw_device)."""
        if self.affine:
            return self.clone()
        out = DevicePoints(self.curve, self.len, affine=True)
        if self.len:
            check(lib().ark_hip_sw_normalize_batch_device(self.curve, self.ptr, out.ptr, self.len), "ark_hip_sw_normalize_batch_device")
        return out

    def msm(self, scalars, montgomery=True):
        """sum_i [k_i] self[i] through the device MSM entry (Affine vectors: `normalize()` first); scalars as for `mul`, one
        per point.  Returns the Projective sum as numpy words."""
        if not self.affine:
            raise ValueError("the MSM takes Affine bases: normalize() first")
        keep = None
        if isinstance(scalars, DeviceVec):
            ns, sp = len(scalars), scalars.ptr
        else:
            a = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            keep = DeviceVec.from_host(cv.scalar_field(self.curve), a)
            ns, sp = a.shape[0], keep.ptr
        if ns != self.len:
            raise ValueError("one scalar per point")
        out = np.zeros(cv.projective_words(self.curve), dtype=np.uint64)
        check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
        check(lib().ark_hip_msm_sw_device(self.curve, self.ptr, sp, self.len, int(montgomery), out.ctypes.data_as(C.c_void_p)),
              "ark_hip_msm_sw_device")
        if keep is not None:
            keep.free()
        return out
