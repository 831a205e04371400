//! Device-resident vectors of curve points: elementwise scalar multiplication, elementwise sum, two-scalar fold.
//!
//! The reference has no batch form of `Projective *= ScalarField` (ec/src/models/short_weierstrass/group.rs:556-570 ->
//! `mul_bigint` -> `SWCurveConfig::mul_projective`, short_weierstrass/mod.rs:101-109 -> `double_and_add`,
//! ec/src/scalar_mul/mod.rs:29-60) or of `Projective += Projective` (group.rs:450-538): callers map them over a vector with
//! rayon, ~80 us per multiplication.  [`DevicePoints`] owns `ark_hip_malloc` memory and runs them where the points live
//! (`ark_hip_sw_mul_device`, `ark_hip_sw_add_device`, `ark_hip_sw_fold_device`: one lane per point): an SRS update
//! `P_i <- [tau^i] P_i` with the powers from a [`DeviceVec`], a round of an inner-product argument
//! `G' = [u^-1] G_lo + [u] G_hi`, a random linear combination of commitment vectors.
//!
//! Every operation is asynchronous on the library's stream of the current device and ordered with the others;
//! [`DevicePoints::to_vec`] waits.  Results are group elements: the Projective representative is not the reference's,
//! `into_affine()` agrees.  Mirrors: `ark_hip::DevicePoints` in include/ark_hip.hpp, `algebra_amd.DevicePoints` in Python.
use crate::device::{DeviceError, DeviceVec};
use crate::msm::HipServed;
use ark_ec::short_weierstrass::{Affine, Projective};
use ark_ff::FftField;
use ark_hip_sys as sys;
use ark_std::vec::Vec;
use core::ffi::{c_int, c_void};
use core::marker::PhantomData;
use core::mem::size_of;

fn rc(code: c_int) -> Result<(), DeviceError> {
    if code == 0 { Ok(()) } else { Err(DeviceError::Library(code)) }
}

/// `len` Projective points of the curve `P` in device memory (Jacobian x | y | z, identity z = 0).
pub struct DevicePoints<P: HipServed> {
    ptr: *mut c_void,
    len: usize,
    device: c_int,
    _p: PhantomData<P>,
}
// the pointer is device memory owned by this value; every access goes through the library, which locks its context
unsafe impl<P: HipServed> Send for DevicePoints<P> {}

impl<P: HipServed> DevicePoints<P>
where
    P::ScalarField: FftField,
{
    fn fe_bytes() -> Result<usize, DeviceError> {
        // bytes of one base-field element (ark_hip_curve_info's fe_words * 8)
        let fe: usize = match P::CURVE {
            sys::BN254_G1 => 32,
            sys::BLS12_381_G1 | sys::BLS12_377_G1 => 48,
            sys::BLS12_377_G2 | sys::BLS12_381_G2 => 96,
            _ => return Err(DeviceError::UnsupportedField),
        };
        if size_of::<Affine<P>>() != 2 * fe || size_of::<Projective<P>>() != 3 * fe || size_of::<P::ScalarField>() != 32 {
            return Err(DeviceError::UnsupportedField);
        }
        Ok(fe)
    }
    fn alloc(len: usize) -> Result<Self, DeviceError> {
        let fe = Self::fe_bytes()?;
        let mut ptr: *mut c_void = core::ptr::null_mut();
        if len != 0 {
            rc(unsafe { sys::ark_hip_malloc(len * 3 * fe, &mut ptr) })?;
        }
        Ok(Self { ptr, len, device: unsafe { sys::ark_hip_get_device() }, _p: PhantomData })
    }
    fn here(&self) -> Result<(), DeviceError> {
        if self.ptr.is_null() || unsafe { sys::ark_hip_get_device() } == self.device { Ok(()) } else { Err(DeviceError::WrongDevice) }
    }
    /// One upload of Projective points (synchronous: `x` may be dropped when this returns).
    pub fn from_projective(x: &[Projective<P>]) -> Result<Self, DeviceError> {
        let v = Self::alloc(x.len())?;
        rc(unsafe { sys::ark_hip_memcpy_h2d(v.ptr, x.as_ptr() as *const c_void, x.len() * size_of::<Projective<P>>()) })?;
        Ok(v)
    }
    /// One upload of Affine points (an SRS as it is stored), converted on the device: `[1] P_i` with the shared scalar one.
    pub fn from_affine(x: &[Affine<P>]) -> Result<Self, DeviceError> {
        let v = Self::alloc(x.len())?;
        if x.is_empty() {
            return Ok(v);
        }
        let bytes = x.len() * size_of::<Affine<P>>();
        let mut tmp: *mut c_void = core::ptr::null_mut();
        rc(unsafe { sys::ark_hip_malloc(bytes + 32, &mut tmp) })?;
        let one: [u64; 4] = [1, 0, 0, 0];
        let d_one = unsafe { (tmp as *mut u8).add(bytes) } as *mut c_void;   // 16-byte aligned: Affine sizes are multiples of 32
        let res = rc(unsafe { sys::ark_hip_memcpy_h2d(tmp, x.as_ptr() as *const c_void, bytes) })
            .and_then(|_| rc(unsafe { sys::ark_hip_memcpy_h2d(d_one, one.as_ptr() as *const c_void, 32) }))
            .and_then(|_| rc(unsafe { sys::ark_hip_sw_mul_device(P::CURVE, tmp, sys::ARK_HIP_FORM_AFFINE, d_one, 1, 0, x.len(), v.ptr) }));
        let freed = rc(unsafe { sys::ark_hip_free(tmp) });   // waits for the stream
        res.and(freed)?;
        Ok(v)
    }
    /// One download; waits for everything queued on the vector.
    pub fn to_vec(&self) -> Result<Vec<Projective<P>>, DeviceError> {
        self.here()?;
        let mut out: Vec<Projective<P>> = Vec::with_capacity(self.len);
        rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, self.ptr, self.len * size_of::<Projective<P>>()) })?;
        unsafe { out.set_len(self.len) };
        Ok(out)
    }
    pub fn try_clone(&self) -> Result<Self, DeviceError> {
        self.here()?;
        let v = Self::alloc(self.len)?;
        rc(unsafe { sys::ark_hip_memcpy_d2d(v.ptr, self.ptr, self.len * size_of::<Projective<P>>()) })?;
        Ok(v)
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
    pub fn as_device_ptr(&self) -> *const c_void {
        self.ptr
    }
    /// `self[i] *= scalars[i]` with the scalars already on the device (e.g. the powers of tau from `distribute_powers`).
    pub fn mul_assign_elementwise(&mut self, scalars: &DeviceVec<P::ScalarField>) -> Result<(), DeviceError> {
        self.here()?;
        if scalars.len() != self.len {
            return Err(DeviceError::Mismatch);
        }
        rc(unsafe {
            sys::ark_hip_sw_mul_device(P::CURVE, self.ptr, sys::ARK_HIP_FORM_PROJECTIVE, scalars.as_device_ptr(), self.len, 1, self.len, self.ptr)
        })
    }
    /// `self[i] *= k` for one scalar shared by every point.
    pub fn mul_assign_scalar(&mut self, k: &P::ScalarField) -> Result<(), DeviceError> {
        self.here()?;
        let s = DeviceVec::<P::ScalarField>::from_slice(core::slice::from_ref(k))?;
        rc(unsafe {
            sys::ark_hip_sw_mul_device(P::CURVE, self.ptr, sys::ARK_HIP_FORM_PROJECTIVE, s.as_device_ptr(), 1, 1, self.len, self.ptr)
        })
        // `s` is freed here: ark_hip_free waits for the stream
    }
    fn add_signed(&mut self, other: &Self, negate: c_int) -> Result<(), DeviceError> {
        self.here()?;
        other.here()?;
        if other.len != self.len {
            return Err(DeviceError::Mismatch);
        }
        rc(unsafe { sys::ark_hip_sw_add_device(P::CURVE, self.ptr, other.ptr, negate, self.len, self.ptr) })
    }
    /// `self[i] += other[i]`
    pub fn add_assign_elementwise(&mut self, other: &Self) -> Result<(), DeviceError> {
        self.add_signed(other, 0)
    }
    /// `self[i] -= other[i]`
    pub fn sub_assign_elementwise(&mut self, other: &Self) -> Result<(), DeviceError> {
        self.add_signed(other, 1)
    }
    /// `[a] self[i] + [b] hi[i]` on one joint doubling chain, as a new vector.
    pub fn fold(&self, hi: &Self, a: &P::ScalarField, b: &P::ScalarField) -> Result<Self, DeviceError> {
        self.here()?;
        hi.here()?;
        if hi.len != self.len {
            return Err(DeviceError::Mismatch);
        }
        let out = Self::alloc(self.len)?;
        rc(unsafe {
            sys::ark_hip_sw_fold_device(
                P::CURVE,
                self.ptr,
                hi.ptr,
                sys::ARK_HIP_FORM_PROJECTIVE,
                a as *const P::ScalarField as *const u64,
                b as *const P::ScalarField as *const u64,
                1,
                self.len,
                out.ptr,
            )
        })?;
        Ok(out)
    }
    /// `CurveGroup::normalize_batch` on the device and one download of the Affine points.
    pub fn normalize_to_vec(&self) -> Result<Vec<Affine<P>>, DeviceError> {
        self.here()?;
        let bytes = self.len * size_of::<Affine<P>>();
        let mut out: Vec<Affine<P>> = Vec::with_capacity(self.len);
        if self.len == 0 {
            return Ok(out);
        }
        let mut tmp: *mut c_void = core::ptr::null_mut();
        rc(unsafe { sys::ark_hip_malloc(bytes, &mut tmp) })?;
        let res = rc(unsafe { sys::ark_hip_sw_normalize_batch_device(P::CURVE, self.ptr, tmp, self.len) })
            .and_then(|_| rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, tmp, bytes) }));
        let freed = rc(unsafe { sys::ark_hip_free(tmp) });
        res.and(freed)?;
        unsafe { out.set_len(self.len) };
        Ok(out)
    }
}

impl<P: HipServed> Drop for DevicePoints<P> {
    fn drop(&mut self) {
        if !self.ptr.is_null() {
            unsafe {
                let cur = sys::ark_hip_get_device();
                if cur != self.device {
                    sys::ark_hip_set_device(self.device);
                }
                sys::ark_hip_free(self.ptr);
                if cur != self.device {
                    sys::ark_hip_set_device(cur);
                }
            }
        }
    }
}
