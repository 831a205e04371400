//! Device-resident vectors of a scalar field: `DensePolynomial` coefficients / `Evaluations` that stay in HBM.
//!
//! The reference's FFT callers chain transforms: `DensePolynomial::evaluate_over_domain`
//! (poly/src/polynomial/univariate/mod.rs:305-360: zero-extend + `fft_in_place` -> `Evaluations`), the pointwise
//! `+`, `-`, `*` of `Evaluations` over one domain (poly/src/evaluations/univariate/mod.rs:104-180) and
//! `Evaluations::interpolate` (mod.rs:40-50: `ifft_in_place` -> coefficients).  Through the `EvaluationDomain` hook every
//! link of such a chain crosses PCIe twice (2 x 128 MiB at 2^22: 5.3 ms around a 0.5 ms transform -- upload, transform and
//! download are serial by data dependence, so no pipelining removes them).  [`DeviceVec`] owns `ark_hip_malloc` memory;
//! with [`DeviceVec::evaluate_over_domain`], the `*Assign` operators of [`DeviceEvaluations`] and
//! [`DeviceEvaluations::interpolate`] the chain costs ONE upload per input and ONE download.
//!
//! Every operation is asynchronous on the library's stream of the current device and ordered with the others;
//! [`DeviceVec::to_vec`] waits.  A vector belongs to the device that was current when it was created: it is freed there, and
//! an operation attempted while another device is current returns `DeviceError::WrongDevice` instead of touching it.
//! Mirrors: `ark_hip::DeviceVec` in include/ark_hip.hpp (compiled and run by tests/test_gpu_cpp_mirror.py against the
//! oracle at 2^20), `algebra_amd.DeviceVec` in Python.
use ark_ff::FftField;
use ark_hip_sys as sys;
use ark_poly::domain::{EvaluationDomain, Radix2EvaluationDomain};
use ark_std::vec::Vec;
use core::ffi::{c_int, c_uint, c_void};
use core::marker::PhantomData;
use core::ops::{AddAssign, DivAssign, MulAssign, SubAssign};

/// Why a device operation did not happen; the data a `DeviceVec` holds is unchanged when an `Err` comes back.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum DeviceError {
    /// `F` is not one of the scalar fields the library serves, or its in-memory size is not 32 bytes.
    UnsupportedField,
    /// lengths / domains of the operands differ (the reference asserts `self.domain == other.domain`)
    Mismatch,
    /// the vector lives on another device than the calling thread's current one (`ark_hip_set_device`)
    WrongDevice,
    /// the library's return code (include/ark_hip.h `ARK_HIP_ERR_*`)
    Library(c_int),
}
fn rc(code: c_int) -> Result<(), DeviceError> {
    if code == 0 { Ok(()) } else { Err(DeviceError::Library(code)) }
}

pub struct DeviceVec<F: FftField> {
    ptr: *mut c_void,
    len: usize,
    cap: usize,
    device: c_int,
    field: c_int,
    /// a view into another vector's memory: it frees nothing
    view: bool,
    _f: PhantomData<F>,
}
// the pointer is device memory owned by this value; every access goes through the library, which locks its context
unsafe impl<F: FftField> Send for DeviceVec<F> {}

impl<F: FftField> DeviceVec<F> {
    fn field_id() -> Result<c_int, DeviceError> {
        if core::mem::size_of::<F>() != 32 || core::mem::align_of::<F>() != core::mem::align_of::<u64>() {
            return Err(DeviceError::UnsupportedField);
        }
        sys::fr_field_id::<F>().ok_or(DeviceError::UnsupportedField)
    }
    pub(crate) fn alloc(len: usize) -> Result<Self, DeviceError> {
        let field = Self::field_id()?;
        let mut ptr: *mut c_void = core::ptr::null_mut();
        if len != 0 {
            rc(unsafe { sys::ark_hip_malloc(len * 32, &mut ptr) })?;
        }
        let device = unsafe { sys::ark_hip_get_device() };
        Ok(Self { ptr, len, cap: len, device, field, view: false, _f: PhantomData })
    }
    /// `len` elements of `owner` from element `offset` on: a view, no copy, which frees nothing when dropped -- the halves of
    /// a product tree's level as the evaluations of a `DenseMultilinearExtension`.  `Err(Mismatch)` if it leaves its owner.
    ///
    /// # Safety
    /// The view must be dropped before its owner is dropped, resized or written through `&mut`.
    pub unsafe fn view(owner: &Self, offset: usize, len: usize) -> Result<Self, DeviceError> {
        owner.here()?;
        if offset > owner.len || len > owner.len - offset {
            return Err(DeviceError::Mismatch);
        }
        let ptr = if len == 0 { core::ptr::null_mut() } else { (owner.ptr as *mut u8).add(32 * offset) as *mut c_void };
        Ok(Self { ptr, len, cap: len, device: owner.device, field: owner.field, view: true, _f: PhantomData })
    }
    pub fn is_view(&self) -> bool {
        self.view
    }
    /// `vec![F::zero(); len]` on the device.
    pub fn zeros(len: usize) -> Result<Self, DeviceError> {
        let v = Self::alloc(len)?;
        rc(unsafe { sys::ark_hip_memset_device(v.ptr, 0, len * 32) })?;
        Ok(v)
    }
    /// One upload (synchronous: `x` may be dropped when this returns).
    pub fn from_slice(x: &[F]) -> Result<Self, DeviceError> {
        let v = Self::alloc(x.len())?;
        rc(unsafe { sys::ark_hip_memcpy_h2d(v.ptr, x.as_ptr() as *const c_void, x.len() * 32) })?;
        Ok(v)
    }
    /// One download; waits for everything queued on the vector.
    pub fn to_vec(&self) -> Result<Vec<F>, DeviceError> {
        self.here()?;
        let mut out: Vec<F> = Vec::with_capacity(self.len);
        rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, self.ptr, self.len * 32) })?;
        unsafe { out.set_len(self.len) }; // canonical Montgomery residues, the reference's own representation
        Ok(out)
    }
    pub fn try_clone(&self) -> Result<Self, DeviceError> {
        self.here()?;
        let v = Self::alloc(self.len)?;
        rc(unsafe { sys::ark_hip_memcpy_d2d(v.ptr, self.ptr, self.len * 32) })?;
        Ok(v)
    }
    pub fn len(&self) -> usize {
        self.len
    }
    pub(crate) fn field(&self) -> c_int {
        self.field
    }
    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
    /// For the `_device` entry points of `ark_hip_sys` (e.g. the scalars of an MSM straight from an inverse transform).
    pub fn as_device_ptr(&self) -> *const c_void {
        self.ptr
    }
    pub fn as_device_mut_ptr(&mut self) -> *mut c_void {
        self.ptr
    }
    /// `Vec::resize(new_len, F::zero())` (also truncates).
    pub fn resize_zeroed(&mut self, new_len: usize) -> Result<(), DeviceError> {
        self.here()?;
        if new_len > self.cap {
            let mut v = Self::alloc(new_len)?;
            rc(unsafe { sys::ark_hip_memcpy_d2d(v.ptr, self.ptr, self.len * 32) })?;
            v.len = self.len;
            core::mem::swap(self, &mut v); // the old allocation is freed by v's drop
        }
        let old = self.len;
        self.len = new_len;
        if new_len > old {
            rc(unsafe { sys::ark_hip_memset_device((self.ptr as *mut u8).add(old * 32) as *mut c_void, 0, (new_len - old) * 32) })?;
        }
        Ok(())
    }
    /// every operation runs on the stream of the thread's CURRENT device: refuse a vector that lives elsewhere
    pub(crate) fn here(&self) -> Result<(), DeviceError> {
        if self.ptr.is_null() || unsafe { sys::ark_hip_get_device() } == self.device { Ok(()) } else { Err(DeviceError::WrongDevice) }
    }
    fn same_len(&self, other: &Self) -> Result<(), DeviceError> {
        self.here()?;
        other.here()?;
        if self.len == other.len && self.field == other.field { Ok(()) } else { Err(DeviceError::Mismatch) }
    }
    pub fn add_assign_pointwise(&mut self, other: &Self) -> Result<(), DeviceError> {
        self.same_len(other)?;
        rc(unsafe { sys::ark_hip_fr_add_device(self.field, self.ptr, other.ptr, self.ptr, self.len) })
    }
    pub fn sub_assign_pointwise(&mut self, other: &Self) -> Result<(), DeviceError> {
        self.same_len(other)?;
        rc(unsafe { sys::ark_hip_fr_sub_device(self.field, self.ptr, other.ptr, self.ptr, self.len) })
    }
    pub fn mul_assign_pointwise(&mut self, other: &Self) -> Result<(), DeviceError> {
        self.same_len(other)?;
        rc(unsafe { sys::ark_hip_fr_mul_device(self.field, self.ptr, other.ptr, self.ptr, self.len) })
    }
    /// `Evaluations /= &Evaluations` (mod.rs:153-163): a zero divisor gives zero, as the reference's `batch_inversion` leaves
    /// zeros in place and `div_assign` multiplies by them
    pub fn div_assign_pointwise(&mut self, other: &Self) -> Result<(), DeviceError> {
        self.same_len(other)?;
        rc(unsafe { sys::ark_hip_fr_div_device(self.field, self.ptr, other.ptr, self.ptr, self.len) })
    }
    /// `ark_ff::batch_inversion` on the device (zeros stay zero)
    pub fn batch_inverse(&mut self) -> Result<(), DeviceError> {
        self.here()?;
        rc(unsafe { sys::ark_hip_fr_inverse_device(self.field, self.ptr, self.ptr, self.len) })
    }
    /// every element times `k` (`&DensePolynomial * F`, dense.rs:604-622)
    pub fn scale(&mut self, k: &F) -> Result<(), DeviceError> {
        self.here()?;
        let kl = sys::limbs(k);
        rc(unsafe { sys::ark_hip_fr_scale_device(self.field, self.ptr, kl.as_ptr(), self.ptr, self.len) })
    }
    pub fn negate(&mut self) -> Result<(), DeviceError> {
        self.here()?;
        rc(unsafe { sys::ark_hip_fr_neg_device(self.field, self.ptr, self.ptr, self.len) })
    }
    /// `DensePolynomial::evaluate_over_domain` (polynomial/univariate/mod.rs:305-360) for coefficients already on the
    /// device: zero-extension and transform in place; at most size/4 coefficients take the degree-aware path
    /// (radix2/mod.rs:141).  More coefficients than the domain holds is the reference's folding case (mod.rs:330-352):
    /// `Err(Mismatch)`, fold on the host first.
    pub fn evaluate_over_domain(mut self, domain: Radix2EvaluationDomain<F>) -> Result<DeviceEvaluations<F>, DeviceError> {
        let have = self.len;
        if have > domain.size() {
            return Err(DeviceError::Mismatch);
        }
        self.resize_zeroed(domain.size())?;
        let d = raw_domain(&domain);
        rc(unsafe { sys::ark_hip_fft_in_place_degree_aware_device(self.field, &d, self.ptr, have) })?;
        Ok(DeviceEvaluations { evals: self, domain })
    }
    /// `DensePolynomial::evaluate` (dense.rs:42-92) on the device; waits for the one element that comes back.
    pub fn evaluate(&self, point: &F) -> Result<F, DeviceError> {
        self.here()?;
        let z = sys::limbs(point);
        let mut out = [0u64; 4];
        rc(unsafe { sys::ark_hip_poly_evaluate_device(self.field, self.ptr, self.len, z.as_ptr(), out.as_mut_ptr()) })?;
        Ok(sys::from_limbs::<F>(&out))
    }
    /// `(quotient, remainder)` of the division by `x - z` (`divide_with_q_and_r` for a degree-1 divisor,
    /// polynomial/univariate/mod.rs:145-159): the KZG witness polynomial and `p(z)`.  The quotient overwrites this vector,
    /// which becomes one element shorter: no second buffer, no host copy.
    pub fn divide_by_linear(mut self, z: &F) -> Result<(Self, F), DeviceError> {
        self.here()?;
        let zl = sys::limbs(z);
        let mut rem = [0u64; 4];
        rc(unsafe { sys::ark_hip_poly_divide_linear_device(self.field, self.ptr, self.len, zl.as_ptr(), self.ptr, rem.as_mut_ptr()) })?;
        self.len = self.len.saturating_sub(1);
        Ok((self, sys::from_limbs::<F>(&rem)))
    }
    /// `DensePolynomial::divide_by_vanishing_poly` (dense.rs:168-211): `(quotient, remainder)`; as in the reference only the
    /// size of the domain enters.
    pub fn divide_by_vanishing_poly(&self, domain: &Radix2EvaluationDomain<F>) -> Result<(Self, Self), DeviceError> {
        self.here()?;
        let m = domain.size();
        let q = Self::alloc(self.len.saturating_sub(m))?;
        let r = Self::alloc(core::cmp::min(self.len, m))?;
        rc(unsafe { sys::ark_hip_poly_divide_by_vanishing_device(self.field, m, self.ptr, self.len, q.ptr, r.ptr) })?;
        Ok((q, r))
    }
    /// `sum_i self[i] * other[i]`; waits for the one element that comes back.
    pub fn inner_product(&self, other: &Self) -> Result<F, DeviceError> {
        self.same_len(other)?;
        let mut out = [0u64; 4];
        rc(unsafe { sys::ark_hip_fr_inner_product_device(self.field, self.ptr, other.ptr, self.len, out.as_mut_ptr()) })?;
        Ok(sys::from_limbs::<F>(&out))
    }
    /// `(vector, total)`: `out[i] = prod_{j <= i} self[j]` (`exclusive`: `j < i`, `out[0] = 1`) and the product of everything;
    /// waits for it.
    pub fn prefix_product(&self, exclusive: bool) -> Result<(Self, F), DeviceError> {
        self.here()?;
        let out = Self::alloc(self.len)?;
        let mut total = [0u64; 4];
        rc(unsafe { sys::ark_hip_fr_prefix_product_device(self.field, self.ptr, self.len, exclusive as i32, out.ptr, total.as_mut_ptr()) })?;
        Ok((out, sys::from_limbs::<F>(&total)))
    }
    /// `(vector, total)`: `out[i] = sum_{j <= i} self[j]` (`exclusive`: `j < i`, `out[0] = 0`) and the sum of everything.
    pub fn prefix_sum(&self, exclusive: bool) -> Result<(Self, F), DeviceError> {
        self.here()?;
        let out = Self::alloc(self.len)?;
        let mut total = [0u64; 4];
        rc(unsafe { sys::ark_hip_fr_prefix_sum_device(self.field, self.ptr, self.len, exclusive as i32, out.ptr, total.as_mut_ptr()) })?;
        Ok((out, sys::from_limbs::<F>(&total)))
    }
    /// `(z, last)` with `self` the numerators: `z[0] = 1`, `z[i+1] = z[i] * self[i] / den[i]` and
    /// `last = prod_j self[j] / den[j]`, the value that is one for a valid permutation; waits for it.  From the first zero
    /// denominator on the outputs are zero, as `/=` divides.
    pub fn prefix_ratio(&self, den: &Self) -> Result<(Self, F), DeviceError> {
        self.same_len(den)?;
        let out = Self::alloc(self.len)?;
        let mut last = [0u64; 4];
        rc(unsafe { sys::ark_hip_fr_prefix_ratio_device(self.field, self.ptr, den.ptr, self.len, out.ptr, last.as_mut_ptr()) })?;
        Ok((out, sys::from_limbs::<F>(&last)))
    }
    /// `EvaluationDomain::evaluate_all_lagrange_coefficients` (poly/src/domain/mod.rs:157-222) as a device vector: with
    /// [`DeviceVec::inner_product`] and the evaluations of `P` over `domain`, that is `P(tau)`.
    pub fn lagrange_coefficients(domain: &Radix2EvaluationDomain<F>, tau: &F) -> Result<Self, DeviceError> {
        let v = Self::alloc(domain.size())?;
        let d = raw_domain(domain);
        let t = sys::limbs(tau);
        rc(unsafe { sys::ark_hip_domain_lagrange_coefficients_device(v.field, &d, t.as_ptr(), v.ptr) })?;
        Ok(v)
    }
    /// `out[i] = self[(i + k) mod len]`, `k` any `i64`: the one-term case of [`SumOfProducts`], a product-free copy.
    pub fn rotate(&self, k: i64) -> Result<Self, DeviceError> {
        let mut s = SumOfProducts::new(self.len);
        s.add_product(&[(self, k)], None)?;
        s.evaluate()
    }
}
impl<F: FftField> Drop for DeviceVec<F> {
    fn drop(&mut self) {
        if self.ptr.is_null() || self.view {
            return;
        }
        unsafe {
            let cur = sys::ark_hip_get_device();
            if self.device >= 0 && cur != self.device {
                sys::ark_hip_set_device(self.device);
            }
            let r = sys::ark_hip_free(self.ptr); // waits for the work queued on it
            debug_assert_eq!(r, 0);
            if self.device >= 0 && cur != self.device && cur >= 0 {
                sys::ark_hip_set_device(cur);
            }
        }
    }
}

/// The C mirror of the domain (include/ark_hip.h `ark_hip_radix2_domain`) from the reference's public fields.
fn raw_domain<F: FftField>(d: &Radix2EvaluationDomain<F>) -> sys::ark_hip_radix2_domain {
    sys::ark_hip_radix2_domain {
        size: d.size,
        log_size_of_group: d.log_size_of_group,
        _pad: 0,
        size_as_field_element: sys::limbs(&d.size_as_field_element),
        size_inv: sys::limbs(&d.size_inv),
        group_gen: sys::limbs(&d.group_gen),
        group_gen_inv: sys::limbs(&d.group_gen_inv),
        offset: sys::limbs(&d.offset),
        offset_inv: sys::limbs(&d.offset_inv),
        offset_pow_size: sys::limbs(&d.offset_pow_size),
    }
}

/// A `rows x cols` matrix over `F` in CSR form, resident on the device: a constraint matrix of an
/// R1CS / CCS instance.  Built once per circuit from host slices, which the library validates and copies; `with_transpose`
/// also keeps `M^T` (stable order), which [`CsrMatrix::mul_t`] needs.
pub struct CsrMatrix<F: FftField> {
    handle: *mut sys::ark_hip_fr_csr,
    rows: usize,
    cols: usize,
    _f: PhantomData<F>,
}
unsafe impl<F: FftField> Send for CsrMatrix<F> {}
/// `ark_hip_csr_plan`: how a handle with this `row_ptr` is cut into work (host only).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct CsrPlan {
    pub tile: c_int,
    pub max_rows: c_int,
    pub blocks: usize,
    pub long_rows: usize,
    pub long_chunks: usize,
}
pub fn csr_plan(row_ptr: &[u32]) -> Result<CsrPlan, DeviceError> {
    if row_ptr.is_empty() {
        return Err(DeviceError::Mismatch);
    }
    let mut p = CsrPlan { tile: 0, max_rows: 0, blocks: 0, long_rows: 0, long_chunks: 0 };
    rc(unsafe { sys::ark_hip_csr_plan(row_ptr.len() - 1, row_ptr.as_ptr(), &mut p.tile, &mut p.max_rows, &mut p.blocks, &mut p.long_rows, &mut p.long_chunks) })?;
    Ok(p)
}
impl<F: FftField> CsrMatrix<F> {
    /// `row_ptr`: `rows + 1` entries; `col_idx` and `vals`: one per nonzero.  Every index is checked by the library on the host.
    pub fn new(rows: usize, cols: usize, row_ptr: &[u32], col_idx: &[u32], vals: &[F], with_transpose: bool) -> Result<Self, DeviceError> {
        let field = DeviceVec::<F>::field_id()?;
        if row_ptr.len() != rows + 1 || col_idx.len() != vals.len() {
            return Err(DeviceError::Mismatch);
        }
        let mut handle: *mut sys::ark_hip_fr_csr = core::ptr::null_mut();
        let flags = if with_transpose { sys::ARK_HIP_CSR_WITH_TRANSPOSE } else { 0 };
        rc(unsafe { sys::ark_hip_fr_csr_create(field, rows, cols, row_ptr.as_ptr(), col_idx.as_ptr(), vals.as_ptr() as *const u64, vals.len(), flags, &mut handle) })?;
        Ok(Self { handle, rows, cols, _f: PhantomData })
    }
    pub fn rows(&self) -> usize {
        self.rows
    }
    pub fn cols(&self) -> usize {
        self.cols
    }
    fn product(&self, transpose: c_int, x: &DeviceVec<F>, n_out: usize) -> Result<DeviceVec<F>, DeviceError> {
        x.here()?;
        let out = DeviceVec::<F>::alloc(n_out)?;
        rc(unsafe { sys::ark_hip_fr_csr_mul_device(self.handle, transpose, x.ptr, x.len, out.ptr, out.len) })?;
        Ok(out)
    }
    /// `y = M x` (`x`: `cols` elements, `y`: `rows`); asynchronous.
    pub fn mul(&self, x: &DeviceVec<F>) -> Result<DeviceVec<F>, DeviceError> {
        self.product(0, x, self.rows)
    }
    /// `y = M^T x` (`x`: `rows` elements, `y`: `cols`); needs `with_transpose`.
    pub fn mul_t(&self, x: &DeviceVec<F>) -> Result<DeviceVec<F>, DeviceError> {
        self.product(1, x, self.cols)
    }
    /// `u^T M v`; with `u = eq(rx, .)`, `v = eq(ry, .)` the value of the matrix's sparse multilinear extension at `(rx, ry)`.
    pub fn bilinear(&self, u: &DeviceVec<F>, v: &DeviceVec<F>) -> Result<F, DeviceError> {
        u.inner_product(&self.mul(v)?)
    }
}
impl<F: FftField> Drop for CsrMatrix<F> {
    fn drop(&mut self) {
        unsafe { sys::ark_hip_fr_csr_free(self.handle) };
    }
}

/// `ARK_HIP_SOP_MAX_COLUMNS`, `_MAX_TERMS`, `_MAX_DEGREE` of include/ark_hip.h
pub const SOP_MAX_COLUMNS: usize = sys::ARK_HIP_SOP_MAX_COLUMNS as usize;
pub const SOP_MAX_TERMS: usize = sys::ARK_HIP_SOP_MAX_TERMS as usize;
pub const SOP_MAX_DEGREE: usize = sys::ARK_HIP_SOP_MAX_DEGREE as usize;
/// `ark_hip_fr_sum_of_products_plan`: workgroups of 256 lanes and the rows one lane walks for `n` rows (host only).
pub fn sum_of_products_plan(n: usize) -> Result<(c_int, c_int), DeviceError> {
    let (mut blocks, mut rows_per_lane) = (0, 0);
    rc(unsafe { sys::ark_hip_fr_sum_of_products_plan(n, &mut blocks, &mut rows_per_lane) })?;
    Ok((blocks, rows_per_lane))
}
/// The gate expression of a univariate (Plonk-style) prover on device vectors: a sum of products of
/// columns, each factor read at a rotation, `out[i] = c0 + sum_j c_j prod_q col_jq[(i + rot_jq) mod n]`, in one call of
/// `ark_hip_fr_sum_of_products_device` -- the univariate counterpart of `ListOfProducts`.  The columns are borrowed for the
/// expression's lifetime; a vector used in several products, or several times in one, is one shared column.
pub struct SumOfProducts<'a, F: FftField> {
    n: usize,
    columns: Vec<&'a DeviceVec<F>>,
    lens: Vec<c_uint>,
    flat: Vec<c_uint>,
    rotations: Vec<i64>,
    coeffs: Vec<F>,
    constant: Option<F>,
}
impl<'a, F: FftField> SumOfProducts<'a, F> {
    pub fn new(n: usize) -> Self {
        Self { n, columns: Vec::new(), lens: Vec::new(), flat: Vec::new(), rotations: Vec::new(), coeffs: Vec::new(), constant: None }
    }
    /// Adds `coefficient * prod factors` (`None`: one, which costs no product); a factor is a column and its rotation.
    /// `Err(Mismatch)` for a length that differs from the expression's or a limit exceeded; nothing is added then.
    pub fn add_product(&mut self, factors: &[(&'a DeviceVec<F>, i64)], coefficient: Option<F>) -> Result<(), DeviceError> {
        if factors.is_empty() || factors.len() > SOP_MAX_DEGREE || self.lens.len() >= SOP_MAX_TERMS {
            return Err(DeviceError::Mismatch);
        }
        let mut columns = self.columns.clone();
        let mut idx = Vec::with_capacity(factors.len());
        for (v, _) in factors {
            v.here()?;
            if v.len != self.n {
                return Err(DeviceError::Mismatch);
            }
            let at = match columns.iter().position(|c| c.ptr == v.ptr) {
                Some(i) => i,
                None => {
                    columns.push(v);
                    columns.len() - 1
                }
            };
            idx.push(at as c_uint);
        }
        if columns.len() > SOP_MAX_COLUMNS {
            return Err(DeviceError::Mismatch);
        }
        self.columns = columns;
        self.lens.push(idx.len() as c_uint);
        self.flat.extend(idx);
        self.rotations.extend(factors.iter().map(|(_, r)| *r));
        self.coeffs.push(coefficient.unwrap_or(F::ONE));
        Ok(())
    }
    pub fn set_constant(&mut self, c0: Option<F>) {
        self.constant = c0;
    }
    /// The expression's `n` rows; asynchronous.
    pub fn evaluate(&self) -> Result<DeviceVec<F>, DeviceError> {
        let out = DeviceVec::<F>::alloc(self.n)?;
        self.run(out.ptr)?;
        Ok(out)
    }
    /// The same over `out`, which may be one of the columns if every factor reads that column at a rotation that is 0 mod
    /// `n` -- by raw pointer, since the column is borrowed: `out` must hold `n` elements of this device.
    ///
    /// # Safety
    /// `out` is device memory of `n` elements owned by the caller.
    pub unsafe fn evaluate_into(&self, out: *mut c_void) -> Result<(), DeviceError> {
        self.run(out)
    }
    fn run(&self, out: *mut c_void) -> Result<(), DeviceError> {
        if self.lens.is_empty() {
            return Err(DeviceError::Mismatch);
        }
        if self.n == 0 {
            return Ok(());
        }
        let field = DeviceVec::<F>::field_id()?;
        let ptrs: Vec<*const c_void> = self.columns.iter().map(|c| c.ptr as *const c_void).collect();
        let c0 = self.constant.as_ref().map(sys::limbs);
        rc(unsafe {
            sys::ark_hip_fr_sum_of_products_device(field, ptrs.as_ptr(), ptrs.len() as c_uint, self.n, self.lens.as_ptr(), self.flat.as_ptr(),
                                                   self.rotations.as_ptr(), self.coeffs.as_ptr() as *const u64, self.lens.len() as c_uint,
                                                   c0.as_ref().map_or(core::ptr::null(), |c| c.as_ptr()), out)
        })
    }
}

/// `Evaluations<F, Radix2EvaluationDomain<F>>` resident on the device (evaluations/univariate/mod.rs:18-29).
pub struct DeviceEvaluations<F: FftField> {
    pub evals: DeviceVec<F>,
    pub domain: Radix2EvaluationDomain<F>,
}
impl<F: FftField> DeviceEvaluations<F> {
    /// `Evaluations::from_vec_and_domain` for values already on the device.
    pub fn from_device_vec_and_domain(evals: DeviceVec<F>, domain: Radix2EvaluationDomain<F>) -> Result<Self, DeviceError> {
        if evals.len() != domain.size() { Err(DeviceError::Mismatch) } else { Ok(Self { evals, domain }) }
    }
    /// `Evaluations::interpolate` (mod.rs:47-50): the `domain.size()` coefficients, still on the device.  The reference
    /// then drops leading zeros (`DensePolynomial::from_coefficients_vec`): do that on the host after `to_vec()`.
    pub fn interpolate(mut self) -> Result<DeviceVec<F>, DeviceError> {
        self.evals.here()?;
        let d = raw_domain(&self.domain);
        rc(unsafe { sys::ark_hip_ifft_in_place_device(self.evals.field, &d, self.evals.ptr) })?;
        Ok(self.evals)
    }
    fn same_domain(&self, other: &Self) {
        assert_eq!(self.domain, other.domain, "domains are unequal"); // the reference's assertion, same message
    }
}
// `Evaluations op= &Evaluations` (mod.rs:104-180).  The reference's operators cannot fail; a device error here panics
// with the library's code (the fallible forms are the `*_assign_pointwise` methods of `DeviceVec`).
impl<'a, F: FftField> AddAssign<&'a DeviceEvaluations<F>> for DeviceEvaluations<F> {
    fn add_assign(&mut self, other: &'a DeviceEvaluations<F>) {
        self.same_domain(other);
        self.evals.add_assign_pointwise(&other.evals).expect("ark-hip: pointwise add on the device");
    }
}
impl<'a, F: FftField> SubAssign<&'a DeviceEvaluations<F>> for DeviceEvaluations<F> {
    fn sub_assign(&mut self, other: &'a DeviceEvaluations<F>) {
        self.same_domain(other);
        self.evals.sub_assign_pointwise(&other.evals).expect("ark-hip: pointwise sub on the device");
    }
}
impl<'a, F: FftField> MulAssign<&'a DeviceEvaluations<F>> for DeviceEvaluations<F> {
    fn mul_assign(&mut self, other: &'a DeviceEvaluations<F>) {
        self.same_domain(other);
        self.evals.mul_assign_pointwise(&other.evals).expect("ark-hip: pointwise mul on the device");
    }
}
impl<'a, F: FftField> DivAssign<&'a DeviceEvaluations<F>> for DeviceEvaluations<F> {
    fn div_assign(&mut self, other: &'a DeviceEvaluations<F>) {
        self.same_domain(other);
        self.evals.div_assign_pointwise(&other.evals).expect("ark-hip: pointwise division on the device");
    }
}
