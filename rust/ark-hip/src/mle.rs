//! `DenseMultilinearExtension` resident on the device: the mirror of ark-poly's type of that name
//! (poly/src/evaluations/multivariate/multilinear/dense.rs).  The table of `2^num_vars` evaluations is a [`DeviceVec`]:
//! committing to it is an MSM with Montgomery scalars on `evaluations().as_device_ptr()`, and `fix_variables` / `evaluate`
//! bind its variables where the table lies.  Index bit 0 is the first variable, as in the reference.
use crate::device::{DeviceError, DeviceVec};
use crate::msm::HipServed;
use ark_ec::short_weierstrass::{Affine, Projective};
use ark_ff::FftField;
use ark_hip_sys as sys;
use ark_std::vec::Vec;
use core::ffi::{c_uint, c_void};

pub struct DeviceMultilinearExtension<F: FftField> {
    num_vars: usize,
    evals: DeviceVec<F>,
}
/// the reference's name for it
pub type DenseMultilinearExtension<F> = DeviceMultilinearExtension<F>;

/// What [`DeviceMultilinearExtension::quotients`] returns: `f(point)` and the quotients `q_i` of
/// `f(x) - f(point) = sum_i (x_i - point_i) q_i(x_{i+1}, ..)`, all in one device vector; `q_i` is the view of
/// `segment_len(i)` elements from `segment_offset(i)` on.
pub struct Quotients<F: FftField> {
    pub value: F,
    num_vars: usize,
    all: DeviceVec<F>,
}
impl<F: FftField> Quotients<F> {
    pub fn num_vars(&self) -> usize {
        self.num_vars
    }
    pub fn segment_offset(&self, i: usize) -> usize {
        (1usize << self.num_vars) - (1usize << (self.num_vars - i))
    }
    pub fn segment_len(&self, i: usize) -> usize {
        1usize << (self.num_vars - 1 - i)
    }
    /// device pointer of `q_i`: a scalar vector for the MSM's device entries (Montgomery form)
    pub fn segment_ptr(&self, i: usize) -> *const c_void {
        unsafe { (self.all.as_device_ptr() as *const u8).add(32 * self.segment_offset(i)) as *const c_void }
    }
    pub fn segment_to_vec(&self, i: usize) -> Result<Vec<F>, DeviceError> {
        let n = self.segment_len(i);
        let mut out: Vec<F> = Vec::with_capacity(n);
        rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, self.segment_ptr(i), n * 32) })?;
        unsafe { out.set_len(n) };
        Ok(out)
    }
    pub fn all(&self) -> &DeviceVec<F> {
        &self.all
    }
}

/// What [`DeviceMultilinearExtension::product_tree`] returns: the product of all entries and the binary product tree pairing
/// over the LAST variable, all in one device vector of `2^num_vars - 1` elements; level `j` (`1 <= j <= num_vars`) is the
/// `level_len(j)` elements from `level_offset(j)` on, its element `i` the product of elements `i` and `i + level_len(j)` of
/// level `j - 1` (level 0: the table).  The last element is the product.
pub struct ProductTree<F: FftField> {
    pub product: F,
    num_vars: usize,
    all: DeviceVec<F>,
}
impl<F: FftField> ProductTree<F> {
    pub fn num_vars(&self) -> usize {
        self.num_vars
    }
    pub fn level_offset(&self, j: usize) -> usize {
        (1usize << self.num_vars) - (2usize << (self.num_vars - j))
    }
    pub fn level_len(&self, j: usize) -> usize {
        1usize << (self.num_vars - j)
    }
    pub fn level_ptr(&self, j: usize) -> *const c_void {
        unsafe { (self.all.as_device_ptr() as *const u8).add(32 * self.level_offset(j)) as *const c_void }
    }
    pub fn level_to_vec(&self, j: usize) -> Result<Vec<F>, DeviceError> {
        let n = self.level_len(j);
        let mut out: Vec<F> = Vec::with_capacity(n);
        rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, self.level_ptr(j), n * 32) })?;
        unsafe { out.set_len(n) };
        Ok(out)
    }
    pub fn all(&self) -> &DeviceVec<F> {
        &self.all
    }
}

/// The launches of [`DeviceMultilinearExtension::product_tree`] as `ark_hip_mle_product_tree_plan` reports them: per run of
/// launches of one kernel variant, (levels, log2 of the chunks of 64 outputs one wave walks).  Host only.
pub fn product_tree_plan(num_vars: usize) -> Result<Vec<(usize, usize)>, DeviceError> {
    let (mut passes, mut widths, mut groups) = (0 as core::ffi::c_int, [0 as core::ffi::c_int; 8], [0 as core::ffi::c_int; 8]);
    rc(unsafe { sys::ark_hip_mle_product_tree_plan(num_vars as c_uint, &mut passes, widths.as_mut_ptr(), groups.as_mut_ptr()) })?;
    Ok((0..passes as usize).map(|p| (widths[p] as usize, groups[p] as usize)).collect())
}

/// What [`DeviceMultilinearExtension::fraction_tree`] returns: the root `(P, Q)` of the sum of fractions `num[b] / den[b]` and
/// the two trees that add them, pairing over the LAST variable (`N = n0 d1 + n1 d0`, `D = d0 d1`), each in one device vector
/// of `2^num_vars - 1` elements in [`ProductTree`]'s layout.  Nothing is inverted.
pub struct FractionTree<F: FftField> {
    pub root: (F, F),
    num_vars: usize,
    num: DeviceVec<F>,
    den: DeviceVec<F>,
}
impl<F: FftField> FractionTree<F> {
    pub fn num_vars(&self) -> usize {
        self.num_vars
    }
    pub fn level_offset(&self, j: usize) -> usize {
        (1usize << self.num_vars) - (2usize << (self.num_vars - j))
    }
    pub fn level_len(&self, j: usize) -> usize {
        1usize << (self.num_vars - j)
    }
    /// the numerator tree and the denominator tree
    pub fn num(&self) -> &DeviceVec<F> {
        &self.num
    }
    pub fn den(&self) -> &DeviceVec<F> {
        &self.den
    }
    fn level_to_vec(&self, all: &DeviceVec<F>, j: usize) -> Result<Vec<F>, DeviceError> {
        let n = self.level_len(j);
        let mut out: Vec<F> = Vec::with_capacity(n);
        let src = unsafe { (all.as_device_ptr() as *const u8).add(32 * self.level_offset(j)) as *const c_void };
        rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, src, n * 32) })?;
        unsafe { out.set_len(n) };
        Ok(out)
    }
    pub fn num_level_to_vec(&self, j: usize) -> Result<Vec<F>, DeviceError> {
        self.level_to_vec(&self.num, j)
    }
    pub fn den_level_to_vec(&self, j: usize) -> Result<Vec<F>, DeviceError> {
        self.level_to_vec(&self.den, j)
    }
}

/// The launches of [`DeviceMultilinearExtension::fraction_tree`] as `ark_hip_mle_fraction_tree_plan` reports them: per run of
/// launches of one kernel variant, (levels, 0).  Host only.
pub fn fraction_tree_plan(num_vars: usize, has_num: bool) -> Result<Vec<(usize, usize)>, DeviceError> {
    let (mut passes, mut widths, mut groups) = (0 as core::ffi::c_int, [0 as core::ffi::c_int; 8], [0 as core::ffi::c_int; 8]);
    rc(unsafe {
        sys::ark_hip_mle_fraction_tree_plan(num_vars as c_uint, has_num as core::ffi::c_int, &mut passes, widths.as_mut_ptr(), groups.as_mut_ptr())
    })?;
    Ok((0..passes as usize).map(|p| (widths[p] as usize, groups[p] as usize)).collect())
}

fn rc(code: core::ffi::c_int) -> Result<(), DeviceError> {
    if code == 0 { Ok(()) } else { Err(DeviceError::Library(code)) }
}
fn flat<F: FftField>(point: &[F]) -> Vec<u64> {
    point.iter().flat_map(|x| sys::limbs(x)).collect()
}

impl<F: FftField> DeviceMultilinearExtension<F> {
    /// `from_evaluations_vec` (dense.rs:58-70) for a table already on the device; `Err(Mismatch)` unless it holds
    /// `2^num_vars` elements.
    pub fn from_device_vec(num_vars: usize, evals: DeviceVec<F>) -> Result<Self, DeviceError> {
        if num_vars >= 64 || evals.len() != 1usize << num_vars {
            return Err(DeviceError::Mismatch);
        }
        Ok(Self { num_vars, evals })
    }
    /// `from_evaluations_slice`: one upload.
    pub fn from_evaluations_slice(num_vars: usize, evaluations: &[F]) -> Result<Self, DeviceError> {
        Self::from_device_vec(num_vars, DeviceVec::from_slice(evaluations)?)
    }
    /// the constant zero: `num_vars = 0`, one zero evaluation (dense.rs:422-427)
    pub fn zero() -> Result<Self, DeviceError> {
        Self::from_device_vec(0, DeviceVec::zeros(1)?)
    }
    /// `num_vars == 0` and a zero evaluation (dense.rs:429-431): one element is downloaded, and only when `num_vars == 0`
    pub fn is_zero(&self) -> Result<bool, DeviceError> {
        if self.num_vars != 0 {
            return Ok(false);
        }
        Ok(self.evals.to_vec()?[0].is_zero())
    }
    pub fn num_vars(&self) -> usize {
        self.num_vars
    }
    pub fn to_evaluations(&self) -> Result<Vec<F>, DeviceError> {
        self.evals.to_vec()
    }
    pub fn evaluations(&self) -> &DeviceVec<F> {
        &self.evals
    }
    pub fn try_clone(&self) -> Result<Self, DeviceError> {
        Ok(Self { num_vars: self.num_vars, evals: self.evals.try_clone()? })
    }
    /// `MultilinearExtension::fix_variables` (dense.rs:224-257): binds the first `partial_point.len()` variables.
    pub fn fix_variables(&self, partial_point: &[F]) -> Result<Self, DeviceError> {
        self.evals.here()?;
        let dim = partial_point.len();
        if dim > self.num_vars {
            return Err(DeviceError::Mismatch);
        }
        let mut out = DeviceVec::<F>::alloc(1usize << (self.num_vars - dim))?;
        let pt = flat(partial_point);
        rc(unsafe {
            sys::ark_hip_mle_fix_variables_device(self.evals.field(), self.evals.as_device_ptr(), self.num_vars as c_uint, pt.as_ptr(),
                                                  dim as c_uint, out.as_device_mut_ptr())
        })?;
        Ok(Self { num_vars: self.num_vars - dim, evals: out })
    }
    /// `Polynomial::evaluate` (dense.rs:460-465); waits for the one element that comes back.
    pub fn evaluate(&self, point: &[F]) -> Result<F, DeviceError> {
        self.evals.here()?;
        if point.len() != self.num_vars {
            return Err(DeviceError::Mismatch);
        }
        let pt = flat(point);
        let mut out = [0u64; 4];
        rc(unsafe {
            sys::ark_hip_mle_evaluate_device(self.evals.field(), self.evals.as_device_ptr(), self.num_vars as c_uint, pt.as_ptr(),
                                             out.as_mut_ptr())
        })?;
        Ok(sys::from_limbs::<F>(&out))
    }
    /// The table `eq(point, b) = prod_i (b_i ? point_i : 1 - point_i)`, times `scale` (`None`: one), built on the device:
    /// `<f, eq(r)> = f(r)`.
    pub fn eq(point: &[F], scale: Option<&F>) -> Result<Self, DeviceError> {
        let num_vars = point.len();
        if num_vars >= 64 {
            return Err(DeviceError::Mismatch);
        }
        let mut out = DeviceVec::<F>::alloc(1usize << num_vars)?;
        let pt = flat(point);
        let k = scale.map(|x| sys::limbs(x));
        rc(unsafe {
            sys::ark_hip_mle_eq_table_device(out.field(), pt.as_ptr(), num_vars as c_uint, k.as_ref().map_or(core::ptr::null(), |x| x.as_ptr()),
                                             out.as_device_mut_ptr())
        })?;
        Ok(Self { num_vars, evals: out })
    }
    /// `f(point)` and the quotients of the opening at `point`; waits for the value.
    pub fn quotients(&self, point: &[F]) -> Result<Quotients<F>, DeviceError> {
        self.evals.here()?;
        if point.len() != self.num_vars {
            return Err(DeviceError::Mismatch);
        }
        let mut all = DeviceVec::<F>::alloc((1usize << self.num_vars) - 1)?;
        let pt = flat(point);
        let mut out = [0u64; 4];
        rc(unsafe {
            sys::ark_hip_mle_quotients_device(self.evals.field(), self.evals.as_device_ptr(), self.num_vars as c_uint, pt.as_ptr(),
                                              all.as_device_mut_ptr(), out.as_mut_ptr())
        })?;
        Ok(Quotients { value: sys::from_limbs::<F>(&out), num_vars: self.num_vars, all })
    }
    /// `f(point)` and a commitment to every `q_i`: [`Self::quotients`], then one device MSM per level over the segment where
    /// it lies.  No verification and no hashing happens here.
    ///
    /// # Safety
    /// `d_bases_per_level[i]` is a device array of `2^(num_vars-1-i)` `Affine<P>` on the current device.
    pub unsafe fn open<P: HipServed<ScalarField = F>>(&self, point: &[F], d_bases_per_level: &[*const Affine<P>])
                                                      -> Result<(F, Vec<Projective<P>>), DeviceError> {
        if d_bases_per_level.len() != self.num_vars {
            return Err(DeviceError::Mismatch);
        }
        let q = self.quotients(point)?;
        let mut points = Vec::with_capacity(self.num_vars);
        for (i, bases) in d_bases_per_level.iter().enumerate() {
            let mut out = core::mem::MaybeUninit::<Projective<P>>::uninit();
            rc(sys::ark_hip_msm_sw_device(P::CURVE, *bases as *const c_void, q.segment_ptr(i), q.segment_len(i), 1,
                                          out.as_mut_ptr() as *mut u64))?;
            points.push(out.assume_init());
        }
        Ok((q.value, points))
    }
    /// The binary product tree over the table and the product of all its entries; waits for the
    /// product.  The table is not written.
    pub fn product_tree(&self) -> Result<ProductTree<F>, DeviceError> {
        self.evals.here()?;
        let mut all = DeviceVec::<F>::alloc((1usize << self.num_vars) - 1)?;
        let mut out = [0u64; 4];
        rc(unsafe {
            sys::ark_hip_mle_product_tree_device(self.evals.field(), self.evals.as_device_ptr(), self.num_vars as c_uint,
                                                 all.as_device_mut_ptr(), out.as_mut_ptr())
        })?;
        Ok(ProductTree { product: sys::from_limbs::<F>(&out), num_vars: self.num_vars, all })
    }
    /// `c0 + sum_k coeffs[k] tables[k]`, entry by entry in one pass (`c0 = None`: zero): the fingerprints that are the
    /// leaves of a grand product.  `Err(Mismatch)` unless there are 1 to 8 tables of one size with one coefficient each.
    pub fn linear_combination(tables: &[&Self], coeffs: &[F], c0: Option<&F>) -> Result<Self, DeviceError> {
        if tables.is_empty() || tables.len() > 8 || coeffs.len() != tables.len() {
            return Err(DeviceError::Mismatch);
        }
        let num_vars = tables[0].num_vars;
        let mut ptrs: Vec<*const c_void> = Vec::with_capacity(tables.len());
        for t in tables {
            t.evals.here()?;
            if t.num_vars != num_vars {
                return Err(DeviceError::Mismatch);
            }
            ptrs.push(t.evals.as_device_ptr());
        }
        let mut out = DeviceVec::<F>::alloc(1usize << num_vars)?;
        let k = flat(coeffs);
        let g = c0.map(|x| sys::limbs(x));
        rc(unsafe {
            sys::ark_hip_fr_lincomb_device(out.field(), ptrs.as_ptr(), ptrs.len() as c_uint, k.as_ptr(),
                                           g.as_ref().map_or(core::ptr::null(), |x| x.as_ptr()), out.as_device_mut_ptr(), out.len())
        })?;
        Ok(Self { num_vars, evals: out })
    }
    /// The tree that adds the fractions `num[b] / self[b]` and its root; `num = None`: every numerator
    /// is one.  Waits for the root.  The tables are not written.  `Err(Mismatch)` if the sizes differ.
    pub fn fraction_tree(&self, num: Option<&Self>) -> Result<FractionTree<F>, DeviceError> {
        self.evals.here()?;
        if let Some(m) = num {
            m.evals.here()?;
            if m.num_vars != self.num_vars {
                return Err(DeviceError::Mismatch);
            }
        }
        let len = (1usize << self.num_vars) - 1;
        let (mut nt, mut dt) = (DeviceVec::<F>::alloc(len)?, DeviceVec::<F>::alloc(len)?);
        let mut out = [0u64; 8];
        rc(unsafe {
            sys::ark_hip_mle_fraction_tree_device(self.evals.field(), num.map_or(core::ptr::null(), |m| m.evals.as_device_ptr()),
                                                  self.evals.as_device_ptr(), self.num_vars as c_uint, nt.as_device_mut_ptr(),
                                                  dt.as_device_mut_ptr(), out.as_mut_ptr())
        })?;
        let (p, q) = ([out[0], out[1], out[2], out[3]], [out[4], out[5], out[6], out[7]]);
        Ok(FractionTree { root: (sys::from_limbs::<F>(&p), sys::from_limbs::<F>(&q)), num_vars: self.num_vars, num: nt, den: dt })
    }
    /// The multiplicity table of a lookup, `m[j] = #{i : indices[i] = j}` for `j < table_len`, counted on the device from `n`
    /// device `u32`.  An index `>= table_len` is skipped and not reported: the counts sum to `n` exactly when none was skipped.
    ///
    /// # Safety
    /// `d_indices` must point to `n` `u32` in device memory of the current device.
    pub unsafe fn count_indices(d_indices: *const u32, n: usize, table_len: usize) -> Result<DeviceVec<F>, DeviceError> {
        let mut out = DeviceVec::<F>::alloc(table_len)?;
        rc(sys::ark_hip_fr_count_indices_device(out.field(), d_indices, n, out.as_device_mut_ptr(), table_len))?;
        Ok(out)
    }
    /// The join of a lookup from the values, on the device: `(m, missing)` with
    /// `m[j] = #{i : values[i] is found at j}`, `j` the FIRST occurrence of the value in `table` (a repeated table value keeps
    /// zero in its later cells), and `missing` the number of cells of `values` that are not in the table.  Waits for `missing`.
    /// `d_indices`: null, or room for `values.len()` device `u32` that receive each cell's index
    /// (`sys::ARK_HIP_LOOKUP_MISSING` where not found).
    ///
    /// # Safety
    /// `d_indices` must be null or point to `values.len()` `u32` in device memory of the current device.
    pub unsafe fn lookup(table: &DeviceVec<F>, values: &DeviceVec<F>, d_indices: *mut u32) -> Result<(DeviceVec<F>, u64), DeviceError> {
        table.here()?;
        values.here()?;
        let mut out = DeviceVec::<F>::alloc(table.len())?;
        let mut missing = 0u64;
        rc(sys::ark_hip_fr_lookup_device(out.field(), table.as_device_ptr(), table.len(), values.as_device_ptr(), values.len(),
                                         d_indices, out.as_device_mut_ptr(), &mut missing))?;
        Ok((out, missing))
    }
    /// `(capacity_log, scratch_bytes)` of `lookup` against a table of `table_len` values: host only.
    pub fn lookup_plan(table_len: usize) -> Result<(u32, usize), DeviceError> {
        let (mut c, mut b): (c_uint, usize) = (0, 0);
        rc(unsafe { sys::ark_hip_fr_lookup_plan(table_len, &mut c, &mut b) })?;
        Ok((c as u32, b))
    }
    /// `relabel` (dense.rs:195-199): a new polynomial with the `k` variables from `a` and from `b` exchanged.
    pub fn relabel(&self, a: usize, b: usize, k: usize) -> Result<Self, DeviceError> {
        self.evals.here()?;
        let mut out = DeviceVec::<F>::alloc(self.evals.len())?;
        rc(unsafe {
            sys::ark_hip_mle_relabel_device(self.evals.field(), self.evals.as_device_ptr(), self.num_vars as c_uint, a as c_uint,
                                            b as c_uint, k as c_uint, out.as_device_mut_ptr())
        })?;
        Ok(Self { num_vars: self.num_vars, evals: out })
    }
    /// `relabel_in_place` (dense.rs:76-92)
    pub fn relabel_in_place(&mut self, a: usize, b: usize, k: usize) -> Result<(), DeviceError> {
        self.evals.here()?;
        let p = self.evals.as_device_mut_ptr();
        rc(unsafe {
            sys::ark_hip_mle_relabel_device(self.evals.field(), p as *const c_void, self.num_vars as c_uint, a as c_uint, b as c_uint,
                                            k as c_uint, p)
        })
    }
    /// `concat` (dense.rs:133-156): the tables one after the other, zero-filled up to the next power of two.
    pub fn concat(polys: &[&Self]) -> Result<Self, DeviceError> {
        let total: usize = polys.iter().map(|p| p.evals.len()).sum();
        let padded = total.next_power_of_two();
        let mut out = DeviceVec::<F>::alloc(padded)?;
        let base = out.as_device_mut_ptr() as *mut u8;
        let mut at = 0usize;
        for p in polys {
            p.evals.here()?;
            rc(unsafe { sys::ark_hip_memcpy_d2d(base.add(at * 32) as *mut c_void, p.evals.as_device_ptr(), p.evals.len() * 32) })?;
            at += p.evals.len();
        }
        if at < padded {
            rc(unsafe { sys::ark_hip_memset_device(base.add(at * 32) as *mut c_void, 0, (padded - at) * 32) })?;
        }
        Ok(Self { num_vars: padded.trailing_zeros() as usize, evals: out })
    }
    fn same(&self, other: &Self) -> Result<(), DeviceError> {
        if self.num_vars == other.num_vars { Ok(()) } else { Err(DeviceError::Mismatch) }
    }
    /// `&self + &rhs` (dense.rs:286-305): the constant zero on either side gives a copy of the other operand.
    pub fn add(&self, rhs: &Self) -> Result<Self, DeviceError> {
        if rhs.is_zero()? {
            return self.try_clone();
        }
        if self.is_zero()? {
            return rhs.try_clone();
        }
        self.same(rhs)?;
        let mut out = self.evals.try_clone()?;
        out.add_assign_pointwise(&rhs.evals)?;
        Ok(Self { num_vars: self.num_vars, evals: out })
    }
    /// `-self` (dense.rs:329-338)
    pub fn neg(&self) -> Result<Self, DeviceError> {
        let mut out = self.evals.try_clone()?;
        out.negate()?;
        Ok(Self { num_vars: self.num_vars, evals: out })
    }
    /// `&self - &rhs` = `self + (-rhs)` (dense.rs:348-354)
    pub fn sub(&self, rhs: &Self) -> Result<Self, DeviceError> {
        self.add(&rhs.neg()?)
    }
    fn scaled(&self, k: &F) -> Result<Self, DeviceError> {
        let mut out = self.evals.try_clone()?;
        out.scale(k)?;
        Ok(Self { num_vars: self.num_vars, evals: out })
    }
    /// `&self * &scalar` (dense.rs:376-392): times zero gives `zero()`.
    pub fn mul_scalar(&self, scalar: &F) -> Result<Self, DeviceError> {
        if scalar.is_zero() {
            return Self::zero();
        }
        self.scaled(scalar)
    }
    /// `self += (f, other)` (dense.rs:319-327) in one pass over the two tables: no scaled temporary.
    pub fn add_assign_scaled(&mut self, f: &F, other: &Self) -> Result<(), DeviceError> {
        if other.is_zero()? || (other.num_vars == 0 && f.is_zero()) {
            return Ok(()); // f * other is the constant zero
        }
        if self.is_zero()? {
            *self = other.scaled(f)?;
            return Ok(());
        }
        self.same(other)?;
        self.evals.here()?;
        let k = sys::limbs(f);
        let n = self.evals.len();
        let p = self.evals.as_device_mut_ptr();
        rc(unsafe { sys::ark_hip_fr_axpy_device(self.evals.field(), p as *const c_void, k.as_ptr(), other.evals.as_device_ptr(), p, n) })
    }
}
