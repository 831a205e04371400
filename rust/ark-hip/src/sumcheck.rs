//! The sumcheck prover over device-resident multilinear tables.  [`ListOfProducts`] has the shape of ark-linear-sumcheck's
//! `ListOfProductsOfPolynomials`: a list of products of shared tables, each with a coefficient,
//! `sum_b sum_j c_j prod_{k in term j} f_k(b)`.  [`ListOfProducts::round`] is one call of `ark_hip_sumcheck_round_device` on
//! the tables where they lie; [`ListOfProducts::prove`] runs the whole prover against a caller-supplied source of challenges.
//! Nothing is hashed here and nothing is verified: the transcript is the caller's.
//!
//! Tables are shared by pointer, as the upstream type shares `Rc`s: the same `Rc<DenseMultilinearExtension<F>>` added to two
//! products (or twice to one) is one table on the device.
use crate::device::{DeviceError, DeviceVec};
use crate::mle::DenseMultilinearExtension;
use ark_ff::FftField;
use ark_hip_sys as sys;
use ark_std::{rc::Rc, vec::Vec};
use core::ffi::{c_uint, c_void};

/// `ARK_HIP_SUMCHECK_MAX_TABLES`, `_MAX_TERMS`, `_MAX_DEGREE` of include/ark_hip.h
pub const MAX_TABLES: usize = 8;
pub const MAX_TERMS: usize = 8;
pub const MAX_DEGREE: usize = 4;

fn rc(code: core::ffi::c_int) -> Result<(), DeviceError> {
    if code == 0 { Ok(()) } else { Err(DeviceError::Library(code)) }
}

/// what [`ListOfProducts::prove`] returns
pub struct SumcheckProof<F: FftField> {
    /// `rounds[i]`: the `D + 1` evaluations `g_i(0 .. D)`
    pub rounds: Vec<Vec<F>>,
    /// the `nu` challenges
    pub point: Vec<F>,
    /// `f_k(point)` for the tables in the order they were first added
    pub final_evaluations: Vec<F>,
    /// `sum_j c_j prod_k f_k(point)`: what the verifier's last check compares
    pub final_value: F,
}

/// The Fiat-Shamir transcript of the device sumcheck: 32 bytes of state the caller initialises; [`Transcript::challenge`] is
/// one call of the host entry `ark_hip_transcript_challenge` (`state | count | elements` through SHAKE256; needs no device).
pub struct Transcript<F: FftField> {
    field: core::ffi::c_int,
    state: [u8; 32],
    _f: core::marker::PhantomData<F>,
}

impl<F: FftField> Transcript<F> {
    /// `Err(UnsupportedField)` when `F` is not one of the scalar fields the library serves
    pub fn new(seed: [u8; 32]) -> Result<Self, DeviceError> {
        let field = sys::fr_field_id::<F>().ok_or(DeviceError::UnsupportedField)?;
        Ok(Self { field, state: seed, _f: core::marker::PhantomData })
    }
    pub fn state(&self) -> &[u8; 32] {
        &self.state
    }
    pub fn challenge(&mut self, elements: &[F]) -> Result<F, DeviceError> {
        let els: Vec<u64> = elements.iter().flat_map(|e| sys::limbs(e)).collect();
        let mut out = [0u64; 4];
        rc(unsafe {
            sys::ark_hip_transcript_challenge(self.field, self.state.as_mut_ptr(), if els.is_empty() { core::ptr::null() } else { els.as_ptr() },
                                              elements.len() as c_uint, out.as_mut_ptr())
        })?;
        Ok(sys::from_limbs::<F>(&out))
    }
}

pub struct ListOfProducts<F: FftField> {
    num_vars: usize,
    tables: Vec<Rc<DenseMultilinearExtension<F>>>,
    products: Vec<(F, Vec<usize>)>,
    degree: usize,
    /// the tables as bound so far (`None`: the caller's) and the variables they still have
    bound: Option<Vec<*const c_void>>,
    vars_left: usize,
    /// halves and quarters: the output of a bind is never the set it reads, and the caller's tables are never written
    sets: Option<[Vec<DeviceVec<F>>; 2]>,
    next: usize,
}

impl<F: FftField> ListOfProducts<F> {
    pub fn new(num_vars: usize) -> Self {
        Self { num_vars, tables: Vec::new(), products: Vec::new(), degree: 0, bound: None, vars_left: num_vars, sets: None, next: 0 }
    }
    pub fn num_vars(&self) -> usize {
        self.num_vars
    }
    pub fn max_multiplicands(&self) -> usize {
        self.degree
    }
    /// adds `coefficient * prod mles`; `Err(Mismatch)` for a wrong `num_vars`, no or too many factors, too many products or tables
    pub fn add_product(&mut self, mles: &[Rc<DenseMultilinearExtension<F>>], coefficient: F) -> Result<(), DeviceError> {
        if mles.is_empty() || mles.len() > MAX_DEGREE || self.products.len() >= MAX_TERMS || self.bound.is_some() {
            return Err(DeviceError::Mismatch);
        }
        let mut tables = self.tables.clone();
        let mut idx = Vec::with_capacity(mles.len());
        for m in mles {
            if m.num_vars() != self.num_vars {
                return Err(DeviceError::Mismatch);
            }
            match tables.iter().position(|t| Rc::ptr_eq(t, m)) {
                Some(i) => idx.push(i),
                None => {
                    idx.push(tables.len());
                    tables.push(m.clone());
                }
            }
        }
        if tables.len() > MAX_TABLES {
            return Err(DeviceError::Mismatch);
        }
        self.tables = tables;
        self.degree = self.degree.max(idx.len());
        self.products.push((coefficient, idx));
        Ok(())
    }

    fn call(&self, tables: &[*const c_void], num_vars: usize, r_prev: Option<&F>, outs: Option<&[*mut c_void]>) -> Result<Vec<F>, DeviceError> {
        let field = self.tables[0].evaluations().field();
        let lens: Vec<c_uint> = self.products.iter().map(|(_, ix)| ix.len() as c_uint).collect();
        let flat: Vec<c_uint> = self.products.iter().flat_map(|(_, ix)| ix.iter().map(|&i| i as c_uint)).collect();
        let coeffs: Vec<u64> = self.products.iter().flat_map(|(c, _)| sys::limbs(c)).collect();
        let r: Option<Vec<u64>> = r_prev.map(|x| sys::limbs(x).into_iter().collect());
        let mut evals = ark_std::vec![0u64; 4 * (self.degree + 1)];
        rc(unsafe {
            sys::ark_hip_sumcheck_round_device(field, tables.as_ptr(), tables.len() as c_uint, num_vars as c_uint, lens.as_ptr(),
                                               flat.as_ptr(), coeffs.as_ptr(), lens.len() as c_uint,
                                               r.as_ref().map_or(core::ptr::null(), |v| v.as_ptr()),
                                               outs.map_or(core::ptr::null(), |o| o.as_ptr()), evals.as_mut_ptr())
        })?;
        Ok(evals.chunks(4).map(|c| sys::from_limbs::<F>(&[c[0], c[1], c[2], c[3]])).collect())
    }

    /// The `D + 1` evaluations of the round polynomial over the tables as bound so far.  With `r_prev` the first remaining
    /// variable is bound to it first, in the same launch, into tables of the list's own.
    pub fn round(&mut self, r_prev: Option<&F>) -> Result<Vec<F>, DeviceError> {
        if self.products.is_empty() || self.vars_left == 0 {
            return Err(DeviceError::Mismatch);
        }
        for t in &self.tables {
            t.evaluations().here()?;
        }
        let cur: Vec<*const c_void> = match &self.bound {
            Some(b) => b.clone(),
            None => self.tables.iter().map(|t| t.evaluations().as_device_ptr()).collect(),
        };
        let r = match r_prev {
            None => {
                let evals = self.call(&cur, self.vars_left, None, None)?;
                self.bound = Some(cur);
                return Ok(evals);
            }
            Some(r) => r,
        };
        if self.sets.is_none() {
            let mut sets: [Vec<DeviceVec<F>>; 2] = [Vec::new(), Vec::new()];
            for (s, set) in sets.iter_mut().enumerate() {
                for _ in 0..self.tables.len() {
                    set.push(DeviceVec::<F>::alloc(1usize << self.num_vars.saturating_sub(1 + s))?);
                }
            }
            self.sets = Some(sets);
        }
        let outs: Vec<*mut c_void> = self.sets.as_mut().unwrap()[self.next].iter_mut().map(|v| v.as_device_mut_ptr()).collect();
        let evals = self.call(&cur, self.vars_left, Some(r), Some(&outs))?;
        self.bound = Some(outs.iter().map(|&p| p as *const c_void).collect());
        self.vars_left -= 1;
        self.next ^= 1;
        Ok(evals)
    }

    /// Runs the `nu + 1` calls: call 0 has no bind, calls `1 .. nu` bind the challenge before.  `challenge(i, evals)` gets
    /// round `i`'s evaluations and returns the verifier's element for it.
    pub fn prove(&mut self, mut challenge: impl FnMut(usize, &[F]) -> F) -> Result<SumcheckProof<F>, DeviceError> {
        if self.bound.is_some() || self.num_vars == 0 {
            return Err(DeviceError::Mismatch);
        }
        let mut rounds = Vec::with_capacity(self.num_vars);
        let mut point = Vec::with_capacity(self.num_vars);
        let mut evals = self.round(None)?;
        for i in 0..self.num_vars {
            let r = challenge(i, &evals);
            rounds.push(evals);
            evals = self.round(Some(&r))?;
            point.push(r);
        }
        // the one-element tables: f_k(point)
        let mut final_evaluations = Vec::with_capacity(self.tables.len());
        for &p in self.bound.as_ref().unwrap() {
            let mut out = [0u64; 4];
            rc(unsafe { sys::ark_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, p, 32) })?;
            final_evaluations.push(sys::from_limbs::<F>(&out));
        }
        Ok(SumcheckProof { rounds, point, final_evaluations, final_value: evals[0] })
    }

    /// The whole proof in one wait: what [`ListOfProducts::prove`] returns when `challenge(i, evals)` is
    /// `transcript.challenge(evals)`, with the challenges derived on the device (one call of `ark_hip_sumcheck_prove_device`).
    /// Advances the transcript; allocates and frees its own work vector.  `tail_vars`: `-1` the library's default, `0` no
    /// one-workgroup tail, else the variables it starts at.
    pub fn prove_device(&mut self, transcript: &mut Transcript<F>, tail_vars: i32) -> Result<SumcheckProof<F>, DeviceError> {
        if self.bound.is_some() || self.num_vars == 0 || self.products.is_empty() {
            return Err(DeviceError::Mismatch);
        }
        for t in &self.tables {
            t.evaluations().here()?;
        }
        let (mut work_elems, mut launches, mut tail_from) = (0usize, 0, 0);
        rc(unsafe {
            sys::ark_hip_sumcheck_prove_plan(self.num_vars as c_uint, self.tables.len() as c_uint, tail_vars, &mut work_elems, &mut launches,
                                             &mut tail_from)
        })?;
        let mut work = DeviceVec::<F>::alloc(work_elems)?;
        let field = self.tables[0].evaluations().field();
        let tables: Vec<*const c_void> = self.tables.iter().map(|t| t.evaluations().as_device_ptr()).collect();
        let lens: Vec<c_uint> = self.products.iter().map(|(_, ix)| ix.len() as c_uint).collect();
        let flat: Vec<c_uint> = self.products.iter().flat_map(|(_, ix)| ix.iter().map(|&i| i as c_uint)).collect();
        let coeffs: Vec<u64> = self.products.iter().flat_map(|(c, _)| sys::limbs(c)).collect();
        let d1 = self.degree + 1;
        let mut rounds = ark_std::vec![0u64; 4 * d1 * self.num_vars];
        let mut point = ark_std::vec![0u64; 4 * self.num_vars];
        let mut finals = ark_std::vec![0u64; 4 * self.tables.len()];
        let mut value = [0u64; 4];
        rc(unsafe {
            sys::ark_hip_sumcheck_prove_device(field, tables.as_ptr(), tables.len() as c_uint, self.num_vars as c_uint, lens.as_ptr(),
                                               flat.as_ptr(), coeffs.as_ptr(), lens.len() as c_uint, transcript.state.as_mut_ptr(), tail_vars,
                                               work.as_device_mut_ptr(), rounds.as_mut_ptr(), point.as_mut_ptr(), finals.as_mut_ptr(),
                                               value.as_mut_ptr())
        })?;
        let els = |v: &[u64]| -> Vec<F> { v.chunks(4).map(|c| sys::from_limbs::<F>(&[c[0], c[1], c[2], c[3]])).collect() };
        Ok(SumcheckProof {
            rounds: rounds.chunks(4 * d1).map(|g| els(g)).collect(),
            point: els(&point),
            final_evaluations: els(&finals),
            final_value: sys::from_limbs::<F>(&value),
        })
    }
}
