//! The layered proof of a sum of fractions `P / Q = sum_b num[b] / den[b]` over device-resident tables (the GKR form of logUp,
//! Papini-Haboeck).  [`DenseMultilinearExtension::fraction_tree`] gives the levels `N_nu = num`,
//! `D_nu = den`, `N_k[i] = N_{k+1}[i] D_{k+1}[i + 2^k] + N_{k+1}[i + 2^k] D_{k+1}[i]`, `D_k[i] = D_{k+1}[i] D_{k+1}[i + 2^k]`,
//! `(N_0[0], D_0[0]) = (P, Q)`; the halves `n0, n1, d0, d1` of the levels above are their polynomials with the LAST variable at
//! 0 and at 1, so `N_k(r) + lambda D_k(r) = sum_x eq(r, x) (n0 d1 + n1 d0 + lambda d0 d1)(x)` is one sumcheck of three products
//! over five tables per layer.  It leaves the claims `n0 + tau (n1 - n0)` and `d0 + tau (d1 - d0)` about the levels above at
//! `(rho, tau)`; the last claims are `num(point)` and `den(point)`, which `evaluate` / `open` answer.  With ones for numerators
//! the level above the last layer is the leaves: its products are `eq d1`, `eq d0` and `lambda eq d0 d1`.  Nothing is hashed
//! here and nothing is verified: the transcript is the caller's.
use crate::device::{DeviceError, DeviceVec};
use crate::mle::DenseMultilinearExtension;
use crate::sumcheck::{ListOfProducts, SumcheckProof};
use ark_ff::FftField;
use ark_std::{rc::Rc, vec::Vec};

/// the `round` a challenge is asked for with when it is the layer's `tau`; the values are the layer's
pub const TAU_ROUND: i32 = -1;
/// the `round` a challenge is asked for with when it is the layer's batching challenge `lambda`, before the layer's sumcheck;
/// there are no values
pub const LAMBDA_ROUND: i32 = -2;

/// what [`FractionalSum::prove`] returns
pub struct FractionalSumProof<F: FftField> {
    /// `(P, Q)`
    pub root: (F, F),
    /// per layer: its sumcheck (`None` for layer 0) and its values `(n0, n1, d0, d1)` -- the two elements each of `N_1` and
    /// `D_1` for layer 0, else the halves at the sumcheck's point --, or `(d0, d1)` where the numerators are the implicit ones
    pub layers: Vec<(Option<SumcheckProof<F>>, Vec<F>)>,
    /// `r_nu`: where the verifier's last claims about `num` and `den` lie
    pub point: Vec<F>,
}

pub struct FractionalSum<'a, F: FftField> {
    num: Option<&'a DenseMultilinearExtension<F>>,
    den: &'a DenseMultilinearExtension<F>,
}

impl<'a, F: FftField> FractionalSum<'a, F> {
    /// `num = None`: every numerator is one.  `Err(Mismatch)` if the sizes differ.
    pub fn new(num: Option<&'a DenseMultilinearExtension<F>>, den: &'a DenseMultilinearExtension<F>) -> Result<Self, DeviceError> {
        if num.map_or(false, |m| m.num_vars() != den.num_vars()) {
            return Err(DeviceError::Mismatch);
        }
        Ok(Self { num, den })
    }
    /// `challenge(layer, round, values)`: with `round = i >= 0` the values are round `i`'s evaluations of the layer's
    /// sumcheck; with [`LAMBDA_ROUND`] there are none and the answer is the layer's batching challenge; with [`TAU_ROUND`]
    /// they are the layer's values and the answer is the layer's `tau`.  The tables and the trees are not written.
    pub fn prove(&self, mut challenge: impl FnMut(usize, i32, &[F]) -> F) -> Result<FractionalSumProof<F>, DeviceError> {
        let nu = self.den.num_vars();
        let tree = self.den.fraction_tree(self.num)?;
        let mut out = FractionalSumProof { root: tree.root, layers: Vec::new(), point: Vec::new() };
        if nu == 0 {
            return Ok(out);
        }
        let one = DenseMultilinearExtension::<F>::eq(&[], None)?.to_evaluations()?[0]; // the eq table of no variables is its scale
        // N_1 (unless it is the implicit ones), then D_1
        let mut v = match (nu, self.num) {
            (1, Some(m)) => m.to_evaluations()?,
            (1, None) => Vec::new(),
            _ => tree.num_level_to_vec(nu - 1)?,
        };
        v.extend(if nu == 1 { self.den.to_evaluations()? } else { tree.den_level_to_vec(nu - 1)? });
        out.point.push(challenge(0, TAU_ROUND, &v));
        out.layers.push((None, v));
        for k in 1..nu {
            let lambda = challenge(k, LAMBDA_ROUND, &[]);
            let h = 1usize << k;
            let top = k + 1 == nu; // the levels above are the tables themselves
            let at = if top { 0 } else { tree.level_offset(nu - k - 1) };
            let d_owner: &DeviceVec<F> = if top { self.den.evaluations() } else { tree.den() };
            let eq = Rc::new(DenseMultilinearExtension::eq(&out.point, None)?);
            // the views are dropped with `lp` at the end of this iteration, before `tree` and without a write to an owner
            let d0 = Rc::new(DenseMultilinearExtension::from_device_vec(k, unsafe { DeviceVec::view(d_owner, at, h)? })?);
            let d1 = Rc::new(DenseMultilinearExtension::from_device_vec(k, unsafe { DeviceVec::view(d_owner, at + h, h)? })?);
            let mut lp = ListOfProducts::new(k);
            let n_owner: Option<&DeviceVec<F>> = if top { self.num.map(|m| m.evaluations()) } else { Some(tree.num()) };
            let (sc, v) = match n_owner {
                None => {
                    lp.add_product(&[eq.clone(), d1.clone()], one)?;
                    lp.add_product(&[eq.clone(), d0.clone()], one)?;
                    lp.add_product(&[eq, d0, d1], lambda)?;
                    let sc = lp.prove(|i, evals| challenge(k, i as i32, evals))?;
                    let f = &sc.final_evaluations; // tables: eq, d1, d0
                    let v = [f[2], f[1]].to_vec();
                    (sc, v)
                }
                Some(owner) => {
                    let n0 = Rc::new(DenseMultilinearExtension::from_device_vec(k, unsafe { DeviceVec::view(owner, at, h)? })?);
                    let n1 = Rc::new(DenseMultilinearExtension::from_device_vec(k, unsafe { DeviceVec::view(owner, at + h, h)? })?);
                    lp.add_product(&[eq.clone(), n0, d1.clone()], one)?;
                    lp.add_product(&[eq.clone(), n1, d0.clone()], one)?;
                    lp.add_product(&[eq, d0, d1], lambda)?;
                    let sc = lp.prove(|i, evals| challenge(k, i as i32, evals))?;
                    let f = &sc.final_evaluations; // tables: eq, n0, d1, n1, d0
                    let v = [f[1], f[3], f[4], f[2]].to_vec();
                    (sc, v)
                }
            };
            let tau = challenge(k, TAU_ROUND, &v);
            out.point = sc.point.clone();
            out.point.push(tau);
            out.layers.push((Some(sc), v));
        }
        Ok(out)
    }
}
