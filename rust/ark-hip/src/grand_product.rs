//! The layered proof of a grand product `P = prod_b f[b]` over a device-resident table (Thaler's GKR grand product; DESIGN.md
//! section 19).  [`DenseMultilinearExtension::product_tree`] gives the levels `L_nu = f`, `L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k]`,
//! `L_0 = [P]`; the two halves of a level are its polynomial with the LAST variable at 0 and at 1, so
//! `L_k(r) = sum_x eq(r, x) L_{k+1}(x, 0) L_{k+1}(x, 1)` is one sumcheck of `eq * left * right` over two views per layer.  It
//! leaves the claim `left(rho) + tau (right(rho) - left(rho))` about `L_{k+1}(rho, tau)`; the last claim is `f(point)`, which
//! `evaluate` / `open` answer.  Nothing is hashed here and nothing is verified: the transcript is the caller's.
use crate::device::{DeviceError, DeviceVec};
use crate::mle::DenseMultilinearExtension;
use crate::sumcheck::{ListOfProducts, SumcheckProof};
use ark_ff::FftField;
use ark_std::{rc::Rc, vec::Vec};

/// what [`GrandProduct::prove`] returns
pub struct GrandProductProof<F: FftField> {
    pub product: F,
    /// per layer: its sumcheck (`None` for layer 0) and the pair `(left, right)`: the two elements of `L_1` for layer 0, else
    /// `left(rho)`, `right(rho)` at the sumcheck's point
    pub layers: Vec<(Option<SumcheckProof<F>>, (F, F))>,
    /// `r_nu`: where the verifier's last claim about `f` lies
    pub point: Vec<F>,
}

pub struct GrandProduct<'a, F: FftField> {
    f: &'a DenseMultilinearExtension<F>,
}

impl<'a, F: FftField> GrandProduct<'a, F> {
    pub fn new(f: &'a DenseMultilinearExtension<F>) -> Self {
        Self { f }
    }
    /// `challenge(layer, round, values)`: with `round = Some(i)` the values are round `i`'s evaluations of the layer's
    /// sumcheck, with `None` they are the layer's pair and the answer is the layer's `tau`.  The table and the tree are not
    /// written.
    pub fn prove(&self, mut challenge: impl FnMut(usize, Option<usize>, &[F]) -> F) -> Result<GrandProductProof<F>, DeviceError> {
        let nu = self.f.num_vars();
        let tree = self.f.product_tree()?;
        let mut out = GrandProductProof { product: tree.product, layers: Vec::new(), point: Vec::new() };
        if nu == 0 {
            return Ok(out);
        }
        let one = DenseMultilinearExtension::<F>::eq(&[], None)?.to_evaluations()?[0]; // the eq table of no variables is its scale
        let l1 = if nu == 1 { self.f.to_evaluations()? } else { tree.level_to_vec(nu - 1)? };
        out.point.push(challenge(0, None, &l1));
        out.layers.push((None, (l1[0], l1[1])));
        for k in 1..nu {
            let h = 1usize << k;
            // L_(k+1): the table itself for the last layer, else level nu - k - 1 of the tree; its halves are views
            let (owner, at): (&DeviceVec<F>, usize) =
                if k + 1 == nu { (self.f.evaluations(), 0) } else { (tree.all(), tree.level_offset(nu - k - 1)) };
            let eq = Rc::new(DenseMultilinearExtension::eq(&out.point, None)?);
            // the views are dropped with `lp` at the end of this iteration, before `tree` and without a write to either owner
            let left = Rc::new(DenseMultilinearExtension::from_device_vec(k, unsafe { DeviceVec::view(owner, at, h)? })?);
            let right = Rc::new(DenseMultilinearExtension::from_device_vec(k, unsafe { DeviceVec::view(owner, at + h, h)? })?);
            let mut lp = ListOfProducts::new(k);
            lp.add_product(&[eq, left, right], one)?;
            let sc = lp.prove(|i, evals| challenge(k, Some(i), evals))?;
            let pair = (sc.final_evaluations[1], sc.final_evaluations[2]);
            let tau = challenge(k, None, &[pair.0, pair.1]);
            out.point = sc.point.clone();
            out.point.push(tau);
            out.layers.push((Some(sc), pair));
        }
        Ok(out)
    }
}
