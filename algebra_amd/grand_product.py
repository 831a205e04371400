"""The layered proof of a grand product P = prod_b f[b] over a device-resident table (Thaler's GKR grand product; DESIGN.md
section 19) -- the Python mirror of `GrandProduct` in include/ark_hip.hpp and rust/ark-hip/src/grand_product.rs.

`product_tree` gives the levels L_nu = f, L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k], L_0 = [P].  The two halves of a level are the
level's polynomial with its LAST variable at 0 and at 1, so for r in F^k

    L_k(r) = sum_{x in {0,1}^k} eq(r, x) L_{k+1}(x, 0) L_{k+1}(x, 1):

one sumcheck of eq * left * right per layer over two views of the level, which reduces the claim about L_k(r_k) to
left(rho) and right(rho), and the line through them at tau to one claim about L_{k+1}(rho, tau).  The last claim is f(point),
which `evaluate` / `open` answer.  No arithmetic happens here and nothing is hashed: the challenges come from the caller,
verification is the caller's (the tests carry a verifier)."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .mle import DenseMultilinearExtension, DeviceSegment, _element
from .poly import DeviceVec
from .sumcheck import ListOfProducts, sumcheck_prove_plan


def _one(field):
    """the field's one as the library writes it (the eq table of no variables is its scale, one): no arithmetic here and
    nothing kept between calls"""
    t = DenseMultilinearExtension.eq(field, np.zeros((0, 4), dtype=np.uint64))
    try:
        return t.to_evaluations()[0].copy()
    finally:
        t.free()


class GrandProductProof:
    """what prove() returns: `product` = P (uint64[4]); `layers[k]` = (SumcheckProof of layer k -- None for k = 0 --,
    numpy uint64 [2, 4] = (left, right): L_1's two elements for k = 0, else left(rho), right(rho) at the sumcheck's point);
    `point` = r_nu [nu, 4], where the verifier's last claim about f lies"""

    def __init__(self, product, layers, point):
        self.product, self.layers, self.point = product, layers, point


class GrandProduct:
    def __init__(self, f):
        if not isinstance(f, DenseMultilinearExtension):
            raise TypeError("a DenseMultilinearExtension expected")
        self.f = f

    def prove(self, challenge):
        """`challenge(layer, round, values)` returns the verifier's next element (uint64[4], Montgomery): with round = i the
        values are round i's evaluations of the layer's sumcheck, with round = None they are the layer's pair (left, right)
        and the answer is the layer's tau.  The table and the tree are not written."""
        return self._prove(challenge, lambda lp, k: lp.prove(lambda i, evals: challenge(k, i, evals)))

    def prove_device(self, transcript, tail_vars=None):
        """The same proof with every challenge from `transcript` (algebra_amd.Transcript): each layer's sumcheck is one
        ListOfProducts.prove_device -- one wait per layer instead of one per round --, the layer's pair goes through
        transcript.challenge on the host.  One work vector serves every layer.
        tail_vars: as in ListOfProducts.prove_device, for every layer."""
        nu = self.f.num_vars
        work = DeviceVec(self.f.field, sumcheck_prove_plan(nu - 1, 3)[0], _zero=False) if nu >= 2 else None
        try:
            return self._prove(lambda k, rnd, values: transcript.challenge(values), lambda lp, k: lp.prove_device(transcript, tail_vars, _work=work))
        finally:
            if work is not None:
                work.free()

    def _prove(self, challenge, sumcheck):
        """the layers; sumcheck(list of products, layer) -> the layer's SumcheckProof"""
        f, nu = self.f, self.f.num_vars
        n = 1 << nu
        # the tree is this call's own vector: released on every way out, also when the challenge or a round raises
        tree = DeviceVec(f.field, n - 1, _zero=False)
        try:
            product = np.zeros(4, dtype=np.uint64)
            check(lib().ark_hip_mle_product_tree_device(f.field, f.evaluations.ptr, nu, tree.ptr if nu else None,
                                                        product.ctypes.data_as(C.c_void_p)), "ark_hip_mle_product_tree_device")
            if nu == 0:
                return GrandProductProof(product, [], np.zeros((0, 4), dtype=np.uint64))
            # level[j] = L_(nu-j): the table, then the tree's levels in product_tree's layout
            level = [f.evaluations] + [DeviceSegment(tree, n - (n >> (j - 1)), n >> j) for j in range(1, nu + 1)]
            pair = level[nu - 1].to_host()                # L_1
            point = _element(challenge(0, None, pair)).copy().reshape(1, 4)
            layers = [(None, pair)]
            one = _one(f.field)
            for k in range(1, nu):
                up = level[nu - k - 1]                    # L_(k+1): its halves are views, no copy
                eq = DenseMultilinearExtension.eq(f.field, point)
                lp = ListOfProducts(f.field, k)
                try:
                    left = DenseMultilinearExtension(k, DeviceSegment(up, 0, 1 << k))
                    right = DenseMultilinearExtension(k, DeviceSegment(up, 1 << k, 1 << k))
                    lp.add_product([eq, left, right], one)
                    proof = sumcheck(lp, k)
                finally:
                    lp.free()
                    eq.free()
                pair = proof.final_evaluations[1:3].copy()
                tau = _element(challenge(k, None, pair)).copy()
                point = np.concatenate([proof.point, tau.reshape(1, 4)])
                layers.append((proof, pair))
            return GrandProductProof(product, layers, point)
        finally:
            tree.free()
