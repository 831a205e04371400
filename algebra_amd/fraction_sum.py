"""The layered proof of a sum of fractions P / Q = sum_b num[b] / den[b] over device-resident tables (the GKR form of logUp,
Papini-Haboeck) -- the Python mirror of `FractionalSum` in include/ark_hip.hpp and
rust/ark-hip/src/fraction_sum.rs.

`fraction_tree` gives the levels N_nu = num, D_nu = den,

    N_k[i] = N_{k+1}[i] D_{k+1}[i + 2^k] + N_{k+1}[i + 2^k] D_{k+1}[i],     D_k[i] = D_{k+1}[i] D_{k+1}[i + 2^k],

(N_0[0], D_0[0]) = (P, Q).  The halves n0, n1, d0, d1 of the levels above are their polynomials with the LAST variable at 0
and at 1, so for r in F^k and a batching challenge lambda

    N_k(r) + lambda D_k(r) = sum_{x in {0,1}^k} eq(r, x) (n0(x) d1(x) + n1(x) d0(x) + lambda d0(x) d1(x)):

one sumcheck of three products over five tables per layer, which reduces the two claims to n0, n1, d0, d1 at rho, and the
lines through the halves at tau to claims about N_{k+1}(rho, tau) and D_{k+1}(rho, tau).  The last claims are num(point) and
den(point), which `evaluate` / `open` answer.  With ones for numerators the level above the last layer is the leaves: its
products are eq d1, eq d0 and lambda eq d0 d1 over three tables.  No arithmetic happens here and nothing is hashed: the
challenges come from the caller, verification is the caller's (the tests carry a verifier)."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .grand_product import _one
from .mle import DenseMultilinearExtension, DeviceSegment, _element
from .poly import DeviceVec
from .sumcheck import ListOfProducts, sumcheck_prove_plan

# what `challenge` gets as its round when the layer's batching challenge lambda is asked for, before the layer's sumcheck
# (None asks for the layer's tau, as in GrandProduct.prove); the C++ and Rust mirrors use -2 (LAMBDA_ROUND) and -1
LAMBDA = "lambda"


class FractionalSumProof:
    """what prove() returns: `root` = (P, Q) (uint64 [2, 4]); `layers[k]` = (SumcheckProof of layer k -- None for k = 0 --,
    values): numpy uint64 [4, 4] = (n0, n1, d0, d1) -- the two elements each of N_1 and D_1 for k = 0, else the halves at the
    sumcheck's point --, or [2, 4] = (d0, d1) where the numerators are the implicit ones; `point` = r_nu [nu, 4], where the
    verifier's last claims about num and den lie"""

    def __init__(self, root, layers, point):
        self.root, self.layers, self.point = root, layers, point


class FractionalSum:
    def __init__(self, num, den):
        """num: a DenseMultilinearExtension or None for ones; den: a DenseMultilinearExtension of the same size"""
        if not isinstance(den, DenseMultilinearExtension) or not (num is None or isinstance(num, DenseMultilinearExtension)):
            raise TypeError("DenseMultilinearExtensions expected (None for numerators that are all one)")
        if num is not None and (num.field != den.field or num.num_vars != den.num_vars):
            raise ValueError("numerators and denominators differ in field or size")
        self.num, self.den = num, den

    def prove(self, challenge):
        """`challenge(layer, round, values)` returns the verifier's next element (uint64[4], Montgomery): with round = i the
        values are round i's evaluations of the layer's sumcheck; with round = LAMBDA there are no values and the answer is
        the layer's batching challenge; with round = None they are the layer's values and the answer is the layer's tau.
        The tables and the trees are not written."""
        return self._prove(challenge, lambda lp, k: lp.prove(lambda i, evals: challenge(k, i, evals)))

    def prove_device(self, transcript, tail_vars=None):
        """The same proof with every challenge from `transcript` (algebra_amd.Transcript): each layer's sumcheck is one
        ListOfProducts.prove_device -- one wait per layer instead of one per round --; lambda (no values), the layer's values
        and the root's go through transcript.challenge on the host.  One work vector serves every layer.
        tail_vars: as in ListOfProducts.prove_device, for every layer."""
        nu = self.den.num_vars
        work = DeviceVec(self.den.field, sumcheck_prove_plan(nu - 1, 5)[0], _zero=False) if nu >= 2 else None
        try:
            return self._prove(lambda k, rnd, values: transcript.challenge(values), lambda lp, k: lp.prove_device(transcript, tail_vars, _work=work))
        finally:
            if work is not None:
                work.free()

    def _prove(self, challenge, sumcheck):
        """the layers; sumcheck(list of products, layer) -> the layer's SumcheckProof"""
        num, den, nu = self.num, self.den, self.den.num_vars
        n = 1 << nu
        # the trees are this call's own vectors: released on every way out, also when the challenge or a round raises
        trees = [DeviceVec(den.field, n - 1, _zero=False) for _ in range(2)]
        try:
            root = np.zeros((2, 4), dtype=np.uint64)
            check(lib().ark_hip_mle_fraction_tree_device(den.field, None if num is None else num.evaluations.ptr, den.evaluations.ptr,
                                                         nu, trees[0].ptr if nu else None, trees[1].ptr if nu else None,
                                                         root.ctypes.data_as(C.c_void_p)), "ark_hip_mle_fraction_tree_device")
            if nu == 0:
                return FractionalSumProof(root, [], np.zeros((0, 4), dtype=np.uint64))
            # level[j] = level nu-j: the tables (None: the implicit ones), then the trees' levels in fraction_tree's layout
            nlevel = [None if num is None else num.evaluations] + [DeviceSegment(trees[0], n - (n >> (j - 1)), n >> j) for j in range(1, nu + 1)]
            dlevel = [den.evaluations] + [DeviceSegment(trees[1], n - (n >> (j - 1)), n >> j) for j in range(1, nu + 1)]
            values = dlevel[nu - 1].to_host()                # D_1
            if nlevel[nu - 1] is not None:
                values = np.concatenate([nlevel[nu - 1].to_host(), values])   # N_1, D_1
            point = _element(challenge(0, None, values)).copy().reshape(1, 4)
            layers = [(None, values)]
            one = _one(den.field)
            for k in range(1, nu):
                lam = _element(challenge(k, LAMBDA, np.zeros((0, 4), dtype=np.uint64))).copy()
                nup, dup = nlevel[nu - k - 1], dlevel[nu - k - 1]   # levels k+1: their halves are views, no copy
                h = 1 << k
                eq = DenseMultilinearExtension.eq(den.field, point)
                lp = ListOfProducts(den.field, k)
                try:
                    d0 = DenseMultilinearExtension(k, DeviceSegment(dup, 0, h))
                    d1 = DenseMultilinearExtension(k, DeviceSegment(dup, h, h))
                    if nup is None:                          # the leaves with ones for numerators: n0 = n1 = 1
                        lp.add_product([eq, d1], one)
                        lp.add_product([eq, d0], one)
                        lp.add_product([eq, d0, d1], lam)
                        proof = sumcheck(lp, k)
                        values = proof.final_evaluations[[2, 1]].copy()           # tables: eq, d1, d0
                    else:
                        n0 = DenseMultilinearExtension(k, DeviceSegment(nup, 0, h))
                        n1 = DenseMultilinearExtension(k, DeviceSegment(nup, h, h))
                        lp.add_product([eq, n0, d1], one)
                        lp.add_product([eq, n1, d0], one)
                        lp.add_product([eq, d0, d1], lam)
                        proof = sumcheck(lp, k)
                        values = proof.final_evaluations[[1, 3, 4, 2]].copy()     # tables: eq, n0, d1, n1, d0
                finally:
                    lp.free()
                    eq.free()
                tau = _element(challenge(k, None, values)).copy()
                point = np.concatenate([proof.point, tau.reshape(1, 4)])
                layers.append((proof, values))
            return FractionalSumProof(root, layers, point)
        finally:
            for t in trees:
                t.free()
