"""The sumcheck prover over device-resident multilinear tables -- the Python mirror of the two layers of include/ark_hip.hpp
and rust/ark-hip/src/sumcheck.rs.  `ListOfProducts` has the shape of ark-linear-sumcheck's ListOfProductsOfPolynomials: a
list of products of shared `DenseMultilinearExtension`s, each with a coefficient,

    sum_b sum_j c_j prod_{k in term j} f_k(b),

and `round` is one call of ark_hip_sumcheck_round_device on the tables where they lie.  No arithmetic happens here; with
`round` and `prove` nothing is hashed either: the challenges come from the caller.  `prove_device` is the whole proof in one
wait, its challenges derived on the device from a `Transcript` (algebra_amd.transcript).  Verification
is the caller's (the tests carry a verifier)."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib
from .mle import DenseMultilinearExtension, _element
from .poly import DeviceVec

MAX_TABLES, MAX_TERMS, MAX_DEGREE = 8, 8, 4     # ARK_HIP_SUMCHECK_MAX_* of include/ark_hip.h

# prove() binds the challenge inside the round's launch (True) or with the fold kernel before a plain round (False), whichever
# profiles/sumcheck.json measured faster for the tables' size: fused from this many variables on.
FUSED_FROM_NUM_VARS = 0


def sumcheck_plan(num_vars, ntables=1, degree=1, fused=False):
    """(workgroups, pairs of rows one lane walks, reduction stages) of a round over 2^num_vars-element tables"""
    b, p, s = C.c_int(), C.c_int(), C.c_int()
    check(lib().ark_hip_sumcheck_plan(num_vars, ntables, degree, 1 if fused else 0, C.byref(b), C.byref(p), C.byref(s)),
          "ark_hip_sumcheck_plan")
    return b.value, p.value, s.value


def sumcheck_prove_plan(num_vars, ntables=1, tail_vars=None):
    """(elements of work vector, kernel launches, variables left when the one-workgroup tail takes over -- 0: no tail) of
    prove_device over 2^num_vars-element tables; tail_vars None: the library's measured default"""
    w, l, t = C.c_size_t(), C.c_int(), C.c_int()
    check(lib().ark_hip_sumcheck_prove_plan(num_vars, ntables, -1 if tail_vars is None else tail_vars, C.byref(w), C.byref(l), C.byref(t)),
          "ark_hip_sumcheck_prove_plan")
    return w.value, l.value, t.value


class SumcheckProof:
    """what prove() returns: `rounds[i]` = the D + 1 evaluations g_i(0 .. D) (numpy uint64 [D + 1, 4]), `point` = the nu
    challenges [nu, 4], `final_evaluations[k]` = f_k(point) for the tables in the order they were first added, `final_value`
    = sum_j c_j prod_k f_k(point)"""

    def __init__(self, rounds, point, final_evaluations, final_value):
        self.rounds, self.point, self.final_evaluations, self.final_value = rounds, point, final_evaluations, final_value


class ListOfProducts:
    def __init__(self, field, num_vars):
        self.field = cv.field_id(field)
        self.num_vars = int(num_vars)
        self.tables = []            # the distinct DenseMultilinearExtensions, by identity, in the order of first use
        self.products = []          # (coefficient uint64[4], [indices into self.tables])
        self.degree = 0
        self._cur, self._m = None, self.num_vars   # device pointers of the tables as bound so far, and their variables
        self._sets, self._next = None, 0   # the two sets of output DeviceVecs the bound tables alternate between

    def add_product(self, mles, coefficient):
        """adds coefficient * prod mles; an extension used in several products (or twice in one) is one shared table"""
        mles = list(mles)
        if not 1 <= len(mles) <= MAX_DEGREE:
            raise ValueError("a product has 1 to %d factors" % MAX_DEGREE)
        if len(self.products) >= MAX_TERMS:
            raise ValueError("at most %d products" % MAX_TERMS)
        if self._cur is not None:
            raise ValueError("rounds have been run on this list")
        tables, idx = list(self.tables), []
        for m in mles:
            if not isinstance(m, DenseMultilinearExtension):
                raise TypeError("factors are DenseMultilinearExtensions")
            if m.field != self.field:
                raise ValueError("polynomials over different fields")
            if m.num_vars != self.num_vars:
                raise ValueError("num_vars differ: %d and %d" % (m.num_vars, self.num_vars))
            for i, t in enumerate(tables):
                if t is m:
                    idx.append(i)
                    break
            else:
                idx.append(len(tables))
                tables.append(m)
        if len(tables) > MAX_TABLES:
            raise ValueError("at most %d distinct tables" % MAX_TABLES)
        self.tables = tables
        self.products.append((_element(coefficient).copy(), idx))
        self.degree = max(self.degree, len(idx))

    # ---- one round ----------------------------------------------------------------------------------------------
    def _call(self, ptrs, num_vars, r_prev, outs):
        nt, nterms = len(ptrs), len(self.products)
        tabs = (C.c_void_p * nt)(*ptrs)
        lens = (C.c_uint * nterms)(*[len(ix) for _, ix in self.products])
        flat = [i for _, ix in self.products for i in ix]
        term_tables = (C.c_uint * len(flat))(*flat)
        coeffs = np.ascontiguousarray(np.stack([c for c, _ in self.products]), dtype=np.uint64)
        evals = np.zeros((self.degree + 1, 4), dtype=np.uint64)
        r = None if r_prev is None else _element(r_prev)
        out_ptrs = None if outs is None else (C.c_void_p * nt)(*outs)
        check(lib().ark_hip_sumcheck_round_device(self.field, tabs, nt, num_vars, lens, term_tables, coeffs.ctypes.data_as(C.c_void_p),
                                                  nterms, None if r is None else r.ctypes.data_as(C.c_void_p), out_ptrs,
                                                  evals.ctypes.data_as(C.c_void_p)), "ark_hip_sumcheck_round_device")
        return evals

    def round(self, r_prev=None, fused=True):
        """The D + 1 evaluations of the round polynomial over the tables as bound so far.  With `r_prev` (one element) the
        first remaining variable is bound to it first, into tables of the list's own -- the caller's are never written.
        fused=False binds with ark_hip_mle_fix_variables_device and then runs a plain round: the same result in 1 + tables
        launches over the same bytes."""
        if not self.products:
            raise ValueError("no products")
        if self._cur is None:
            self._cur = [t.evaluations.ptr.value for t in self.tables]
        if r_prev is None:
            if self._m == 0:
                raise ValueError("every variable is bound")
            return self._call(self._cur, self._m, None, None)
        if self._m == 0:
            raise ValueError("every variable is bound")
        if self._sets is None:      # halves and quarters: the output of a bind is never the set it reads
            nt = len(self.tables)
            self._sets = [[DeviceVec(self.field, 1 << max(self.num_vars - 1 - s, 0), _zero=False) for _ in range(nt)] for s in (0, 1)]
        outs = [v.ptr.value for v in self._sets[self._next]]
        if fused or self._m == 1:   # the plain entry has no sum over one-element tables
            evals = self._call(self._cur, self._m, r_prev, outs)
        else:
            r = _element(r_prev)
            for src, dst in zip(self._cur, outs):
                check(lib().ark_hip_mle_fix_variables_device(self.field, C.c_void_p(src), self._m, r.ctypes.data_as(C.c_void_p), 1,
                                                             C.c_void_p(dst)), "ark_hip_mle_fix_variables_device")
            evals = self._call(outs, self._m - 1, None, None)
        self._cur, self._m, self._next = outs, self._m - 1, self._next ^ 1
        return evals

    def reset(self):
        """forgets the binds: the next round reads the caller's tables again (the list keeps its own tables for reuse)"""
        self._cur, self._m, self._next = None, self.num_vars, 0

    def bound_pointers(self):
        """device pointers of the tables as bound so far (the caller's before the first bind)"""
        return list(self._cur) if self._cur is not None else [t.evaluations.ptr.value for t in self.tables]

    def bound_tables(self):
        """the tables as bound so far, downloaded: numpy uint64 [tables, 2^(variables left), 4]"""
        if self._cur is None:
            return np.stack([t.to_evaluations() for t in self.tables])
        out = np.empty((len(self._cur), 1 << self._m, 4), dtype=np.uint64)
        for k, p in enumerate(self._cur):
            check(lib().ark_hip_memcpy_d2h(out[k].ctypes.data_as(C.c_void_p), C.c_void_p(p), out[k].nbytes), "ark_hip_memcpy_d2h")
        return out

    # ---- the whole prover ---------------------------------------------------------------------------------------
    def prove(self, challenge, fused=None):
        """Runs the nu + 1 calls: call 0 has no bind, calls 1 .. nu bind the challenge before.  `challenge(i, evals)` gets
        round i's evaluations and returns the verifier's element r_(i+1) (uint64[4], Montgomery): the transcript is the
        caller's.  fused: None picks per size what was measured faster."""
        if self._cur is not None:
            raise ValueError("rounds have been run on this list")
        if self.num_vars == 0:
            raise ValueError("nothing to sum over: num_vars == 0")
        rounds, point = [], []
        evals = self.round()
        for i in range(self.num_vars):
            rounds.append(evals)
            r = _element(challenge(i, evals)).copy()
            point.append(r)
            evals = self.round(r, fused=(self._m >= FUSED_FROM_NUM_VARS) if fused is None else fused)
        finals = self.bound_tables()[:, 0, :]
        return SumcheckProof(rounds, np.stack(point), finals, evals[0].copy())

    def prove_device(self, transcript, tail_vars=None, _work=None):
        """The whole proof in one wait: what prove() returns when its challenge is
        `transcript.challenge(evals)`, with the challenges derived on the device -- one call of
        ark_hip_sumcheck_prove_device.  Advances `transcript` by the nu challenges.  The work vector for the bound tables is
        allocated and freed here (_work: a caller's DeviceVec of at least sumcheck_prove_plan's elements, kept across proofs).
        tail_vars: see sumcheck_prove_plan; tests move the seam with it."""
        if self._cur is not None:
            raise ValueError("rounds have been run on this list")
        if not self.products:
            raise ValueError("no products")
        if self.num_vars == 0:
            raise ValueError("nothing to sum over: num_vars == 0")
        if transcript.field != self.field:
            raise ValueError("the transcript is over another field")
        nt, nterms, nu, d1 = len(self.tables), len(self.products), self.num_vars, self.degree + 1
        elems = sumcheck_prove_plan(nu, nt, tail_vars)[0]
        if _work is not None and _work.len < elems:
            raise ValueError("the work vector has %d elements, %d are needed" % (_work.len, elems))
        work = _work if _work is not None else DeviceVec(self.field, elems, _zero=False)
        try:
            tabs = (C.c_void_p * nt)(*[t.evaluations.ptr.value for t in self.tables])
            lens = (C.c_uint * nterms)(*[len(ix) for _, ix in self.products])
            flat = [i for _, ix in self.products for i in ix]
            term_tables = (C.c_uint * len(flat))(*flat)
            coeffs = np.ascontiguousarray(np.stack([c for c, _ in self.products]), dtype=np.uint64)
            rounds, point = np.zeros((nu, d1, 4), dtype=np.uint64), np.zeros((nu, 4), dtype=np.uint64)
            finals, value = np.zeros((nt, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
            check(lib().ark_hip_sumcheck_prove_device(self.field, tabs, nt, nu, lens, term_tables, coeffs.ctypes.data_as(C.c_void_p), nterms,
                                                      C.cast(transcript._state, C.c_void_p), -1 if tail_vars is None else tail_vars, work.ptr,
                                                      rounds.ctypes.data_as(C.c_void_p), point.ctypes.data_as(C.c_void_p),
                                                      finals.ctypes.data_as(C.c_void_p), value.ctypes.data_as(C.c_void_p)),
                  "ark_hip_sumcheck_prove_device")
        finally:
            if _work is None:
                work.free()
        return SumcheckProof([rounds[i] for i in range(nu)], point, finals, value)

    def free(self):
        """releases the list's own bound tables (not the caller's extensions)"""
        for s in self._sets or []:
            for v in s:
                v.free()
        self._sets = None
        self.reset()
