"""Gate expressions on device vectors -- the Python mirror of `SumOfProducts` in include/ark_hip.hpp and
rust/ark-hip/src/device.rs.  The row-by-row constraint expression of a univariate (Plonk-style) prover over a domain or an
extended coset: a sum of products of columns, each factor read at a rotation,

    out[i] = c0 + sum_j c_j prod_q col_{j,q}[(i + rot_{j,q}) mod n],

in one call of ark_hip_fr_sum_of_products_device on the columns where they lie.  No arithmetic happens
here."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib
from .poly import DeviceVec

MAX_COLUMNS, MAX_TERMS, MAX_DEGREE = 16, 16, 8     # ARK_HIP_SOP_MAX_* of include/ark_hip.h
_I64 = (-(1 << 63), (1 << 63) - 1)


def sum_of_products_plan(n):
    """(workgroups, rows one lane walks) of SumOfProducts.evaluate over n rows (ark_hip_fr_sum_of_products_plan; host only)"""
    b, r = C.c_int(), C.c_int()
    check(lib().ark_hip_fr_sum_of_products_plan(n, C.byref(b), C.byref(r)), "ark_hip_fr_sum_of_products_plan")
    return b.value, r.value


def _one(field):
    p = cv.SCALAR_MODULUS[cv.FIELDS[field]]
    return np.frombuffer(((1 << 256) % p).to_bytes(32, "little"), dtype="<u8").astype(np.uint64)


class SumOfProducts:
    def __init__(self, field, n):
        self.field = cv.field_id(field)
        if cv.FIELDS[self.field] not in cv.SCALAR_MODULUS:
            raise ValueError("not a scalar field")
        self.n = int(n)
        if self.n < 0:
            raise ValueError("a negative length")
        self.columns = []           # the distinct DeviceVecs, by device pointer, in the order of first use
        self.products = []          # (coefficient uint64[4], [(index into self.columns, rotation)])
        self.constant = None

    def add_product(self, factors, coefficient=None):
        """adds coefficient * prod factors; a factor is a DeviceVec (rotation 0) or a (DeviceVec, rotation) pair, the rotation
        any integer an int64 holds.  coefficient None: one.  A vector used in several products, or several times in one, is
        one shared column."""
        factors = list(factors)
        if not 1 <= len(factors) <= MAX_DEGREE:
            raise ValueError("a product has 1 to %d factors" % MAX_DEGREE)
        if len(self.products) >= MAX_TERMS:
            raise ValueError("at most %d products" % MAX_TERMS)
        columns, idx = list(self.columns), []
        for f in factors:
            v, rot = f if isinstance(f, tuple) else (f, 0)
            if not isinstance(v, DeviceVec):
                raise TypeError("factors are DeviceVecs or (DeviceVec, rotation) pairs")
            rot = int(rot)
            if not _I64[0] <= rot <= _I64[1]:
                raise ValueError("a rotation is an int64")
            if v.field != self.field:
                raise ValueError("vectors over different fields")
            if v.len != self.n:
                raise ValueError("lengths differ: %d and %d" % (v.len, self.n))
            for i, c in enumerate(columns):
                if c.ptr.value == v.ptr.value:
                    idx.append((i, rot))
                    break
            else:
                idx.append((len(columns), rot))
                columns.append(v)
        if len(columns) > MAX_COLUMNS:
            raise ValueError("at most %d distinct columns" % MAX_COLUMNS)
        c = _one(self.field) if coefficient is None else np.ascontiguousarray(coefficient, dtype=np.uint64).reshape(4).copy()
        self.columns = columns
        self.products.append((c, idx))
        return self

    def set_constant(self, c0):
        """the constant term c0 (one element); None takes it away"""
        self.constant = None if c0 is None else np.ascontiguousarray(c0, dtype=np.uint64).reshape(4).copy()
        return self

    def evaluate(self, out=None):
        """the expression's n rows as a DeviceVec; asynchronous.  out: the vector to write -- one of the columns only if every
        factor reads that column at a rotation that is 0 mod n -- or a new one."""
        if not self.products:
            raise ValueError("no products")
        if out is None:
            out = DeviceVec(self.field, self.n, _zero=False)
        elif not isinstance(out, DeviceVec) or out.field != self.field or out.len != self.n:
            raise ValueError("the output is a DeviceVec of %d elements over the same field" % self.n)
        if self.n == 0:
            return out
        _call(self.field, [c.ptr.value for c in self.columns], self.n, self.products, self.constant, out.ptr)
        return out


def _call(field, ptrs, n, products, constant, out_ptr):
    """one call of the entry; products: (coefficient, [(column, rotation)]) per term"""
    nterms = len(products)
    cols = (C.c_void_p * len(ptrs))(*ptrs)
    lens = (C.c_uint * nterms)(*[len(ix) for _, ix in products])
    flat = [f for _, ix in products for f in ix]
    term_columns = (C.c_uint * len(flat))(*[k for k, _ in flat])
    rots = (C.c_int64 * len(flat))(*[r for _, r in flat]) if any(r for _, r in flat) else None
    coeffs = np.ascontiguousarray(np.stack([c for c, _ in products]), dtype=np.uint64)
    check(lib().ark_hip_fr_sum_of_products_device(field, cols, len(ptrs), n, lens, term_columns, rots, coeffs.ctypes.data_as(C.c_void_p),
                                                  nterms, None if constant is None else constant.ctypes.data_as(C.c_void_p), out_ptr),
          "ark_hip_fr_sum_of_products_device")

