"""DenseMultilinearExtension on a device-resident evaluation table -- the Python mirror of ark_poly's type of that name
(poly/src/evaluations/multivariate/multilinear/dense.rs; C++: include/ark_hip.hpp, Rust: rust/ark-hip/src/mle.rs).  The table
of 2^num_vars Montgomery elements is a `DeviceVec`: committing to it is an MSM on `evaluations.ptr` with Montgomery
scalars, binding variables (`fix_variables`, `evaluate`) runs on it where it lies.  Index bit 0 is the first variable.
No arithmetic happens here: scalars are handed to the library as they are."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib
from .poly import DeviceVec


def mle_fold_plan(num_vars, dim):
    """(tile_log, [variables bound by each launch]) of fix_variables / evaluate for `dim` variables of a 2^num_vars table"""
    t, ps = C.c_int(), C.c_int()
    widths = (C.c_int * 8)()
    check(lib().ark_hip_mle_fold_plan(num_vars, dim, C.byref(t), C.byref(ps), widths), "ark_hip_mle_fold_plan")
    return t.value, [widths[i] for i in range(ps.value)]


def mle_fold_tiles(num_vars, dim):
    """[log2 of the tiles one wave takes] for each launch of mle_fold_plan(num_vars, dim): which kernel variant runs"""
    tiles = (C.c_int * 8)()
    check(lib().ark_hip_mle_fold_tiles(num_vars, dim, tiles), "ark_hip_mle_fold_tiles")
    return [tiles[i] for i in range(len(mle_fold_plan(num_vars, dim)[1]))]


def _plan5(entry, num_vars):
    t, ps = C.c_int(), C.c_int()
    widths, tiles = (C.c_int * 8)(), (C.c_int * 8)()
    check(getattr(lib(), entry)(num_vars, C.byref(t), C.byref(ps), widths, tiles), entry)
    return t.value, [widths[i] for i in range(ps.value)], [tiles[i] for i in range(ps.value)]


def mle_eq_plan(num_vars):
    """(tile_log, [variables of each launch], [log2 of the tiles one wave takes in it]) of DenseMultilinearExtension.eq:
    launch p writes the table of the top widths[0] + .. + widths[p] variables"""
    return _plan5("ark_hip_mle_eq_plan", num_vars)


def mle_quotients_plan(num_vars):
    """(tile_log, [variables bound by each launch], [log2 of the tiles one wave takes in it]) of `quotients`"""
    return _plan5("ark_hip_mle_quotients_plan", num_vars)


PRODUCT_TREE_LEVELS = 3     # ARK_HIP_PRODUCT_TREE_LEVELS of include/ark_hip.h: the most levels one launch forms


def mle_product_tree_plan(num_vars):
    """([levels of each run of launches], [log2 of the chunks of 64 outputs one wave takes in them: always 0]) of
    `product_tree`, as ark_hip_mle_product_tree_plan reports them: the full launches as one run, then the remainder launch"""
    ps = C.c_int()
    widths, groups = (C.c_int * 8)(), (C.c_int * 8)()
    check(lib().ark_hip_mle_product_tree_plan(num_vars, C.byref(ps), widths, groups), "ark_hip_mle_product_tree_plan")
    return [widths[i] for i in range(ps.value)], [groups[i] for i in range(ps.value)]


def mle_product_tree_launches(num_vars):
    """[(levels, group_log)] launch by launch: the runs of mle_product_tree_plan spelled out"""
    out = []
    for w, g in zip(*mle_product_tree_plan(num_vars)):
        out += [(PRODUCT_TREE_LEVELS, g)] * (w // PRODUCT_TREE_LEVELS) if w >= PRODUCT_TREE_LEVELS else [(w, g)]
    return out


FRACTION_TREE_LEVELS = 2    # ARK_HIP_FRACTION_TREE_LEVELS of include/ark_hip.h: the most levels one launch forms


def mle_fraction_tree_plan(num_vars, has_num=True):
    """([levels of each run of launches], [always 0]) of `fraction_tree`, as ark_hip_mle_fraction_tree_plan reports them: the
    full launches as one run, then the remainder launch"""
    ps = C.c_int()
    widths, groups = (C.c_int * 8)(), (C.c_int * 8)()
    check(lib().ark_hip_mle_fraction_tree_plan(num_vars, 1 if has_num else 0, C.byref(ps), widths, groups),
          "ark_hip_mle_fraction_tree_plan")
    return [widths[i] for i in range(ps.value)], [groups[i] for i in range(ps.value)]


def mle_fraction_tree_launches(num_vars, has_num=True):
    """[(levels, numerators are read)] launch by launch: the runs of mle_fraction_tree_plan spelled out; only the first
    launch of a sum with ones for numerators reads none"""
    out = []
    for w in mle_fraction_tree_plan(num_vars, has_num)[0]:
        out += [FRACTION_TREE_LEVELS] * (w // FRACTION_TREE_LEVELS) if w >= FRACTION_TREE_LEVELS else [w]
    return [(w, bool(has_num) or i > 0) for i, w in enumerate(out)]


LOOKUP_MISSING = 0xFFFFFFFF     # ARK_HIP_LOOKUP_MISSING of include/ark_hip.h: the index of a witness cell that is not in the table


def lookup_plan(table_len):
    """(capacity_log, scratch_bytes) of `lookup` against a table of table_len values, as ark_hip_fr_lookup_plan reports them:
    2^capacity_log >= 2 table_len slots are hashed into per call, in scratch_bytes of the context's scratch"""
    c, b = C.c_uint(), C.c_size_t()
    check(lib().ark_hip_fr_lookup_plan(int(table_len), C.byref(c), C.byref(b)), "ark_hip_fr_lookup_plan")
    return c.value, b.value


class DeviceSegment:
    """`len` elements inside a DeviceVec, from element `offset` on: a view, no copy.  `ptr` is a device pointer that the
    MSM's device entries accept as a scalar vector; the view keeps its owner alive."""

    def __init__(self, owner, offset, length):
        self.owner, self.offset, self.len, self.field = owner, int(offset), int(length), owner.field
        self.ptr = C.c_void_p(owner.ptr.value + 32 * self.offset if self.len else 0)

    def __len__(self):
        return self.len

    def to_host(self):
        out = np.empty((self.len, 4), dtype=np.uint64)
        if self.len:
            check(lib().ark_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes), "ark_hip_memcpy_d2h")
        return out

    def free(self):
        """a view owns nothing: the memory goes with its owner (so a DenseMultilinearExtension over a view frees nothing)"""


def _device_pointer(x):
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if hasattr(x, "ptr"):
        return x.ptr
    return x if isinstance(x, C.c_void_p) else C.c_void_p(int(x))


def _element(x):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(4)


def _elements(xs, count=None):
    a = np.ascontiguousarray(xs, dtype=np.uint64).reshape(-1, 4)
    if count is not None and a.shape[0] != count:
        raise ValueError("the point has %d coordinates, %d expected" % (a.shape[0], count))
    return a


class DenseMultilinearExtension:
    def __init__(self, num_vars, evaluations):
        """takes ownership of the DeviceVec `evaluations` (from_evaluations_vec, dense.rs:58-70)"""
        if len(evaluations) != 1 << num_vars:
            raise ValueError("The size of evaluations should be 2^num_vars.")   # the reference's assertion
        self.num_vars = int(num_vars)
        self.evaluations = evaluations
        self.field = evaluations.field

    @classmethod
    def from_evaluations(cls, field, num_vars, evaluations):
        """numpy uint64 [2^num_vars, 4] (Montgomery) -> one upload"""
        a = _elements(evaluations)
        if a.shape[0] != 1 << num_vars:
            raise ValueError("The size of evaluations should be 2^num_vars.")
        return cls(num_vars, DeviceVec.from_host(field, a))

    @classmethod
    def zero(cls, field):
        """the constant zero: num_vars = 0 and one zero evaluation (dense.rs:422-427)"""
        return cls(0, DeviceVec(field, 1))

    def is_zero(self):
        """num_vars == 0 and the evaluation is zero (dense.rs:429-431): a 32-byte download, and only when num_vars == 0"""
        return self.num_vars == 0 and not self.evaluations.to_host().any()

    def to_evaluations(self):
        return self.evaluations.to_host()

    def clone(self):
        return DenseMultilinearExtension(self.num_vars, self.evaluations.clone())

    def free(self):
        self.evaluations.free()

    def __len__(self):
        return len(self.evaluations)

    def commit(self, wait=True):
        """MerkleTree.commit_fr of the evaluation table as one column (merkle.py)"""
        return self.evaluations.commit(wait=wait)

    # ---- binding variables --------------------------------------------------------------------------------------
    def fix_variables(self, partial_point):
        """binds the first len(partial_point) variables (dense.rs:224-257); a new polynomial, self is left as it is"""
        pt = _elements(partial_point)
        dim = pt.shape[0]
        if dim > self.num_vars:
            raise ValueError("invalid size of partial point")
        out = DeviceVec(self.field, 1 << (self.num_vars - dim), _zero=False)
        check(lib().ark_hip_mle_fix_variables_device(self.field, self.evaluations.ptr, self.num_vars, pt.ctypes.data_as(C.c_void_p),
                                                     dim, out.ptr), "ark_hip_mle_fix_variables_device")
        return DenseMultilinearExtension(self.num_vars - dim, out)

    def evaluate(self, point):
        """the value at `point` (num_vars coordinates) as a numpy uint64[4]; waits for it (dense.rs:460-465)"""
        pt = _elements(point, self.num_vars)
        out = np.zeros(4, dtype=np.uint64)
        check(lib().ark_hip_mle_evaluate_device(self.field, self.evaluations.ptr, self.num_vars, pt.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p)), "ark_hip_mle_evaluate_device")
        return out

    # ---- openings ------------------------------------------------------------------------
    @classmethod
    def eq(cls, field, point, scale=None):
        """the table eq(point, b) = prod_i (b_i ? point_i : 1 - point_i), times `scale` (an element; None: one), built on
        the device: <f, eq(r)> = f(r).  point: numpy uint64 [num_vars, 4] (Montgomery)"""
        pt = _elements(point)
        num_vars = pt.shape[0]
        out = DeviceVec(field, 1 << num_vars, _zero=False)
        k = None if scale is None else _element(scale)
        check(lib().ark_hip_mle_eq_table_device(out.field, pt.ctypes.data_as(C.c_void_p), num_vars,
                                                None if k is None else k.ctypes.data_as(C.c_void_p), out.ptr),
              "ark_hip_mle_eq_table_device")
        return cls(num_vars, out)

    def quotients(self, point, wait=True):
        """(f(point), [q_0, .., q_{num_vars-1}]) with f(x) - f(point) = sum_i (x_i - point_i) q_i(x_{i+1}, ..): q_i is a
        DeviceSegment of 2^(num_vars-1-i) elements, all of them views into one DeviceVec.  wait=False returns None for the
        value and leaves the call asynchronous."""
        pt = _elements(point, self.num_vars)
        n = 1 << self.num_vars
        quot = DeviceVec(self.field, n - 1, _zero=False)
        out = np.zeros(4, dtype=np.uint64) if wait else None
        check(lib().ark_hip_mle_quotients_device(self.field, self.evaluations.ptr, self.num_vars, pt.ctypes.data_as(C.c_void_p),
                                                 quot.ptr, out.ctypes.data_as(C.c_void_p) if wait else None),
              "ark_hip_mle_quotients_device")
        return out, [DeviceSegment(quot, n - (n >> i), n >> (i + 1)) for i in range(self.num_vars)]

    def open(self, point, bases_per_level, curve):
        """(f(point), [commitment to q_i for every i]): `quotients`, then one device MSM per level over the segment where it
        lies.  bases_per_level[i]: a device array (pointer, tensor or DeviceVec-like) of 2^(num_vars-1-i) affine points of
        `curve`, whose scalar field is the table's.  The points are Jacobian x|y|z as the MSM returns them.  No
        verification and no hashing happens here."""
        cid = cv.curve_id(curve)
        if cv.field_id(cv.scalar_field(cid)) != self.field:
            raise ValueError("the curve's scalar field is not the table's field")
        if len(bases_per_level) != self.num_vars:
            raise ValueError("one base array per variable expected")
        value, segments = self.quotients(point)
        points = []
        for seg, bases in zip(segments, bases_per_level):
            out = np.zeros(cv.projective_words(cid), dtype=np.uint64)
            check(lib().ark_hip_msm_sw_device(cid, _device_pointer(bases), seg.ptr, len(seg), 1, out.ctypes.data_as(C.c_void_p)),
                  "ark_hip_msm_sw_device")
            points.append(out)
        return value, points

    # ---- grand products ------------------------------------------------------------------
    def product_tree(self, wait=True):
        """(product, [level_1, .., level_nu]): the binary product tree pairing over the LAST variable.  level_j has
        2^(num_vars-j) elements, level_j[i] = level_(j-1)[i] * level_(j-1)[i + 2^(num_vars-j)] with level_0 the table; all
        are DeviceSegments of one DeviceVec of 2^num_vars - 1 elements whose last is the product.  wait=False returns None
        for the product and leaves the call asynchronous.  The table is not written."""
        n = 1 << self.num_vars
        tree = DeviceVec(self.field, n - 1, _zero=False)
        out = np.zeros(4, dtype=np.uint64) if wait else None
        check(lib().ark_hip_mle_product_tree_device(self.field, self.evaluations.ptr, self.num_vars, tree.ptr if n > 1 else None,
                                                    out.ctypes.data_as(C.c_void_p) if wait else None),
              "ark_hip_mle_product_tree_device")
        return out, [DeviceSegment(tree, n - (n >> (j - 1)), n >> j) for j in range(1, self.num_vars + 1)]

    @classmethod
    def linear_combination(cls, tables, coeffs, c0=None):
        """the new extension c0 + sum_k coeffs[k] tables[k], entry by entry in one pass: 1 to 8 extensions of one field and
        size; coeffs: numpy uint64 [len(tables), 4] (Montgomery); c0: an element or None for zero"""
        tables = list(tables)
        if not 1 <= len(tables) <= 8:
            raise ValueError("1 to 8 tables")
        first = tables[0]
        for t in tables:
            if t.field != first.field:
                raise ValueError("polynomials over different fields")
            if t.num_vars != first.num_vars:
                raise ValueError("num_vars differ: %d and %d" % (t.num_vars, first.num_vars))
        k = _elements(coeffs, len(tables))
        g = None if c0 is None else _element(c0)
        out = DeviceVec(first.field, len(first), _zero=False)
        ptrs = (C.c_void_p * len(tables))(*[t.evaluations.ptr.value for t in tables])
        check(lib().ark_hip_fr_lincomb_device(first.field, ptrs, len(tables), k.ctypes.data_as(C.c_void_p),
                                              None if g is None else g.ctypes.data_as(C.c_void_p), out.ptr, len(out)),
              "ark_hip_fr_lincomb_device")
        return cls(first.num_vars, out)

    # ---- fractional sums -------------------------------------------------------------------
    def fraction_tree(self, num=None, wait=True):
        """(root, [num_level_1, ..], [den_level_1, ..]) of the sum of fractions num[b] / self[b]: the tree that adds
        fractions pairing over the LAST variable, N = n0 d1 + n1 d0, D = d0 d1.  `num`: an extension of the same size, or
        None for ones.  level_j has 2^(num_vars-j) elements; the levels of a tree are DeviceSegments of one DeviceVec of
        2^num_vars - 1 elements in product_tree's layout.  root: numpy uint64 [2, 4] = (P, Q) with P / Q the sum; wait=False
        returns None for it and leaves the call asynchronous.  Nothing is inverted; the tables are not written."""
        if num is not None:
            if num.field != self.field:
                raise ValueError("polynomials over different fields")
            if num.num_vars != self.num_vars:
                raise ValueError("num_vars differ: %d and %d" % (num.num_vars, self.num_vars))
        n = 1 << self.num_vars
        trees = [DeviceVec(self.field, n - 1, _zero=False) for _ in range(2)]
        out = np.zeros((2, 4), dtype=np.uint64) if wait else None
        check(lib().ark_hip_mle_fraction_tree_device(self.field, None if num is None else num.evaluations.ptr, self.evaluations.ptr,
                                                     self.num_vars, trees[0].ptr if n > 1 else None, trees[1].ptr if n > 1 else None,
                                                     out.ctypes.data_as(C.c_void_p) if wait else None),
              "ark_hip_mle_fraction_tree_device")
        levels = [[DeviceSegment(t, n - (n >> (j - 1)), n >> j) for j in range(1, self.num_vars + 1)] for t in trees]
        return out, levels[0], levels[1]

    @staticmethod
    def count_indices(field, indices, table_len):
        """the multiplicity table of a lookup: m[j] = #{i : indices[i] = j} for j < table_len as Montgomery elements, counted
        on the device.  indices: numpy uint32 [n] (one upload).  An index >= table_len is skipped and not reported: the
        counts sum to n exactly when none was skipped.  -> a new DenseMultilinearExtension when table_len is a power of two,
        else a DeviceVec."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        table_len = int(table_len)
        if table_len < 1:
            raise ValueError("table_len must be positive")
        out = DeviceVec(field, table_len, _zero=False)
        d_idx = C.c_void_p(0)
        try:
            if idx.size:
                check(lib().ark_hip_malloc(idx.nbytes, C.byref(d_idx)), "ark_hip_malloc")
                check(lib().ark_hip_memcpy_h2d(d_idx, idx.ctypes.data_as(C.c_void_p), idx.nbytes), "ark_hip_memcpy_h2d")
            check(lib().ark_hip_fr_count_indices_device(out.field, d_idx if idx.size else None, idx.size, out.ptr, table_len),
                  "ark_hip_fr_count_indices_device")
        except Exception:
            out.free()
            raise
        finally:
            if d_idx.value:
                check(lib().ark_hip_free(d_idx), "ark_hip_free")
        if table_len & (table_len - 1) == 0:
            return DenseMultilinearExtension(table_len.bit_length() - 1, out)
        return out

    # ---- lookup by value ------------------------------------------------------------------
    @staticmethod
    def lookup(table, values, indices=False, multiplicities=True, wait=True):
        """the join of a lookup on the device, from the values: `table` and `values` are device vectors of one field (a
        DeviceVec, an extension or a DeviceSegment).  -> (m, missing, idx):
          m        m[j] = #{i : values[i] is found at j}, j the FIRST occurrence of the value in the table (a repeated table
                   value keeps zero in its later cells): a new DenseMultilinearExtension when len(table) is a power of two,
                   else a DeviceVec; None with multiplicities=False;
          missing  the number of cells of `values` that are not in the table; None with wait=False, which leaves the call
                   asynchronous;
          idx      numpy uint32 [len(values)], LOOKUP_MISSING where not found; downloaded only with indices=True, else None.
        At least one of the three must be asked for."""
        table = getattr(table, "evaluations", table)
        values = getattr(values, "evaluations", values)
        if table.field != values.field:
            raise ValueError("vectors over different fields")
        table_len, n = len(table), len(values)
        if table_len < 1:
            raise ValueError("the table is empty")
        if not (indices or multiplicities or wait):
            raise ValueError("nothing is asked for")
        out = DeviceVec(table.field, table_len, _zero=False) if multiplicities else None
        d_idx = C.c_void_p(0)
        missing = C.c_uint64(0)
        idx = None
        try:
            if indices and n:
                check(lib().ark_hip_malloc(4 * n, C.byref(d_idx)), "ark_hip_malloc")
            check(lib().ark_hip_fr_lookup_device(table.field, _device_pointer(table), table_len, _device_pointer(values) if n else None, n,
                                                 d_idx if d_idx.value else None, out.ptr if multiplicities else None,
                                                 C.byref(missing) if wait or not (d_idx.value or multiplicities) else None),
                  "ark_hip_fr_lookup_device")
            if indices:
                idx = np.empty(n, dtype=np.uint32)
                if n:
                    check(lib().ark_hip_memcpy_d2h(idx.ctypes.data_as(C.c_void_p), d_idx, idx.nbytes), "ark_hip_memcpy_d2h")
        except Exception:
            if out is not None:
                out.free()
            raise
        finally:
            if d_idx.value:
                check(lib().ark_hip_free(d_idx), "ark_hip_free")
        if out is not None and table_len & (table_len - 1) == 0:
            out = DenseMultilinearExtension(table_len.bit_length() - 1, out)
        return out, (missing.value if wait else None), idx

    # ---- relabel ------------------------------------------------------------------------------------------------
    def _relabel(self, a, b, k, dst):
        lo, hi = min(a, b), max(a, b)
        if lo != hi and k != 0:
            if hi + k > self.num_vars:
                raise ValueError("invalid relabel argument")
            if lo + k > hi:
                raise ValueError("overlapped swap window is not allowed")
        check(lib().ark_hip_mle_relabel_device(self.field, self.evaluations.ptr, self.num_vars, a, b, k, dst.ptr),
              "ark_hip_mle_relabel_device")

    def relabel(self, a, b, k):
        """exchanges the k variables from position a with those from position b (dense.rs:195-199); a new polynomial"""
        out = DeviceVec(self.field, len(self.evaluations), _zero=False)
        self._relabel(a, b, k, out)
        return DenseMultilinearExtension(self.num_vars, out)

    def relabel_in_place(self, a, b, k):
        self._relabel(a, b, k, self.evaluations)
        return self

    # ---- concat -------------------------------------------------------------------------------------------------
    @classmethod
    def concat(cls, polys):
        """the tables one after the other, zero-filled up to the next power of two (dense.rs:133-156)"""
        polys = list(polys)
        if not polys:
            raise ValueError("concat of no polynomials")
        field = polys[0].field
        total = sum(len(p) for p in polys)
        num_vars = max(total - 1, 0).bit_length()
        out = DeviceVec(field, 1 << num_vars, _zero=False)
        L, at = lib(), 0
        for p in polys:
            if p.field != field:
                raise ValueError("polynomials over different fields")
            check(L.ark_hip_memcpy_d2d(C.c_void_p(out.ptr.value + at * 32), p.evaluations.ptr, len(p) * 32), "ark_hip_memcpy_d2d")
            at += len(p)
        if at < len(out):
            check(L.ark_hip_memset_device(C.c_void_p(out.ptr.value + at * 32), 0, (len(out) - at) * 32), "ark_hip_memset_device")
        return cls(num_vars, out)

    # ---- the vector space ---------------------------------------------------------------------------------------
    def _pointwise(self, entry, other):
        if other.field != self.field:
            raise ValueError("polynomials over different fields")
        out = DeviceVec(self.field, len(self.evaluations), _zero=False)
        check(getattr(lib(), entry)(self.field, self.evaluations.ptr, other.evaluations.ptr, out.ptr, len(out)), entry)
        return DenseMultilinearExtension(self.num_vars, out)

    def __add__(self, rhs):
        """dense.rs:286-305: the constant zero on either side gives a copy of the other, whatever its num_vars"""
        if rhs.is_zero():
            return self.clone()
        if self.is_zero():
            return rhs.clone()
        if self.num_vars != rhs.num_vars:
            raise ValueError("num_vars differ: %d and %d" % (self.num_vars, rhs.num_vars))
        return self._pointwise("ark_hip_fr_add_device", rhs)

    def __neg__(self):
        out = DeviceVec(self.field, len(self.evaluations), _zero=False)
        check(lib().ark_hip_fr_neg_device(self.field, self.evaluations.ptr, out.ptr, len(out)), "ark_hip_fr_neg_device")
        return DenseMultilinearExtension(self.num_vars, out)

    def __sub__(self, rhs):
        """self + (-rhs), with the zero cases of + (dense.rs:348-354)"""
        if rhs.is_zero():
            return self.clone()
        if self.is_zero():
            return -rhs
        if self.num_vars != rhs.num_vars:
            raise ValueError("num_vars differ: %d and %d" % (self.num_vars, rhs.num_vars))
        return self._pointwise("ark_hip_fr_sub_device", rhs)

    def __mul__(self, scalar):
        """times one field element (numpy uint64[4], Montgomery); times zero gives zero() (dense.rs:376-392)"""
        k = _element(scalar)
        if not k.any():
            return DenseMultilinearExtension.zero(self.field)
        out = DeviceVec(self.field, len(self.evaluations), _zero=False)
        check(lib().ark_hip_fr_scale_device(self.field, self.evaluations.ptr, k.ctypes.data_as(C.c_void_p), out.ptr, len(out)),
              "ark_hip_fr_scale_device")
        return DenseMultilinearExtension(self.num_vars, out)

    def __iadd__(self, rhs):
        """`+= other` and `+= (f, other)`: self + f other in one pass over the tables (dense.rs:307-327)"""
        if not isinstance(rhs, tuple):
            new = self + rhs
        else:
            f, other = rhs
            k = _element(f)
            if other.is_zero() or (other.num_vars == 0 and not k.any()):      # f other is the constant zero
                return self
            if self.is_zero():                                                # the scaled table itself, also when f is zero
                out = DeviceVec(self.field, len(other.evaluations), _zero=False)
                check(lib().ark_hip_fr_scale_device(self.field, other.evaluations.ptr, k.ctypes.data_as(C.c_void_p), out.ptr, len(out)),
                      "ark_hip_fr_scale_device")
                new = DenseMultilinearExtension(other.num_vars, out)
            else:
                if self.num_vars != other.num_vars:
                    raise ValueError("num_vars differ: %d and %d" % (self.num_vars, other.num_vars))
                check(lib().ark_hip_fr_axpy_device(self.field, self.evaluations.ptr, k.ctypes.data_as(C.c_void_p), other.evaluations.ptr,
                                                   self.evaluations.ptr, len(self.evaluations)), "ark_hip_fr_axpy_device")
                return self
        old = self.evaluations
        self.num_vars, self.evaluations = new.num_vars, new.evaluations
        new.evaluations = old
        new.free()
        return self
