"""Extension-field vectors over the one-word fields and the FRI commit phase behind the ark_hip_xfp_* / ark_hip_fri_* entries.

The extension fields are the reference's tower models over SmallFp<P>: Fp2 = Fp[u] / (u^2 - 7) over Goldilocks, Fp4 =
Fp2[v] / (v^2 - u) over Fp2 = Fp[u] / (u^2 - W) for BabyBear (W = 11) and KoalaBear (W = 3).  An element is its d components in
the order CanonicalSerialize writes them, each a stored Montgomery word; here a tuple of d Python integers.  A SmallExtVec is a
SmallDeviceMatrix of d columns, so the base-field transform, add / sub / neg / scale and the Merkle commit of that matrix are the
extension's.  Products run in libark_hip.so; the verifier below adds residues and compares, nothing more."""
import ctypes as C

import numpy as np

from ._lib import FriNextBeta, SmallRadix2DomainStruct, check, lib
from .merkle import DIGEST_BYTES, MerkleTree
from .smallfp import SMALL_FIELDS, SmallDeviceMatrix, SmallRadix2EvaluationDomain, small_field_dtype, small_field_id, small_field_pow

_NAMES = {v[0]: k for k, v in SMALL_FIELDS.items()}


def _elem(x, d=None):
    a = (C.c_uint64 * 4)()
    vals = [int(v) for v in x]
    if d is not None and len(vals) != d:
        raise ValueError("an element of this extension has %d components" % d)
    for k, v in enumerate(vals):
        a[k] = v
    return a


def small_ext_degree(field):
    return 2 if small_field_id(field) == 0 else 4


def small_ext_info(field):
    """ark_hip_xfp_info as a dict: component k is the coefficient of X^exponents[k] in Fp[X] / (X^d - W)."""
    out = (C.c_uint64 * 8)()
    check(lib().ark_hip_xfp_info(small_field_id(field), out), "ark_hip_xfp_info")
    d = int(out[0])
    return dict(degree=d, w=int(out[1]), w_stored=int(out[2]), exponents=[int(out[3 + k]) for k in range(d)])


def ext_mul(field, a, b):
    d, out = small_ext_degree(field), (C.c_uint64 * 4)()
    check(lib().ark_hip_xfp_mul(small_field_id(field), _elem(a, d), _elem(b, d), out), "ark_hip_xfp_mul")
    return tuple(int(out[k]) for k in range(d))


def ext_inverse(field, a):
    d, out = small_ext_degree(field), (C.c_uint64 * 4)()
    check(lib().ark_hip_xfp_inverse(small_field_id(field), _elem(a, d), out), "ark_hip_xfp_inverse")
    return tuple(int(out[k]) for k in range(d))


def ext_pow(field, a, e):
    d, out = small_ext_degree(field), (C.c_uint64 * 4)()
    check(lib().ark_hip_xfp_pow(small_field_id(field), _elem(a, d), e, out), "ark_hip_xfp_pow")
    return tuple(int(out[k]) for k in range(d))


class SmallExtVec:
    """n extension elements on the device: a SmallDeviceMatrix of d columns, component k at element offset k * stride."""

    def __init__(self, field, n, stride=None, matrix=None):
        self.field = small_field_id(field)
        self.degree = small_ext_degree(field)
        self.n = int(n)
        self.matrix = matrix if matrix is not None else SmallDeviceMatrix(field, self.degree, self.n if stride is None else stride)
        if self.matrix.count != self.degree or self.matrix.stride < self.n or self.matrix.field != self.field:
            raise ValueError("d columns of at least n words of the field")

    @property
    def stride(self):
        return self.matrix.stride

    @property
    def ptr(self):
        return self.matrix.vec.ptr

    @property
    def _p(self):
        return self.matrix.vec._p

    @classmethod
    def from_host(cls, field, components, stride=None):
        """components: [d, n] stored words"""
        m = SmallDeviceMatrix.from_host(field, components, stride)
        return cls(field, np.shape(components)[1], matrix=m)

    def to_host(self):
        return self.matrix.to_host(self.n)

    def _like(self, o):
        if o.field != self.field or o.n != self.n:
            raise ValueError("vectors of one field and one length are combined")

    def __imul__(self, o):
        self._like(o)
        check(lib().ark_hip_xfp_vec_mul(self.field, self._p, self.stride, o._p, o.stride, self._p, self.stride, self.n), "ark_hip_xfp_vec_mul")
        return self

    def batch_inverse(self):
        """every non-zero element inverted, zeros left alone"""
        check(lib().ark_hip_xfp_vec_inverse(self.field, self._p, self.stride, self._p, self.stride, self.n), "ark_hip_xfp_vec_inverse")
        return self

    def mul_const(self, k):
        check(lib().ark_hip_xfp_vec_mul_const(self.field, self._p, self.stride, _elem(k, self.degree), self._p, self.stride, self.n),
              "ark_hip_xfp_vec_mul_const")
        return self

    def mul_base(self, vec):
        """by a SmallDeviceVec of n base-field words"""
        if vec.field != self.field or vec.len != self.n:
            raise ValueError("one base-field word per element")
        check(lib().ark_hip_xfp_vec_mul_base(self.field, self._p, self.stride, vec._p, self._p, self.stride, self.n), "ark_hip_xfp_vec_mul_base")
        return self

    def commit(self, wait=True):
        """the tree whose leaf i hashes header | serialize_compressed(element i)"""
        return MerkleTree.commit_small(self.matrix, n=self.n, wait=wait)

    def free(self):
        self.matrix.vec.free()


def combine_columns(matrix, rows, alpha, first_power=0, out=None, accumulate=False):
    """out[i] (+)= alpha^first_power * sum_j alpha^j col_j[i] over the first `rows` words of every column of a SmallDeviceMatrix;
    a new compact SmallExtVec unless `out` is given."""
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the vector to add to")
        out = SmallExtVec(matrix.field, rows)
    if out.field != matrix.field or out.n != rows or rows > matrix.stride:
        raise ValueError("one extension element per row")
    check(lib().ark_hip_xfp_combine_columns(matrix.field, matrix.vec._p, matrix.count, matrix.stride, rows, _elem(alpha, out.degree),
                                            first_power, out._p, out.stride, 1 if accumulate else 0), "ark_hip_xfp_combine_columns")
    return out


def fri_plan(field, log_n, log_arity, num_folds):
    """ark_hip_fri_plan as a dict; host only.  Offsets of layers in words, of trees in bytes."""
    out = (C.c_uint64 * (8 + 5 * (num_folds + 1)))()
    check(lib().ark_hip_fri_plan(small_field_id(field), log_n, log_arity, num_folds, out), "ark_hip_fri_plan")
    layers = [dict(log_size=int(out[8 + 5 * l]), log_arity=int(out[9 + 5 * l]), layer_offset=int(out[10 + 5 * l]),
                   tree_offset=int(out[11 + 5 * l]), lo_bits=int(out[12 + 5 * l])) for l in range(int(out[1]))]
    return dict(degree=int(out[0]), layer_words=int(out[2]), tree_bytes=int(out[3]), launches_per_fold=int(out[4]),
                final_size=int(out[5]), final_copy_offset=int(out[6]), layers=layers)


def fri_folded_domain(dom, log_arity):
    s = SmallRadix2DomainStruct()
    check(lib().ark_hip_fri_folded_domain(dom.field, C.byref(dom._s), log_arity, C.byref(s)), "ark_hip_fri_folded_domain")
    return SmallRadix2EvaluationDomain(dom.field, s)


def fri_fold_row(dom, log_arity, index, row, beta):
    """The fold of one opened row (row[k * 2^a + j] = component k of f[index + j n / 2^a]); host only."""
    d = small_ext_degree(dom.field)
    r = np.ascontiguousarray([int(v) for v in row], dtype=np.uint64)
    if r.size != d << log_arity:
        raise ValueError("a row holds d * 2^log_arity words")
    out = (C.c_uint64 * 4)()
    check(lib().ark_hip_fri_fold_row(dom.field, C.byref(dom._s), log_arity, index, r.ctypes.data_as(C.POINTER(C.c_uint64)), _elem(beta, d), out),
          "ark_hip_fri_fold_row")
    return tuple(int(out[k]) for k in range(d))


def fri_fold(vec, dom, log_arity, beta, out=None):
    """The fold of a SmallExtVec of dom.size() evaluations by beta: a new compact vector of size >> log_arity unless `out` is given."""
    if vec.n != dom.size() or vec.field != dom.field:
        raise ValueError("one evaluation per element of the domain")
    if out is None:
        out = SmallExtVec(vec.field, vec.n >> log_arity)
    check(lib().ark_hip_fri_fold(vec.field, C.byref(dom._s), log_arity, _elem(beta, vec.degree), vec._p, vec.stride, out._p, out.stride),
          "ark_hip_fri_fold")
    return out


class _TreeView(MerkleTree):
    """A tree that lives inside a FriProver's workspace: opened like any other, owned by the prover."""

    def __init__(self, field, n, count, elem_bytes, d_data, d_tree, keep):
        self.small, self.field = True, field
        self.n, self.count, self.stride, self.elem_bytes = int(n), int(count), int(n), int(elem_bytes)
        self.log_n = self.n.bit_length() - 1
        self._data, self._keep, self._tree, self._root = C.c_void_p(d_data), keep, C.c_void_p(d_tree), None

    def free(self):
        self._tree = C.c_void_p()


class FriProver:
    """The commit phase over a compact SmallExtVec of dom.size() evaluations (layer 0, never written), and its queries."""

    def __init__(self, layer0, dom, log_arity, num_folds):
        if layer0.n != dom.size() or layer0.stride != layer0.n or layer0.field != dom.field:
            raise ValueError("layer 0 is compact and holds one evaluation per element of the domain")
        self.field, self.dom, self.log_arity, self.num_folds = dom.field, dom, int(log_arity), int(num_folds)
        self.layer0 = layer0
        self.plan = fri_plan(self.field, dom.log_size_of_group(), log_arity, num_folds)
        self._eb = small_field_dtype(self.field).itemsize
        self._layers, self._trees = C.c_void_p(), C.c_void_p()
        check(lib().ark_hip_malloc(max(self.plan["layer_words"] * self._eb, 16), C.byref(self._layers)), "ark_hip_malloc")
        check(lib().ark_hip_malloc(max(self.plan["tree_bytes"], 16), C.byref(self._trees)), "ark_hip_malloc")
        self.roots, self.betas, self.final_poly, self.trees, self.domains = [], [], None, [], []

    def layer_ptr(self, l):
        return self.layer0.ptr if l == 0 else self._layers.value + self.plan["layers"][l]["layer_offset"] * self._eb

    def layer_to_host(self, l):
        """layer l as [d, size] stored words (a download: tests and tools)"""
        d, size = self.plan["degree"], 1 << self.plan["layers"][l]["log_size"]
        out = np.empty((d, size), dtype=small_field_dtype(self.field))
        check(lib().ark_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.layer_ptr(l)), out.nbytes), "ark_hip_memcpy_d2h")
        return out

    def commit_phase(self, challenge_fn):
        """challenge_fn(root: bytes) -> the d components of the layer's challenge.  Fills roots, betas, final_poly ([d, size] stored
        coefficient words of the last layer) and the per-layer trees."""
        d = self.plan["degree"]
        betas, error = [], []

        def cb(_user, root_p, beta_p):
            try:
                beta = [int(v) for v in challenge_fn(C.string_at(root_p, DIGEST_BYTES))]
                if len(beta) != d:
                    raise ValueError("a challenge has %d components" % d)
                for k in range(d):
                    beta_p[k] = beta[k]
                betas.append(tuple(beta))
                return 0
            except Exception as ex:  # noqa: BLE001 -- carried over the C frames and raised below
                error.append(ex)
                return -100

        roots = np.zeros((self.num_folds, DIGEST_BYTES), dtype=np.uint8)
        final = np.empty((d, self.plan["final_size"]), dtype=small_field_dtype(self.field))
        callback = FriNextBeta(cb)   # alive for as long as the call runs
        rc = lib().ark_hip_fri_commit_phase(self.field, C.byref(self.dom._s), self.log_arity, self.num_folds, self.layer0._p, self._layers,
                                            self._trees, C.cast(callback, C.c_void_p), None,
                                            roots.ctypes.data_as(C.c_void_p), final.ctypes.data_as(C.c_void_p))
        if error:
            raise error[0]
        check(rc, "ark_hip_fri_commit_phase")
        self.roots, self.betas, self.final_poly = [r.tobytes() for r in roots], betas, final
        self.trees, self.domains = [], [self.dom]
        for l in range(self.num_folds):
            lay = self.plan["layers"][l]
            rows = 1 << (lay["log_size"] - lay["log_arity"])
            self.trees.append(_TreeView(self.field, rows, d << lay["log_arity"], self._eb, self.layer_ptr(l),
                                        self._trees.value + lay["tree_offset"], self))
            self.domains.append(fri_folded_domain(self.domains[-1], lay["log_arity"]))
        return self.roots

    def query(self, indices):
        """Per layer l < num_folds: (row indices = index mod rows, rows [q, d * 2^a] words, paths [q, log rows, 32])."""
        out = []
        idx = [int(i) for i in indices]
        for t in self.trees:
            idx = [i % t.n for i in idx]
            rows, paths = t.open(idx)
            out.append((list(idx), rows, paths))
        return out

    def free(self):
        for p in (self._layers, self._trees):
            if p:
                lib().ark_hip_free(p)
        self._layers, self._trees, self.trees = C.c_void_p(), C.c_void_p(), []

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


def fri_verify_query(dom, log_arity, num_folds, roots, betas, final_poly, index, openings):
    """One query of a commit phase, on the host: `openings` = [(row, path)] per layer l < num_folds for row index
    (index mod rows of layer l).  Every row must open against its root, carry the value the previous fold produced, and the last
    fold must equal the final polynomial at its point."""
    field = dom.field
    name = _NAMES[field]
    p = SMALL_FIELDS[name][2]
    d = small_ext_degree(field)
    plan = fri_plan(field, dom.log_size_of_group(), log_arity, num_folds)
    final = np.asarray(final_poly)
    if len(roots) != num_folds or len(betas) != num_folds or len(openings) != num_folds or final.shape != (d, plan["final_size"]):
        return False
    pos, cur, value = int(index) % dom.size(), dom, None
    for l in range(num_folds):
        lay = plan["layers"][l]
        a = lay["log_arity"]
        rows = 1 << (lay["log_size"] - a)
        r, j = pos % rows, pos // rows
        row, path = openings[l]
        row = [int(v) for v in np.asarray(row).reshape(-1)]
        if len(row) != d << a or any(v >= p for v in row):
            return False
        if not MerkleTree.verify(name, roots[l], rows, r, row, path):
            return False
        if value is not None and tuple(row[(k << a) + j] for k in range(d)) != value:
            return False
        value = fri_fold_row(cur, a, r, row, betas[l])
        cur, pos = fri_folded_domain(cur, a), r
    if value is None:
        return True
    # the final polynomial at x = h w^pos, by Horner on every component (x lies in the base field)
    x = ext_mul(field, (cur.coset_offset(),) + (0,) * (d - 1), (small_field_pow(field, cur.group_gen(), pos),) + (0,) * (d - 1))
    acc = (0,) * d
    for i in range(final.shape[1] - 1, -1, -1):
        acc = ext_mul(field, acc, x)
        acc = tuple((acc[k] + int(final[k, i])) % p for k in range(d))
    return acc == value
