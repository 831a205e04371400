"""Merkle commitments over device-resident column batches behind the ark_hip_merkle_* entries: a SHA3-256 tree over the rows of a
matrix of one-word field elements (SmallDeviceMatrix / SmallDeviceVec) or of Fr elements (DeviceVec, DenseMultilinearExtension).

    leaf(i) = SHA3-256( u32_le(count) | u32_le(elem_bytes) | the row's elements as CanonicalSerialize::serialize_compressed writes them )
    node    = SHA3-256( u32_le(0xFFFFFFFF) | u32_le(0) | left | right )

The tree (2n - 1 digests, root first) stays on the device; `open` brings back rows and authentication paths of chosen indices, and
`verify` checks one opening on the host without a GPU.  This module holds no hashing: everything runs in libark_hip.so."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib
from .smallfp import SMALL_FIELDS, small_field_dtype, small_field_id

DIGEST_BYTES = 32


def merkle_plan(n, count, elem_bytes):
    """ark_hip_merkle_plan as a dict; host only."""
    out = (C.c_uint64 * 8)()
    check(lib().ark_hip_merkle_plan(n, count, elem_bytes, out), "ark_hip_merkle_plan")
    keys = ("tree_bytes", "leaf_permutations", "launches", "tail_level", "leaf_blocks", "node_blocks", "levels_per_launch", "permutation")
    return dict(zip(keys, (int(v) for v in out)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def merkle_node(left, right):
    out = np.empty(DIGEST_BYTES, dtype=np.uint8)
    l, r = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (left, right))
    if l.size != DIGEST_BYTES or r.size != DIGEST_BYTES:
        raise ValueError("a digest is 32 bytes")
    check(lib().ark_hip_merkle_node(_ptr(l), _ptr(r), _ptr(out)), "ark_hip_merkle_node")
    return out.tobytes()


def _row(small, field, row):
    if small:
        return np.ascontiguousarray(row, dtype=small_field_dtype(field)).reshape(-1)
    return np.ascontiguousarray(row, dtype=np.uint64).reshape(-1, 4)


def merkle_leaf_small(field, row):
    """The leaf digest of one row of one-word elements (as stored); host only."""
    a = _row(True, field, row)
    out = np.empty(DIGEST_BYTES, dtype=np.uint8)
    check(lib().ark_hip_merkle_leaf_sfp(small_field_id(field), _ptr(a), a.size, _ptr(out)), "ark_hip_merkle_leaf_sfp")
    return out.tobytes()


def merkle_leaf_fr(field, row):
    """The leaf digest of one row of Fr elements ([count, 4] uint64, Montgomery); host only."""
    a = _row(False, field, row)
    out = np.empty(DIGEST_BYTES, dtype=np.uint8)
    check(lib().ark_hip_merkle_leaf_fr(cv.field_id(field), _ptr(a), a.shape[0], _ptr(out)), "ark_hip_merkle_leaf_fr")
    return out.tobytes()


class MerkleTree:
    """A committed matrix: the tree in device memory, and the matrix it was built from (kept alive for `open`)."""

    def __init__(self, small, field, n, count, stride, elem_bytes, d_data, keep):
        self.small, self.field = small, field
        self.n, self.count, self.stride, self.elem_bytes = int(n), int(count), int(stride), int(elem_bytes)
        self.log_n = self.n.bit_length() - 1
        self._data, self._keep = d_data, keep
        self._tree = C.c_void_p()
        check(lib().ark_hip_malloc((2 * self.n - 1) * DIGEST_BYTES, C.byref(self._tree)), "ark_hip_malloc")

    @classmethod
    def commit_small(cls, matrix_or_vec, n=None, wait=True):
        """The tree over the first n = 2^k elements of every column of a SmallDeviceMatrix, or of a SmallDeviceVec (one column);
        n = None: the whole stride / vector."""
        m = matrix_or_vec
        if hasattr(m, "vec"):
            count, stride, vec = m.count, m.stride, m.vec
        else:
            count, stride, vec = 1, m.len, m
        n = stride if n is None else int(n)
        if n < 1 or n > stride or n & (n - 1):
            raise ValueError("a column holds 2^k elements")
        t = cls(True, vec.field, n, count, stride, vec.dtype.itemsize, vec._p, m)
        return t._commit(wait)

    @classmethod
    def commit_fr(cls, field, vecs, wait=True):
        """The tree over one DeviceVec (one column) or over `count` equal-length columns laid out in ONE DeviceVec of
        count * n elements (vecs = (vec, count))."""
        vec, count = vecs if isinstance(vecs, tuple) else (vecs, 1)
        if vec.len == 0 or vec.len % count:
            raise ValueError("count columns of one length")
        n = vec.len // count
        if n & (n - 1):
            raise ValueError("a column holds 2^k elements")
        t = cls(False, cv.field_id(field), n, count, n, 32, vec.ptr, vec)
        return t._commit(wait)

    def _commit(self, wait):
        self._root = None
        root = np.empty(DIGEST_BYTES, dtype=np.uint8) if wait else None
        args = (self.field, self._data, self.count, self.stride, self.n, self._tree, _ptr(root) if wait else None)
        try:
            if self.small:
                check(lib().ark_hip_merkle_commit_sfp_device(*args), "ark_hip_merkle_commit_sfp_device")
            else:
                check(lib().ark_hip_merkle_commit_fr_device(*args), "ark_hip_merkle_commit_fr_device")
        except Exception:
            self.free()
            raise
        if wait:
            self._root = root.tobytes()
        return self

    @property
    def device_ptr(self):
        return self._tree.value

    @property
    def root(self):
        """The 32-byte root; after an asynchronous commit this is a (waiting) 32-byte download."""
        if self._root is None:
            out = np.empty(DIGEST_BYTES, dtype=np.uint8)
            check(lib().ark_hip_memcpy_d2h(_ptr(out), self._tree, DIGEST_BYTES), "ark_hip_memcpy_d2h")
            self._root = out.tobytes()
        return self._root

    def to_host(self):
        """The whole tree, 2n - 1 digests (a download: tests and tools)."""
        out = np.empty((2 * self.n - 1, DIGEST_BYTES), dtype=np.uint8)
        check(lib().ark_hip_memcpy_d2h(_ptr(out), self._tree, out.nbytes), "ark_hip_memcpy_d2h")
        return out

    def open(self, indices, rows=True):
        """(rows, paths) of the given indices: rows [q, count] words ([q, count, 4] for Fr) in memory form, or None with
        rows=False; paths uint8 [q, log n, 32], siblings from the leaf level upwards."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        q = idx.size
        paths = np.empty((q, self.log_n, DIGEST_BYTES), dtype=np.uint8)
        out = None
        if rows:
            out = np.empty((q, self.count), dtype=small_field_dtype(self.field)) if self.small else np.empty((q, self.count, 4), dtype=np.uint64)
        check(lib().ark_hip_merkle_open_device(self._tree, self.n, self._data if rows else None, self.elem_bytes, self.count, self.stride,
                                               _ptr(idx), q, _ptr(out) if rows else None, _ptr(paths)), "ark_hip_merkle_open_device")
        return out, paths

    @staticmethod
    def verify(field, root, n, index, row, path, small=None):
        """One opening against a root, on the host: `field` a one-word field's name (or small=True with its id) or a scalar
        field's name / id."""
        if small is None:
            small = isinstance(field, str) and field in SMALL_FIELDS
        a = _row(small, field, row)
        p = np.ascontiguousarray(path, dtype=np.uint8).reshape(-1)
        r = np.frombuffer(bytes(root), dtype=np.uint8)
        if r.size != DIGEST_BYTES or p.size % DIGEST_BYTES:
            raise ValueError("a digest is 32 bytes")
        if p.size != (int(n).bit_length() - 1) * DIGEST_BYTES:
            return False   # a path of another tree height
        ok = C.c_int(0)
        if small:
            check(lib().ark_hip_merkle_verify_sfp(small_field_id(field), _ptr(r), n, index, _ptr(a), a.size, _ptr(p), C.byref(ok)),
                  "ark_hip_merkle_verify_sfp")
        else:
            check(lib().ark_hip_merkle_verify_fr(cv.field_id(field), _ptr(r), n, index, _ptr(a), a.shape[0], _ptr(p), C.byref(ok)),
                  "ark_hip_merkle_verify_fr")
        return bool(ok.value)

    def free(self):
        if self._tree:
            lib().ark_hip_free(self._tree)
            self._tree = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
