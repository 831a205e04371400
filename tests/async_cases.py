"""The case table of the asynchrony contract: every `*_device` entry of include/ark_hip.h behind a busy
context stream.  Pure host code -- numpy, ctypes and the existing models; nothing here touches a GPU, so that
tests/test_async_contract_host.py can read it where there is none.  tests/async_contract_child.py runs the cases.

A case names an entry and builds, per variant, what one call of it needs:
  variant 0     the call under test;
  variant "B"   the same call with OTHER VALID host arguments of the same shapes -- what part B writes over the host memory
                right after the call returned (canonical elements, in-range indices, pointers to other live device vectors,
                the fields of another valid domain: a library that read late computes a wrong vector, it never faults);
  variant "C"   the second call of part C (other constants, or the other direction), made with nothing in between.
What a variant builds (`Built`):
  dev      name -> numpy array: the device buffers, uploaded as they are (inputs, and the outputs with their STALE content);
  outs     the names in `dev` the call writes: out of place they start as valid scalars S0 that are not the result, in place
           they start as the input -- either way what a consumer that ran ahead would read;
  host     name -> numpy array: the arguments that are HOST memory (elements, term descriptors, the domain struct as words);
  ptrs     name -> [names in dev]: host arrays of device pointers (d_tables, d_columns, d_data);
  call     (L, a) -> rc, a: name -> address (device buffers, host arguments, "wait": the host result or None, "handle");
  ref      () -> {out name: numpy array}: what each output holds afterwards, from the existing models (a prefix of the
           buffer: what the call does not write stays as it was);
  consume  (out name, element offset, elements): the Fr vector part A hands to the MSM on the second lane;
  wait     (bytes, () -> expected bytes) of the HOST result of the waiting form (part D), None where there is none.
The references are the models the other tests use: oracle_lib for the field operations, the transforms and the MSM, and the
big-integer models pyref, mle_ref, mle_open_ref, prefix_scan_ref, grand_product_ref, fraction_sum_ref, lookup_ref, csr_ref,
gate_ref, sumcheck_ref, merkle_ref and poly_ops_ref.  No arithmetic is written here."""
import ctypes as C
import re

import numpy as np

import csr_ref
import fraction_sum_ref
import gate_ref
import grand_product_ref
import lookup_ref
import merkle_ref
import mle_open_ref
import mle_ref
import oracle_lib as O
import poly_ops_ref as PO
import prefix_scan_ref as PS
import pyref
import sumcheck_ref as S
import algebra_amd as A
from algebra_amd._lib import Radix2DomainStruct

FR = "BLS12_381_FR"
FIELDS = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
CURVE_OF = {"BN254_FR": "BN254_G1", "BLS12_381_FR": "BLS12_381_G1", "BLS12_377_FR": "BLS12_377_G1"}
LOG_N = 12
N = 1 << LOG_N          # vectors; tables have LOG_N variables (two launches of the fold and the eq plans)
N_ODD = 3001            # where an entry takes any n
STALE_SEED = 0x57A1E
vp = C.c_void_p


def g(fname, seed, n):
    """n valid Montgomery elements"""
    return O.gen_scalars(O.FID[fname], seed, n, montgomery=True).reshape(n, 4)


def stale(fname, n):
    return g(fname, STALE_SEED, n)


def dec(a, fname):
    return S.decode(a, pyref.MODULI[fname][0])


def enc(xs, fname):
    return S.encode(xs, pyref.MODULI[fname][0])


def fop(fname, op, a, b=None):
    return O.field_op(O.FID[fname], op, a, b).reshape(-1, 4)


def tile(k, n):
    return np.ascontiguousarray(np.tile(np.asarray(k, dtype=np.uint64).reshape(1, 4), (n, 1)))


def dom_words(fname, n, offset=None):
    """the ark_hip_radix2_domain of size n (a coset with `offset`) as its 30 64-bit words: host arithmetic of the library"""
    d = A.Radix2EvaluationDomain.new(fname, n)
    if offset is not None:
        d = d.get_coset(offset)
    assert d is not None and C.sizeof(Radix2DomainStruct) == 240
    return np.frombuffer(bytes(d._s), dtype=np.uint64).copy()


def dom_ptr(addr):
    return C.cast(vp(addr), C.POINTER(Radix2DomainStruct))


def pp(addr):
    return C.cast(vp(addr), C.POINTER(C.c_void_p))


def up(addr):
    return C.cast(vp(addr), C.POINTER(C.c_uint))


def ip64(addr):
    return C.cast(vp(addr), C.POINTER(C.c_int64))


class Built:
    def __init__(self, dev, outs, call, ref, host=None, ptrs=None, consume=None, wait=None, handle=None, compare=None):
        self.dev, self.outs, self.call, self._ref = dev, list(outs), call, ref
        self.host, self.ptrs = dict(host or {}), dict(ptrs or {})
        self.consume, self.wait, self.handle, self.compare = consume, wait, handle, compare
        self._cache = None

    def ref(self):
        if self._cache is None:
            self._cache = {k: np.ascontiguousarray(v) for k, v in self._ref().items()}
        return self._cache

    def expected(self, name):
        """the bytes of the whole output buffer afterwards: the reference's prefix, the rest as it was"""
        want = np.ascontiguousarray(self.dev[name]).reshape(-1).view(np.uint8).copy()
        r = self.ref()[name].reshape(-1).view(np.uint8)
        assert r.size <= want.size, (name, r.size, want.size)
        want[:r.size] = r
        return want


class Case:
    def __init__(self, name, entry, group, parts, build, fname=FR):
        self.name, self.entry, self.group, self.parts, self.build, self.fname = name, entry, group, tuple(parts), build, fname
        self._built = {}

    def make(self, variant=0):
        if variant not in self._built:
            self._built[variant] = self.build(variant)
        return self._built[variant]


CASES = []


def case(name, entry, group, parts, fname=FR):
    def deco(build):
        assert entry.startswith("ark_hip_") and all(c.name != name for c in CASES), name
        CASES.append(Case(name, entry, group, parts, build, fname))
        return build
    return deco


# ---- pointwise and copies ---------------------------------------------------------------------------------------------------
def _pointwise(fname, n):
    fid = O.FID[fname]
    tag = "%s:%d" % (fname, n)
    a, b = g(fname, 1, n), g(fname, 2, n)

    def two(entry, op):
        @case("%s %s" % (op, tag), entry, "pointwise", "A", fname)
        def _(v):
            return Built({"a": a, "b": b, "out": stale(fname, n)}, ["out"],
                         lambda L, x: getattr(L, entry)(fid, vp(x["a"]), vp(x["b"]), vp(x["out"]), n),
                         lambda: {"out": fop(fname, "mul", a, fop(fname, "inv", b)) if op == "div" else fop(fname, op, a, b)},
                         consume=("out", 0, n))
    for op in ("add", "sub", "mul", "div"):
        two("ark_hip_fr_%s_device" % op, op)

    def one(entry, op):
        @case("%s %s" % (op, tag), entry, "pointwise", "A", fname)
        def _(v):
            return Built({"a": a, "out": stale(fname, n)}, ["out"],
                         lambda L, x: getattr(L, entry)(fid, vp(x["a"]), vp(x["out"]), n),
                         lambda: {"out": fop(fname, op, a)}, consume=("out", 0, n))
    one("ark_hip_fr_neg_device", "neg")
    one("ark_hip_fr_inverse_device", "inv")

    @case("scale %s" % tag, "ark_hip_fr_scale_device", "pointwise", "ABC" if fname == FR else "AB", fname)
    def _(v):
        k = g(fname, 3 if v == 0 else 4, 1)
        return Built({"a": a, "out": stale(fname, n)}, ["out"],
                     lambda L, x: L.ark_hip_fr_scale_device(fid, vp(x["a"]), vp(x["k"]), vp(x["out"]), n),
                     lambda: {"out": fop(fname, "mul", a, tile(k, n))}, host={"k": k}, consume=("out", 0, n))

    @case("axpy %s" % tag, "ark_hip_fr_axpy_device", "pointwise", "AB", fname)
    def _(v):
        k = g(fname, 5 if v == 0 else 6, 1)
        return Built({"a": a, "b": b, "out": stale(fname, n)}, ["out"],
                     lambda L, x: L.ark_hip_fr_axpy_device(fid, vp(x["a"]), vp(x["k"]), vp(x["b"]), vp(x["out"]), n),
                     lambda: {"out": fop(fname, "add", a, fop(fname, "mul", tile(k, n), b))}, host={"k": k}, consume=("out", 0, n))

    @case("lincomb %s" % tag, "ark_hip_fr_lincomb_device", "pointwise", "ABC" if fname == FR else "AB", fname)
    def _(v):
        dev = {"t%d" % i: g(fname, 10 + i, n) for i in range(3)}
        dev.update({"u%d" % i: g(fname, 20 + i, n) for i in range(3)})
        dev["out"] = stale(fname, n)
        names = ["t0", "t1", "t2"] if v != "B" else ["u2", "u0", "u1"]      # part C keeps the tables and changes the constants
        coeffs, c0 = g(fname, 30 if v == 0 else 31, 3), g(fname, 32 if v == 0 else 33, 1)
        p = pyref.MODULI[fname][0]
        return Built(dev, ["out"],
                     lambda L, x: L.ark_hip_fr_lincomb_device(fid, pp(x["d_tables"]), 3, vp(x["coeffs"]), vp(x["c0"]), vp(x["out"]), n),
                     lambda: {"out": enc(grand_product_ref.lincomb([dec(dev[t], fname) for t in names], dec(coeffs, fname),
                                                                   dec(c0, fname)[0], p), fname)},
                     host={"coeffs": coeffs, "c0": c0}, ptrs={"d_tables": names}, consume=("out", 0, n))

    @case("sum_of_products %s" % tag, "ark_hip_fr_sum_of_products_device", "pointwise", "AB", fname)
    def _(v):
        f = PS.Field(fname)
        dev = {"c%d" % i: g(fname, 40 + i, n) for i in range(3)}
        dev.update({"e%d" % i: g(fname, 50 + i, n) for i in range(3)})
        dev["out"] = stale(fname, n)
        if v == 0:
            names, lens, cols, rots = ["c0", "c1", "c2"], [2, 1, 3], [0, 1, 2, 0, 1, 2], [0, 1, -1, 5, 0, -7]
            coeffs, c0 = g(fname, 60, 3), g(fname, 61, 1)
        else:   # other in-range lengths (the same total), columns, rotations, constants and pointers
            names, lens, cols, rots = ["e1", "e2", "e0"], [3, 2, 1], [2, 2, 1, 0, 0, 1], [3, 0, -2, 1, 9, -1]
            coeffs, c0 = g(fname, 62, 3), g(fname, 63, 1)
        terms, at = [], 0
        for j, ln in enumerate(lens):
            terms.append((PS.ints(coeffs[j:j + 1])[0], [(cols[at + q], rots[at + q]) for q in range(ln)]))
            at += ln
        host = {"term_len": np.array(lens, dtype=np.uint32), "term_columns": np.array(cols, dtype=np.uint32),
                "term_rotations": np.array(rots, dtype=np.int64), "coeffs": coeffs, "c0": c0}
        return Built(dev, ["out"],
                     lambda L, x: L.ark_hip_fr_sum_of_products_device(fid, pp(x["d_columns"]), 3, n, up(x["term_len"]),
                                                                      up(x["term_columns"]), ip64(x["term_rotations"]),
                                                                      vp(x["coeffs"]), 3, vp(x["c0"]), vp(x["out"])),
                     lambda: {"out": PS.limbs(gate_ref.sum_of_products(f, [PS.ints(dev[c]) for c in names], n, terms,
                                                                       PS.ints(c0)[0]))},
                     host=host, ptrs={"d_columns": names}, consume=("out", 0, n))


for _f in FIELDS:
    for _n in (N, N_ODD):
        _pointwise(_f, _n)


def _copies(n):
    fid = O.FID[FR]
    src = g(FR, 70, n)

    @case("memcpy_d2d %d" % n, "ark_hip_memcpy_d2d", "pointwise", "A")
    def _(v):
        return Built({"src": src, "out": stale(FR, n)}, ["out"], lambda L, x: L.ark_hip_memcpy_d2d(vp(x["out"]), vp(x["src"]), n * 32),
                     lambda: {"out": src}, consume=("out", 0, n))

    @case("memset_device zero %d" % n, "ark_hip_memset_device", "pointwise", "A")
    def _(v):
        return Built({"out": stale(FR, n)}, ["out"], lambda L, x: L.ark_hip_memset_device(vp(x["out"]), 0, n * 32),
                     lambda: {"out": np.zeros((n, 4), dtype=np.uint64)}, consume=("out", 0, n))

    @case("count_indices %d" % n, "ark_hip_fr_count_indices_device", "pointwise", "A")
    def _(v):
        table_len = 1000
        idx = np.random.default_rng(71).integers(0, table_len + 20, size=n).astype(np.uint32)   # some are skipped
        return Built({"idx": idx, "out": stale(FR, table_len)}, ["out"],
                     lambda L, x: L.ark_hip_fr_count_indices_device(fid, vp(x["idx"]), n, vp(x["out"]), table_len),
                     lambda: {"out": enc(fraction_sum_ref.counts([int(i) for i in idx], table_len), FR)},
                     consume=("out", 0, table_len))

    @case("lookup %d" % n, "ark_hip_fr_lookup_device", "pointwise", "AD")
    def _(v):
        table_len = 1000
        ta = g(FR, 72, table_len)
        rng = np.random.default_rng(73)
        va = ta[rng.integers(0, table_len, size=n)].copy()
        miss = np.nonzero(rng.random(n) < 0.1)[0]
        va[miss] = g(FR, 74, 16)[rng.integers(0, 16, size=miss.size)]
        model = lambda: lookup_ref.lookup(mle_ref.ints(ta), mle_ref.ints(va))     # noqa: E731
        return Built({"table": ta, "values": va, "out": stale(FR, table_len)}, ["out"],
                     lambda L, x: L.ark_hip_fr_lookup_device(fid, vp(x["table"]), table_len, vp(x["values"]), n, None, vp(x["out"]),
                                                             C.cast(vp(x["wait"]), C.POINTER(C.c_uint64)) if x["wait"] else None),
                     lambda: {"out": enc(model()[1], FR)}, consume=("out", 0, table_len),
                     wait=(8, lambda: int(model()[2]).to_bytes(8, "little")))


for _n in (N, N_ODD):
    _copies(_n)


# ---- sparse matrices ------------------------------------------------------------------------------------------------------
def _csr(rows, cols, transpose):
    fid = O.FID[FR]
    f = PS.Field(FR)
    rng = np.random.default_rng(80)
    per_row = rng.integers(0, 7, size=rows)
    per_row[5] = 300                                      # one long row
    row_ptr = np.concatenate([[0], np.cumsum(per_row)]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    col_idx = rng.integers(0, cols, size=nnz).astype(np.uint32)
    vals = g(FR, 81, nnz)
    x_len, y_len = (rows, cols) if transpose else (cols, rows)
    xv = g(FR, 82, x_len)

    @case("csr_mul%s %dx%d" % (" transposed" if transpose else "", rows, cols), "ark_hip_fr_csr_mul_device", "pointwise", "A")
    def _(v):
        def handle(L):
            h = vp(0)
            rc = L.ark_hip_fr_csr_create(fid, rows, cols, vp(row_ptr.ctypes.data), vp(col_idx.ctypes.data), vp(vals.ctypes.data), nnz, 1,
                                         C.byref(h))
            assert rc == 0, rc
            return h, lambda: L.ark_hip_fr_csr_free(h)

        def ref():
            if transpose:
                tp, ti, tv = csr_ref.transpose(rows, cols, row_ptr, col_idx, PS.ints(vals))
                return {"out": PS.limbs(csr_ref.mul(f, cols, tp, ti, tv, PS.ints(xv)))}
            return {"out": PS.limbs(csr_ref.mul(f, rows, row_ptr, col_idx, PS.ints(vals), PS.ints(xv)))}
        return Built({"x": xv, "out": stale(FR, y_len)}, ["out"],
                     lambda L, x: L.ark_hip_fr_csr_mul_device(x["handle"], int(transpose), vp(x["x"]), x_len, vp(x["out"]), y_len),
                     ref, consume=("out", 0, y_len), handle=handle)


for _t in (False, True):
    _csr(N, N_ODD, _t)
    _csr(N_ODD, N, _t)


# ---- transforms -------------------------------------------------------------------------------------------------------------
OFFSET = g(FR, 90, 1)[0]                                     # the coset offset, and its square for the other constants
OFFSET2 = fop(FR, "sqr", OFFSET)[0]


def _dom_variant(v, offset):
    """variant 0: the case's own domain; the others: a coset with another offset (a valid domain of the same size)"""
    if v == 0:
        return offset
    return OFFSET2 if offset is not None and np.array_equal(offset, OFFSET) else OFFSET


def _transform(name, entry, inverse, offset, parts="AB"):
    fid = O.FID[FR]
    xs = g(FR, 91, N)

    @case(name, entry, "transforms", parts)
    def _(v):
        off = _dom_variant(v, offset)
        return Built({"out": xs}, ["out"], lambda L, x: getattr(L, entry)(fid, dom_ptr(x["dom"]), vp(x["out"])),
                     lambda: {"out": O.fft(fid, xs, LOG_N, off, inverse, 4).reshape(N, 4)},
                     host={"dom": dom_words(FR, N, off)}, consume=("out", 0, N))


_transform("fft", "ark_hip_fft_in_place_device", False, None)
_transform("ifft", "ark_hip_ifft_in_place_device", True, None)
_transform("fft coset", "ark_hip_fft_in_place_device", False, OFFSET, "ABC")       # part C: offset g then g^2, both warmed
_transform("ifft coset", "ark_hip_ifft_in_place_device", True, OFFSET, "ABC")


def _degree_aware(num_coeffs):
    fid = O.FID[FR]
    xs = g(FR, 92, N)                                      # whatever lies past num_coeffs is not read: it counts as zero

    @case("fft degree-aware %d" % num_coeffs, "ark_hip_fft_in_place_degree_aware_device", "transforms", "AB")
    def _(v):
        off = _dom_variant(v, None)
        padded = xs.copy()
        padded[num_coeffs:] = 0
        return Built({"out": xs}, ["out"],
                     lambda L, x: L.ark_hip_fft_in_place_degree_aware_device(fid, dom_ptr(x["dom"]), vp(x["out"]), num_coeffs),
                     lambda: {"out": O.fft(fid, padded, LOG_N, off, False, 4).reshape(N, 4)},
                     host={"dom": dom_words(FR, N, off)}, consume=("out", 0, N))


_degree_aware(1000)        # at most a quarter of the domain: stages are skipped
_degree_aware(N_ODD)       # more: the plain transform of the zero-extended vector


def _batch(inverse):
    fid = O.FID[FR]
    vecs = {"v%d" % i: g(FR, 93 + i, N) for i in range(3)}

    @case("fft batch%s" % (" inverse" if inverse else ""), "ark_hip_fft_batch_in_place_device", "transforms", "AB")
    def _(v):
        off = _dom_variant(v, None)
        return Built(dict(vecs), list(vecs),
                     lambda L, x: L.ark_hip_fft_batch_in_place_device(fid, dom_ptr(x["dom"]), pp(x["d_data"]), 3, int(inverse)),
                     lambda: {k: O.fft(fid, a, LOG_N, off, inverse, 4).reshape(N, 4) for k, a in vecs.items()},
                     host={"dom": dom_words(FR, N, off)}, ptrs={"d_data": list(vecs)},
                     consume=("v2", 0, N))              # the batch runs on side streams: the last vector


_batch(False)
_batch(True)


def axis_reference(fname, data, G, cols, inverse):
    """out[j][c] = sum_i root^(i j) in[i][c] for root the generator of the size-G domain (inverse: its inverse): the oracle's
    size-G transform of every column; with root^-1 the sums are the forward ones at index (G - j) mod G"""
    fid = O.FID[fname]
    a = np.ascontiguousarray(data).reshape(G, cols, 4)
    out = np.empty_like(a)
    log_g = G.bit_length() - 1
    for c in range(cols):
        y = O.fft(fid, np.ascontiguousarray(a[:, c, :]), log_g, None, False, 1).reshape(G, 4)
        out[:, c, :] = y[[(G - j) % G for j in range(G)]] if inverse else y
    return out.reshape(G * cols, 4)


def _axis(G, cols, parts):
    fid = O.FID[FR]
    data = g(FR, 96, G * cols)

    @case("fft_axis G=%d cols=%d" % (G, cols), "ark_hip_fft_axis_device", "transforms", parts)
    def _(v):
        inverse = v != 0                                   # the other root: the inverse one
        gen, gen_inv, _ = O.domain(fid, G.bit_length() - 1)
        return Built({"out": data}, ["out"],
                     lambda L, x: L.ark_hip_fft_axis_device(fid, vp(x["out"]), G, cols, vp(x["root"])),
                     lambda: {"out": axis_reference(FR, data, G, cols, inverse)},
                     host={"root": (gen_inv if inverse else gen).copy()}, consume=("out", 0, min(G * cols, N)))


_axis(4, N // 4, "AB")
_axis(16, N_ODD, "AB")
for _G in (2, 4, 8, 16):
    for _cols in (300, 4097):
        _axis(_G, _cols, "C")

WORLD = 4


def _shards():
    fid = O.FID[FR]
    m, sub = N // WORLD, N // WORLD // WORLD
    rank = 1
    xs = g(FR, 97, m)

    @case("fft_shard_local world 4 rank 1", "ark_hip_fft_shard_local_device", "transforms", "AB")
    def _(v):
        off = _dom_variant(v, None)

        def ref():
            # the rank's shard alone in the cyclic layout, x[rank + G i2], zeros elsewhere: the first m outputs of the whole
            # transform are then w_n^(rank j2) times the size-m transform of the shard -- the local half, twiddle included
            z = np.zeros((N, 4), dtype=np.uint64)
            z[rank::WORLD] = xs
            return {"out": O.fft(fid, z, LOG_N, off, False, 4).reshape(N, 4)[:m]}
        return Built({"out": xs}, ["out"],
                     lambda L, x: L.ark_hip_fft_shard_local_device(fid, dom_ptr(x["dom"]), rank, WORLD, vp(x["out"]), 0),
                     ref, host={"dom": dom_words(FR, N, off)}, consume=("out", 0, m))

    data = g(FR, 98, m)

    @case("fft_shard_cross world 4", "ark_hip_fft_shard_cross_device", "transforms", "AC")
    def _(v):
        inverse = v == "C"                                 # part C: forward then inverse
        return Built({"src": data, "out": stale(FR, m)}, ["out"],
                     lambda L, x: L.ark_hip_fft_shard_cross_device(fid, dom_ptr(x["dom"]), WORLD, vp(x["src"]), vp(x["out"]), int(inverse)),
                     lambda: {"out": axis_reference(FR, data, WORLD, sub, inverse)},
                     host={"dom": dom_words(FR, N, None)}, consume=("out", 0, m))

    @case("fft_shard_cross world 4, the domain rewritten", "ark_hip_fft_shard_cross_device", "transforms", "B")
    def _(v):
        # the G-point transform takes the size and the root from the domain and nothing of a coset: the other valid value is
        # the domain of a quarter of the size (a late read transforms and writes a quarter of the columns, inside the buffers)
        cols = sub if v == 0 else sub // 4
        return Built({"src": data, "out": stale(FR, m)}, ["out"],
                     lambda L, x: L.ark_hip_fft_shard_cross_device(fid, dom_ptr(x["dom"]), WORLD, vp(x["src"]), vp(x["out"]), 0),
                     lambda: {"out": axis_reference(FR, data[:WORLD * cols], WORLD, cols, False)},
                     host={"dom": dom_words(FR, N if v == 0 else N // 4, None)})

    full = g(FR, 99, N)

    @case("fft_sharded without a communicator", "ark_hip_fft_sharded_device", "transforms", "AB")
    def _(v):
        off = _dom_variant(v, None)
        return Built({"out": full}, ["out"], lambda L, x: L.ark_hip_fft_sharded_device(fid, dom_ptr(x["dom"]), vp(x["out"]), 0),
                     lambda: {"out": O.fft(fid, full, LOG_N, off, False, 4).reshape(N, 4)},
                     host={"dom": dom_words(FR, N, off)}, consume=("out", 0, N))


_shards()


# ---- polynomial operations ----------------------------------------------------------------------------------------------------
def _poly(n):
    fid = O.FID[FR]
    f = PS.Field(FR)
    p = f.p
    coeffs = g(FR, 100, n)

    @case("poly_evaluate %d" % n, "ark_hip_poly_evaluate_device", "poly", "D")
    def _(v):
        z = g(FR, 101, 1)
        return Built({"coeffs": coeffs}, [], lambda L, x: L.ark_hip_poly_evaluate_device(fid, vp(x["coeffs"]), n, vp(x["z"]), vp(x["wait"])),
                     lambda: {}, host={"z": z},
                     wait=(32, lambda: PS.limbs([PO.synthetic_division(PS.ints(coeffs), dec(z, FR)[0], p)[1]]).tobytes()))

    @case("poly_divide_linear %d" % n, "ark_hip_poly_divide_linear_device", "poly", "ABD")
    def _(v):
        z = g(FR, 102 if v == 0 else 103, 1)
        model = lambda: PO.synthetic_division(PS.ints(coeffs), dec(z, FR)[0], p)      # noqa: E731
        return Built({"coeffs": coeffs, "out": stale(FR, n)}, ["out"],
                     lambda L, x: L.ark_hip_poly_divide_linear_device(fid, vp(x["coeffs"]), n, vp(x["z"]), vp(x["out"]), vp(x["wait"])),
                     lambda: {"out": PS.limbs(model()[0])}, host={"z": z}, consume=("out", 0, n - 1),
                     wait=(32, lambda: PS.limbs([model()[1]]).tobytes()))

    m = 1024

    def vanishing(which):
        @case("poly_divide_by_vanishing %d, the %s" % (n, which), "ark_hip_poly_divide_by_vanishing_device", "poly", "A")
        def _(v):
            return Built({"coeffs": coeffs, "quot": stale(FR, n - m), "rem": stale(FR, m)}, ["quot", "rem"],
                         lambda L, x: L.ark_hip_poly_divide_by_vanishing_device(fid, m, vp(x["coeffs"]), n, vp(x["quot"]), vp(x["rem"])),
                         lambda: dict(zip(("quot", "rem"), PO.vanishing_reference(fid, coeffs, m))),
                         consume=("quot", 0, n - m) if which == "quotient" else ("rem", 0, m))
    vanishing("quotient")
    vanishing("remainder")

    a, b = g(FR, 104, n), g(FR, 105, n)

    @case("inner_product %d" % n, "ark_hip_fr_inner_product_device", "poly", "D")
    def _(v):
        return Built({"a": a, "b": b}, [], lambda L, x: L.ark_hip_fr_inner_product_device(fid, vp(x["a"]), vp(x["b"]), n, vp(x["wait"])),
                     lambda: {}, wait=(32, lambda: PS.limbs([csr_ref.inner(f, PS.ints(a), PS.ints(b))]).tobytes()))

    def scan(op, exclusive):
        entry = "ark_hip_fr_prefix_%s_device" % op
        model = {"product": PS.prefix_product, "sum": PS.prefix_sum}[op]

        @case("prefix_%s %d%s" % (op, n, " exclusive" if exclusive else ""), entry, "poly", "AD")
        def _(v):
            res = lambda: model(f, PS.ints(a), exclusive)      # noqa: E731
            return Built({"a": a, "out": stale(FR, n)}, ["out"],
                         lambda L, x: getattr(L, entry)(fid, vp(x["a"]), n, int(exclusive), vp(x["out"]), vp(x["wait"])),
                         lambda: {"out": PS.limbs(res()[0])}, consume=("out", 0, n), wait=(32, lambda: PS.limbs([res()[1]]).tobytes()))
    for _op in ("product", "sum"):
        scan(_op, False)
        scan(_op, True)

    @case("prefix_ratio %d" % n, "ark_hip_fr_prefix_ratio_device", "poly", "AD")
    def _(v):
        res = lambda: PS.prefix_ratio(f, PS.ints(a), PS.ints(b))      # noqa: E731
        return Built({"a": a, "b": b, "out": stale(FR, n)}, ["out"],
                     lambda L, x: L.ark_hip_fr_prefix_ratio_device(fid, vp(x["a"]), vp(x["b"]), n, vp(x["out"]), vp(x["wait"])),
                     lambda: {"out": PS.limbs(res()[0])}, consume=("out", 0, n), wait=(32, lambda: PS.limbs([res()[1]]).tobytes()))


_poly(N)
_poly(N_ODD)


def _lagrange(offset):
    fid = O.FID[FR]
    p = pyref.MODULI[FR][0]

    @case("lagrange_coefficients%s" % (" coset" if offset is not None else ""), "ark_hip_domain_lagrange_coefficients_device", "poly", "AB")
    def _(v):
        off = _dom_variant(v, offset)
        tau = g(FR, 110 if v == 0 else 111, 1)
        h = 1 if off is None else dec(off.reshape(1, 4), FR)[0]
        return Built({"out": stale(FR, N)}, ["out"],
                     lambda L, x: L.ark_hip_domain_lagrange_coefficients_device(fid, dom_ptr(x["dom"]), vp(x["tau"]), vp(x["out"])),
                     lambda: {"out": PO.mont_list(PO.lagrange_reference(FR, LOG_N, h, dec(tau, FR)[0]), p)},
                     host={"dom": dom_words(FR, N, off), "tau": tau}, consume=("out", 0, N))


_lagrange(None)
_lagrange(OFFSET)


# ---- multilinear extensions ---------------------------------------------------------------------------------------------------
NV = LOG_N


def _mle():
    fid = O.FID[FR]
    p = pyref.MODULI[FR][0]
    table = g(FR, 120, N)

    def fix(dim):
        @case("mle_fix_variables dim=%d" % dim, "ark_hip_mle_fix_variables_device", "mle", "AB" if dim else "A")
        def _(v):
            pt = g(FR, 121 if v == 0 else 122, max(dim, 1))[:dim]
            host = {"partial_point": pt} if dim else {}
            return Built({"table": table, "out": stale(FR, N >> dim)}, ["out"],
                         lambda L, x: L.ark_hip_mle_fix_variables_device(fid, vp(x["table"]), NV, vp(x.get("partial_point", 0) or None), dim,
                                                                         vp(x["out"])),
                         lambda: {"out": mle_ref.limbs(mle_ref.fix_variables(mle_ref.ints(table), dec(pt, FR), p))},
                         host=host, consume=("out", 0, N >> dim))
    for _d in (0, 3, NV - 1):
        fix(_d)

    @case("mle_evaluate", "ark_hip_mle_evaluate_device", "mle", "D")
    def _(v):
        pt = g(FR, 123, NV)
        return Built({"table": table}, [], lambda L, x: L.ark_hip_mle_evaluate_device(fid, vp(x["table"]), NV, vp(x["point"]), vp(x["wait"])),
                     lambda: {}, host={"point": pt},
                     wait=(32, lambda: mle_ref.limbs([mle_ref.evaluate(mle_ref.ints(table), dec(pt, FR), p)]).tobytes()))

    def relabel(a, b, k, in_place):
        @case("mle_relabel %s %s" % ("identity" if a == b else "swap", "in place" if in_place else "out of place"),
              "ark_hip_mle_relabel_device", "mle", "A")
        def _(v):
            want = lambda: {"out": mle_ref.limbs(mle_ref.relabel(mle_ref.ints(table), a, b, k))}      # noqa: E731
            if in_place:
                return Built({"out": table}, ["out"], lambda L, x: L.ark_hip_mle_relabel_device(fid, vp(x["out"]), NV, a, b, k, vp(x["out"])),
                             want, consume=("out", 0, N))
            return Built({"table": table, "out": stale(FR, N)}, ["out"],
                         lambda L, x: L.ark_hip_mle_relabel_device(fid, vp(x["table"]), NV, a, b, k, vp(x["out"])), want,
                         consume=("out", 0, N))
    relabel(2, 2, 3, False)
    relabel(1, 7, 4, False)
    relabel(1, 7, 4, True)

    def eq(scaled):
        @case("mle_eq_table%s" % (" scaled" if scaled else ""), "ark_hip_mle_eq_table_device", "mle", "ABC")
        def _(v):
            pt = g(FR, 124 if v == 0 else 125, NV)
            sc = g(FR, 126 if v == 0 else 127, 1)
            host = {"point": pt, "scale": sc} if scaled else {"point": pt}
            return Built({"out": stale(FR, N)}, ["out"],
                         lambda L, x: L.ark_hip_mle_eq_table_device(fid, vp(x["point"]), NV, vp(x["scale"]) if scaled else None, vp(x["out"])),
                         lambda: {"out": mle_ref.limbs(mle_open_ref.eq_table_mont(dec(pt, FR), dec(sc, FR)[0] if scaled else 1, p,
                                                                                  pyref.R_of(p)))},
                         host=host, consume=("out", 0, N))
    eq(False)
    eq(True)

    def quotients(seg):
        @case("mle_quotients, segment %d" % seg, "ark_hip_mle_quotients_device", "mle", "ABD" if seg == 0 else "A")
        def _(v):
            pt = g(FR, 128 if v == 0 else 129, NV)
            model = lambda: mle_open_ref.quotients(mle_ref.ints(table), dec(pt, FR), p)      # noqa: E731
            return Built({"table": table, "out": stale(FR, N - 1)}, ["out"],
                         lambda L, x: L.ark_hip_mle_quotients_device(fid, vp(x["table"]), NV, vp(x["point"]), vp(x["out"]), vp(x["wait"])),
                         lambda: {"out": mle_ref.limbs([q for qs in model()[1] for q in qs])}, host={"point": pt},
                         consume=("out", mle_open_ref.segment_offset(NV, seg), mle_open_ref.segment_len(NV, seg)),
                         wait=(32, lambda: mle_ref.limbs([model()[0]]).tobytes()))
    quotients(0)
    quotients(NV - 1)

    @case("mle_product_tree", "ark_hip_mle_product_tree_device", "mle", "AD")
    def _(v):
        model = lambda: grand_product_ref.tree(dec(table, FR), p)      # noqa: E731
        return Built({"table": table, "out": stale(FR, N - 1)}, ["out"],
                     lambda L, x: L.ark_hip_mle_product_tree_device(fid, vp(x["table"]), NV, vp(x["out"]), vp(x["wait"])),
                     lambda: {"out": enc(model()[1], FR)},
                     consume=("out", grand_product_ref.level_offset(NV, 1), grand_product_ref.level_len(NV, 1)),
                     wait=(32, lambda: enc([model()[0]], FR).tobytes()))

    den = g(FR, 130, N)

    def fraction(has_num, which):
        @case("mle_fraction_tree%s, the %s tree" % ("" if has_num else " without numerators", which),
              "ark_hip_mle_fraction_tree_device", "mle", "AD" if which == "numerator" else "A")
        def _(v):
            model = lambda: fraction_sum_ref.tree(dec(table, FR) if has_num else None, dec(den, FR), p)      # noqa: E731
            dev = {"den": den, "ntree": stale(FR, N - 1), "dtree": g(FR, STALE_SEED + 1, N - 1)}
            if has_num:
                dev["num"] = table
            return Built(dev, ["ntree", "dtree"],
                         lambda L, x: L.ark_hip_mle_fraction_tree_device(fid, vp(x["num"]) if has_num else None, vp(x["den"]), NV,
                                                                         vp(x["ntree"]), vp(x["dtree"]), vp(x["wait"])),
                         lambda: {"ntree": enc(model()[1], FR), "dtree": enc(model()[2], FR)},
                         consume=("ntree" if which == "numerator" else "dtree", grand_product_ref.level_offset(NV, 1),
                                  grand_product_ref.level_len(NV, 1)),
                         wait=(64, lambda: enc(list(model()[0]), FR).tobytes()))
    for _h in (True, False):
        fraction(_h, "numerator")
        fraction(_h, "denominator")

    def sumcheck(fused):
        nt = 3
        tabs = {"t%d" % i: g(FR, 140 + i, N) for i in range(nt)}
        terms_ix = [[0, 1, 2], [0, 1], [2]]
        coeffs = g(FR, 145, 3)

        @case("sumcheck_round%s" % (" with r_prev" if fused else ""), "ark_hip_sumcheck_round_device", "mle", "D")
        def _(v):
            r = g(FR, 146, 1)
            dev = dict(tabs)
            outs = []
            if fused:
                dev.update({"o%d" % i: stale(FR, N // 2) for i in range(nt)})
                outs = ["o%d" % i for i in range(nt)]
            terms = [(c, ix) for c, ix in zip(dec(coeffs, FR), terms_ix)]
            bound = lambda: S.bind([dec(t, FR) for t in tabs.values()], dec(r, FR)[0], p)      # noqa: E731
            sums = lambda: S.round_sums(bound() if fused else [dec(t, FR) for t in tabs.values()], terms, p)      # noqa: E731
            host = {"term_len": np.array([3, 2, 1], dtype=np.uint32), "term_tables": np.array(sum(terms_ix, []), dtype=np.uint32),
                    "coeffs": coeffs}
            ptrs = {"d_tables": list(tabs)}
            if fused:
                host["r_prev"] = r
                ptrs["d_out_tables"] = outs
            return Built(dev, outs,
                         lambda L, x: L.ark_hip_sumcheck_round_device(fid, pp(x["d_tables"]), nt, NV, up(x["term_len"]), up(x["term_tables"]),
                                                                      vp(x["coeffs"]), 3, vp(x["r_prev"]) if fused else None,
                                                                      pp(x["d_out_tables"]) if fused else None, vp(x["wait"])),
                         lambda: {"o%d" % i: enc(t, FR) for i, t in enumerate(bound())} if fused else {},
                         host=host, ptrs=ptrs, wait=(4 * 32, lambda: enc(sums(), FR).tobytes()))
    sumcheck(False)
    sumcheck(True)

    @case("merkle_commit_fr", "ark_hip_merkle_commit_fr_device", "mle", "D")
    def _(v):
        count, n = 3, 512
        data = g(FR, 150, count * n)
        tree = lambda: merkle_ref.tree(FR, [mle_ref.ints(data[j * n:(j + 1) * n]) for j in range(count)])      # noqa: E731
        return Built({"data": data, "tree": np.full((2 * n - 1) * 32, 0x5A, dtype=np.uint8)}, ["tree"],
                     lambda L, x: L.ark_hip_merkle_commit_fr_device(fid, vp(x["data"]), count, n, n, vp(x["tree"]), vp(x["wait"])),
                     lambda: {"tree": np.frombuffer(b"".join(tree()), dtype=np.uint8)}, wait=(32, lambda: tree()[0]))


_mle()


# ---- point vectors: host scalars of the fold and of the shared-scalar multiplication ------------------------------------
def _points():
    cname = "BLS12_381_G1"
    cid = O.CID[cname]
    n = 257
    a4 = np.array([0xA11CE, 1, 2, 0], dtype=np.uint64)
    b4 = np.array([0xB0B, 3, 0, 0], dtype=np.uint64)
    pts = O.gen_bases(cid, a4, b4, 2 * n)
    lo, hi = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(pts[n:])
    words = 3 * O.fe_words(cid)
    stale_pts = np.ascontiguousarray(np.tile(O.scalar_mul(cid, pts[0], np.array([7, 0, 0, 0], dtype=np.uint64)).reshape(1, words), (n, 1)))

    def affine(x):
        return O.to_affine(cid, np.ascontiguousarray(x).reshape(-1))

    @case("sw_fold", "ark_hip_sw_fold_device", "points", "BC")
    def _(v):
        a, b = g(FR, 160 if v == 0 else 162, 1), g(FR, 161 if v == 0 else 163, 1)

        def ref():
            from algebra_amd import _lib
            out = np.zeros((n, words), dtype=np.uint64)
            rc = _lib.test_lib().ark_hip_test_host_sw_fold(cid, vp(lo.ctypes.data), vp(hi.ctypes.data), 0, vp(a.ctypes.data), vp(b.ctypes.data),
                                                          1, 0, n, vp(out.ctypes.data))
            assert rc == 0, rc
            return {"out": out}
        return Built({"lo": lo, "hi": hi, "out": stale_pts}, ["out"],
                     lambda L, x: L.ark_hip_sw_fold_device(cid, vp(x["lo"]), vp(x["hi"]), 0, vp(x["a"]), vp(x["b"]), 1, n, vp(x["out"])),
                     ref, host={"a": a, "b": b}, compare=affine)


_points()


# ---- completeness -------------------------------------------------------------------------------------------------------------
# every other *_device declaration of include/ark_hip.h, with the reason it has no case
EXCLUDED = {
    "ark_hip_msm_sw_small_device": "synchronises before it returns: the result is a host point",
    "ark_hip_msm_sw_device": "synchronises before it returns: the result is a host point",
    "ark_hip_msm_bases_prepare_device": "synchronises before it returns: the table is complete",
    "ark_hip_msm_prepared_device": "synchronises before it returns: the result is a host point",
    "ark_hip_msm_prepared_small_device": "synchronises before it returns: the result is a host point",
    "ark_hip_msm_sw_multi_device": "needs one GPU per rank",
    "ark_hip_batch_mul_device": "synchronises before it returns",
    "ark_hip_sw_add_affine_device": "synchronises before it returns",
    "ark_hip_sw_normalize_batch_device": "synchronises before it returns",
    "ark_hip_sw_check_device": "synchronises before it returns",
    "ark_hip_sw_decompress_device": "synchronises before it returns",
    "ark_hip_sw_compress_device": "output is not an MSM input, no host input",
    "ark_hip_sw_mul_device": "output is not an MSM input; its scalars are device memory",
    "ark_hip_sw_add_device": "output is not an MSM input, no host input",
    "ark_hip_fft_group_in_place_device": "output is not an MSM input: the transform over group elements",
    "ark_hip_sumcheck_prove_device": "every output is host memory behind ONE wait of the call's own; its round is covered by sumcheck_round",
    "ark_hip_sfp_fft_batch_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_add_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_sub_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_mul_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_neg_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_inverse_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_scale_device": "output is not an MSM input: one-word fields; the constant travels by value",
    "ark_hip_sfp_from_canonical_device": "output is not an MSM input: one-word fields",
    "ark_hip_sfp_into_canonical_device": "output is not an MSM input: one-word fields",
    "ark_hip_merkle_commit_sfp_device": "output is not an MSM input: one-word fields; the Fr form is covered",
    "ark_hip_merkle_open_device": "synchronises before it returns: paths and rows are host memory",
    "ark_hip_test_transcript_challenge_device": "a test hook, not an entry of the product",
    "ark_hip_set_device": "selects the calling thread's device: enqueues nothing on any stream",
    "ark_hip_get_device": "reports the calling thread's device: enqueues nothing on any stream",
}
# the sliced RCCL exchange of ark_hip_fft_sharded_device and the all-gather of ark_hip_msm_*_device_sharded need one GPU per
# rank: the former is covered without a communicator, the latter synchronise (the result is a host point)
EXCLUDED["ark_hip_msm_sw_device_sharded"] = "needs one GPU per rank"
EXCLUDED["ark_hip_msm_prepared_device_sharded"] = "needs one GPU per rank"
# the other side of the contract: what every case hands its output to
EXCLUDED["ark_hip_msm_sw_device_async"] = "a consumer, not a producer: the plain form of the MSM every case of part A enqueues"
EXCLUDED["ark_hip_msm_prepared_device_async"] = "a consumer, not a producer: the blocker of every case and the consumer of part A"


def declared_entries(header_text):
    """every ark_hip_*_device declaration (the _device_sharded and _device_async forms included), ark_hip_memcpy_d2d and
    ark_hip_memset_device"""
    names = set(re.findall(r"^int (ark_hip_\w*_device(?:_sharded|_async)?)\(", header_text, flags=re.M))
    return names | {"ark_hip_memcpy_d2d", "ark_hip_memset_device"}


def cases_of(part, group=None):
    return [c for c in CASES if part in c.parts and (group is None or c.group == group)]


GROUPS = ["A:pointwise", "A:transforms", "A:poly", "A:mle", "B", "C", "D"]
