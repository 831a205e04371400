"""Reference for the bucket array of a streamed MSM (csrc/msm.cuh MsmPiece): what every (window, bucket) cell must hold after
pieces 0 .. k, stated on discrete logarithms.  It states the operation, not the kernels: no lanes, no heavy runs, no chunks.

  Input          bases given by their logarithms to the generator G (None: the identity, all-zero limbs), scalars as ints
  BucketModel    membership from msm_sort_ref.fold_scalars / model_keys; sums[k][cell] = sum of +-k_i mod r over pieces 0 .. k
  expected       the affine points [sums] G of one dump, from ONE oracle batch_mul call
  encode_dump    a valid dump made on the CPU (XYZZ with a non-trivial ZZ), for the host tests of the checker
  check_buckets  piece k of a dump against the model; raises StageMismatch naming piece, window and bucket
  fold           sum_w 2^off_w sum_b (b + 1) bucket[w][b] on the logarithms: ties the model to the oracle's MSM without a GPU

A stored bucket is a canonical XYZZ point over the curve's coordinate field, x | y | zz | zzz in Montgomery limbs (csrc/ec.cuh):
(X / ZZ, Y / ZZZ) with ZZ^3 = ZZZ^2; the identity is (1, 1, 0, 0).  Cell (w, b) sits at index (w << (c - 1)) + b; the top
`narrow` windows are c - 1 bits wide and own the lower half of their cells only -- the upper half is written as the identity by
the first piece and never touched again.
"""
import ctypes as C
import random

import numpy as np

import msm_sort_ref as R
import oracle_lib as O
import pyref
from msm_sort_ref import StageMismatch

HEADER = ("c", "W", "narrow", "nbuckets", "pt_bytes", "npieces", "pieces_run", "bad_piece", "L0", "m", "mn", "nbits", "Q", "two_digit",
          "npairs", "lazy")
KNOBS = ("c", "heavy", "hb", "probe", "compact", "lazy", "tile", "big_slices", "prepared")
KNOB_DEFAULTS = dict(c=0, heavy=0, hb=-1, probe=1, compact=1, lazy=1, tile=0, big_slices=1, prepared=0)
NO_PIECE = (1 << 64) - 1
ERR_ARG, ERR_SIZE, ERR_SCALAR_RANGE = -1, -2, -4


# ---- the curve's side ------------------------------------------------------------------------------------------------------
class CurveRef:
    """Coordinate field, scalar field and generator of a curve; cached per name"""
    _cache = {}

    def __new__(cls, name):
        if name not in cls._cache:
            self = super().__new__(cls)
            bf, sf, ext, beta, _ = pyref.CURVE_PARAMS[name]
            self.name, self.cid, self.field = name, O.CID[name], sf
            self.p, self.r = pyref.MODULI[bf][0], pyref.MODULI[sf][0]
            self.bits = self.r.bit_length()
            self.F = pyref.Fld(self.p, beta)
            self.ext, self.nl = ext, pyref.nlimbs(self.p)
            self.fw = self.nl * ext                      # u64 words of one coordinate
            self.one = self.F.from_int(1)
            self.g_jac = O.scalar_mul(self.cid, O.generator(self.cid), np.array([1, 0, 0, 0], dtype=np.uint64))
            cls._cache[name] = self
        return cls._cache[name]

    def mul_gen(self, logs):
        """[k] G for every k of `logs` (ints mod r) as affine limbs (len, 2 fw); k = 0 gives all-zero limbs.  One oracle call."""
        logs = [int(k) % self.r for k in logs]
        if not logs:
            return np.zeros((0, 2 * self.fw), dtype=np.uint64)
        out = O.batch_mul(self.cid, self.g_jac, R.ints_to_limbs(logs))
        zero = np.array([k == 0 for k in logs])
        out[zero] = 0
        return out

    def bases(self, logs):
        """the base array of an Input: None -> the identity (all-zero limbs)"""
        return self.mul_gen([0 if k is None else k for k in logs])


class Input:
    """One MSM cut into pieces.  logs[i]: base i = [logs[i]] G, None: the identity; scalars: ints as the entry takes them (below
    2^256; `mont`: the Montgomery words of the scalars meant); sizes: the pieces"""

    def __init__(self, curve, logs, scalars, sizes, mont=0):
        assert len(logs) == len(scalars) == sum(sizes) and all(s > 0 for s in sizes)
        self.curve, self.logs, self.sizes, self.mont = curve, list(logs), list(sizes), mont
        self.scalars = R.ints_to_limbs([int(s) for s in scalars])
        self.cr = CurveRef(curve)
        self._bases = None

    @property
    def bases(self):
        if self._bases is None:
            self._bases = self.cr.bases(self.logs)
        return self._bases

    def bounds(self):
        b = np.concatenate([[0], np.cumsum(self.sizes)])
        return [(int(b[k]), int(b[k + 1])) for k in range(len(self.sizes))]


# ---- the model -------------------------------------------------------------------------------------------------------------
def plan_header(curve, c, n_by_piece, HB=None):
    """The header a dump of `curve` under window size c must carry, made without a device (the layout rule of msm_sort_ref;
    HB: the sort split per piece -- 0 for the few buckets and few scalars used here)"""
    cr = CurveRef(curve)
    W, narrow = R.layout(c, cr.bits)
    HB = [0] * len(n_by_piece) if HB is None else HB
    return dict(c=c, W=W, narrow=narrow, nbuckets=W << (c - 1), pt_bytes=32 * cr.fw, npieces=len(n_by_piece),
                pieces=[dict(HB=hb, LB=c - 1 - hb, n=n, ngroups=1) for hb, n in zip(HB, n_by_piece)])


class BucketModel:
    def __init__(self, inp, header, heavy=0):
        self.inp, self.h, self.heavy = inp, header, heavy
        cr = inp.cr
        c, W, narrow = header["c"], header["W"], header["narrow"]
        self.B = 1 << (c - 1)
        nbk = W * self.B
        assert header["nbuckets"] == nbk and [p["n"] for p in header["pieces"]] == inp.sizes
        self.widths = R.window_widths(c, W, narrow)
        self.sums, self.counts, self.out_of_range, self.keys = [], [], [], []
        cur = [0] * nbk
        for lo, hi in inp.bounds():
            v, flip, bad = R.fold_scalars(inp.scalars[lo:hi], cr.field, inp.mont)
            keys = R.model_keys(v, flip, c, W, narrow)
            self.keys.append(keys)
            self.out_of_range.append(bool(bad))
            cnt = np.zeros(nbk, dtype=np.int64)
            cur = list(cur)
            for w in range(W):
                idx = np.flatnonzero(keys[w] != R.KEY_NONE)
                kw = keys[w][idx]
                cells = (w * self.B + (kw & np.uint32(0x7FFFFFFF)).astype(np.int64))
                np.add.at(cnt, cells, 1)
                for i, cell, neg in zip(idx.tolist(), cells.tolist(), (kw >> np.uint32(31)).tolist()):
                    k = inp.logs[lo + i]
                    if k is not None:
                        cur[cell] = (cur[cell] - k if neg else cur[cell] + k) % cr.r
            self.counts.append(cnt)
            self.sums.append(cur)
        self._expected = {}

    def cell(self, w, b):
        return w * self.B + b

    def where(self, cell):
        return cell // self.B, cell % self.B

    def upper_half(self):
        """cells no digit can reach: the upper half of the narrow windows"""
        W, narrow = self.h["W"], self.h["narrow"]
        m = np.zeros(W * self.B, dtype=bool)
        for w in range(W - narrow, W):
            m[w * self.B + self.B // 2:(w + 1) * self.B] = True
        return m

    def expected(self, k):
        """affine limbs (nbuckets, 2 fw) of piece k's buckets; all-zero rows: the identity"""
        if k not in self._expected:
            self._expected[k] = self.inp.cr.mul_gen(self.sums[k])
        return self._expected[k]

    def sort_dump(self, k):
        """msm_sort_ref.build_dump of piece k's scalars: its hctr words are what the device must count"""
        lo, hi = self.inp.bounds()[k]
        P = self.h["pieces"][k]
        hd = R.make_header(hi - lo, self.h["c"], self.h["W"], self.h["narrow"], P["HB"])
        return R.build_dump(self.inp.scalars[lo:hi], self.inp.cr.field, hd, self.inp.mont, heavy=self.heavy)

    def regime(self, k):
        """(chunk items, heavy runs, threshold, range flag) of piece k and the cells of its heavy runs"""
        d = self.sort_dump(k)
        P = self.h["pieces"][k]
        cells = sorted(int(R.slot_to_bucket(int(s), P["HB"], P["LB"])) for s in d["hlist"][0][:, 0])
        thr = int(d["hctr"][2])
        assert cells == np.flatnonzero(self.counts[k] > thr).tolist(), "the sort model and the bucket model disagree on the heavy runs"
        return tuple(int(x) for x in d["hctr"][:4]), cells

    def fold(self, k=None):
        """sum_w 2^off_w sum_b (b + 1) sums[w][b] mod r of piece k (default: the last)"""
        s = self.sums[-1 if k is None else k]
        total, off = 0, 0
        for w, cw in enumerate(self.widths):
            total += sum((b + 1) * s[w * self.B + b] for b in range(self.B)) << off
            off += cw
        return total % self.inp.cr.r


# ---- stored points ---------------------------------------------------------------------------------------------------------
def identity_limbs(cr):
    z = cr.F.enc(cr.F.zero())
    one = cr.F.enc(cr.one)
    return np.concatenate([one, one, z, z])


def encode_bucket(cr, aff_limbs, lam):
    """the affine point (limbs; all-zero: the identity) as stored XYZZ limbs with ZZ = lam^2, ZZZ = lam^3"""
    if not np.any(aff_limbs):
        return identity_limbs(cr)
    F = cr.F
    x, y = F.dec(aff_limbs[:cr.fw]), F.dec(aff_limbs[cr.fw:])
    zz = F.mul(lam, lam)
    zzz = F.mul(zz, lam)
    return np.concatenate([F.enc(F.mul(x, zz)), F.enc(F.mul(y, zzz)), F.enc(zz), F.enc(zzz)])


def encode_dump(model, seed=1):
    """A correct dump for `model` made on the CPU: every non-identity bucket with a ZZ of its own"""
    cr, h = model.inp.cr, model.h
    rng = random.Random(seed)
    buckets, hctr = [], []
    for k in range(h["npieces"]):
        exp = model.expected(k)
        rows = []
        for cell in range(h["nbuckets"]):
            lam = cr.F.from_int(rng.randrange(2, cr.p) if cr.ext == 1 else (rng.randrange(2, cr.p), rng.randrange(1, cr.p)))
            rows.append(encode_bucket(cr, exp[cell], lam))
        buckets.append(np.stack(rows))
        w = np.zeros(16, dtype=np.uint32)
        w[:4] = model.regime(k)[0]
        hctr.append(w)
    return dict(header=h, buckets=buckets, hctr=hctr, rc=0)


def _coords(cr, row):
    """the four coordinates of a stored bucket as raw integers per component (not yet out of Montgomery form)"""
    b = np.ascontiguousarray(row, dtype="<u8").tobytes()
    step = 8 * cr.nl
    return [int.from_bytes(b[i:i + step], "little") for i in range(0, len(b), step)]


# ---- the checker -----------------------------------------------------------------------------------------------------------
def check_buckets(dump, model, k, skip_unchanged=False):
    """Piece k of `dump` against `model`.  skip_unchanged: piece k - 1 of the same dump has been checked -- a cell that holds the
    same bytes under the same expectation is not decoded again."""
    cr, h = model.inp.cr, model.h
    F, fw = cr.F, cr.fw
    bk = np.asarray(dump["buckets"][k])
    if bk.shape != (h["nbuckets"], 4 * fw):
        raise StageMismatch("buckets", "piece %d: %s words, the plan has %d buckets of %d" % (k, bk.shape, h["nbuckets"], 4 * fw))
    exp = model.expected(k)
    ident = identity_limbs(cr)
    upper = model.upper_half()
    is_ident = (bk == ident).all(axis=1)
    same_as_before = np.zeros(h["nbuckets"], dtype=bool)
    if k > 0 and skip_unchanged:
        same_as_before = (bk == np.asarray(dump["buckets"][k - 1])).all(axis=1) & (exp == model.expected(k - 1)).all(axis=1)
    ncomp = 4 * cr.ext
    for cell in range(h["nbuckets"]):
        w, b = model.where(cell)
        where = "piece %d, window %d, bucket %d: " % (k, w, b)
        row = bk[cell]
        if upper[cell] and not is_ident[cell]:
            raise StageMismatch("buckets", where + "the upper half of a narrow window must stay the identity (1, 1, 0, 0)")
        want_ident = not np.any(exp[cell])
        if is_ident[cell] and want_ident:
            continue
        if same_as_before[cell]:
            continue
        raw = _coords(cr, row)
        assert len(raw) == ncomp
        for j, v in enumerate(raw):
            if v >= cr.p:
                raise StageMismatch("buckets", where + "coordinate %s is not canonical (a limb vector of p or more)"
                                    % ("x", "y", "zz", "zzz")[j // cr.ext])
        x, y, zz, zzz = (F.dec(row[j * fw:(j + 1) * fw]) for j in range(4))
        if zz == F.zero():
            if want_ident:
                raise StageMismatch("buckets", where + "the identity is stored as (1, 1, 0, 0), found another point with zz = 0")
            raise StageMismatch("buckets", where + "holds the identity, the model has a point (sum %d entries so far)"
                                % sum(int(c[cell]) for c in model.counts[:k + 1]))
        if want_ident:
            raise StageMismatch("buckets", where + "holds a point, the model has the identity")
        if F.mul(F.mul(zz, zz), zz) != F.mul(zzz, zzz):
            raise StageMismatch("buckets", where + "zz^3 != zzz^2")
        ex, ey = F.dec(exp[cell][:fw]), F.dec(exp[cell][fw:])
        if x != F.mul(ex, zz) or y != F.mul(ey, zzz):
            what = "the negative of the model's point" if x == F.mul(ex, zz) and y == F.neg(F.mul(ey, zzz)) else "not the model's point"
            if k > 0 and (row == np.asarray(dump["buckets"][k - 1])[cell]).all():
                what += " (unchanged since piece %d)" % (k - 1)
            raise StageMismatch("buckets", where + what)


def check_hctr(dump, model, k):
    want, _ = model.regime(k)
    got = tuple(int(x) for x in np.asarray(dump["hctr"][k])[:4])
    if got != want:
        raise StageMismatch("hctr", "piece %d: (items, runs, threshold, range flag) = %s, the model says %s" % (k, got, want))
    return want


def check_dump(dump, model):
    """every piece's counters and buckets; returns the regimes"""
    out = []
    for k in range(len(dump["buckets"])):
        out.append(check_hctr(dump, model, k))
        check_buckets(dump, model, k, skip_unchanged=True)
    return out


# ---- the hook --------------------------------------------------------------------------------------------------------------
def _knob_record(knobs):
    bad = set(knobs) - set(KNOBS)
    assert not bad, bad
    k = dict(KNOB_DEFAULTS, **knobs)
    return (C.c_int32 * 12)(*([int(k[name]) for name in KNOBS] + [0, 0, 0]))


def _header(hdr):
    h = dict(zip(HEADER, [int(x) for x in hdr]))
    h["pieces"] = [dict(zip(("HB", "LB", "n", "ngroups"), [int(x) for x in hdr[16 + 4 * k:20 + 4 * k]])) for k in range(h["npieces"])]
    return h


def gpu_pieces(inp, bases=None, scalars=None, short_caps=None, **knobs):
    """ark_hip_test_msm_pieces: a header-only call sizes the arrays, the second call fills them.  bases / scalars: device tensors
    to pass instead of the Input's host arrays.  short_caps: (hctr words, bucket bytes) to take off the capacities.
    Returns dict(header, rc, hctr[k], buckets[k], result) -- the arrays of the pieces that ran."""
    from algebra_amd import _lib
    T = _lib.test_lib()
    cr = inp.cr
    n = len(inp.logs)
    on_device = bases is not None
    if on_device:
        pb, ps = C.c_void_p(bases.data_ptr()), C.c_void_p(scalars.data_ptr())
    else:
        hb, hs = np.ascontiguousarray(inp.bases), np.ascontiguousarray(inp.scalars)
        pb, ps = hb.ctypes.data_as(C.c_void_p), hs.ctypes.data_as(C.c_void_p)
    sizes = (C.c_size_t * len(inp.sizes))(*inp.sizes)
    rec, hdr = _knob_record(knobs), (C.c_uint64 * 80)()
    args = (cr.cid, pb, ps, int(on_device), n, inp.mont, sizes, len(inp.sizes), rec, hdr)
    rc = T.ark_hip_test_msm_pieces(*args, None, 0, None, 0, None)
    if rc:
        return dict(header=None, rc=rc)
    h = _header(hdr)
    assert h["pt_bytes"] == 32 * cr.fw and h["nbuckets"] == h["W"] << (h["c"] - 1)
    np_, nbk = h["npieces"], h["nbuckets"]
    hctr = np.full(16 * np_, 0xDEADBEEF, dtype=np.uint32)
    buckets = np.full((np_, nbk, 4 * cr.fw), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    result = np.zeros(3 * cr.fw, dtype=np.uint64)
    cap_h, cap_b = 16 * np_ - (short_caps[0] if short_caps else 0), buckets.nbytes - (short_caps[1] if short_caps else 0)
    rc = T.ark_hip_test_msm_pieces(*args, hctr.ctypes.data_as(C.c_void_p), cap_h, buckets.ctypes.data_as(C.c_void_p), cap_b,
                                   result.ctypes.data_as(C.c_void_p))
    h2 = _header(hdr)
    run = h2["pieces_run"] if rc in (0, ERR_SCALAR_RANGE) else 0
    if rc == ERR_SCALAR_RANGE:
        run -= 1   # the piece that raised the flag ran, its arrays were not copied
    assert {k: h2[k] for k in HEADER[:6]} == {k: h[k] for k in HEADER[:6]}, "the two calls planned differently"
    return dict(header=h2, rc=rc, hctr=[hctr[16 * k:16 * k + 16] for k in range(run)], buckets=[buckets[k] for k in range(run)],
                result=result, raw=(hctr, buckets))
