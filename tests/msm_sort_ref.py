"""Reference for the integer stages of the MSM pipeline (csrc/msm.cuh K0c / K1 / K1n / K3b / msm_find_heavy_kernel,
csrc/msm_sort.cuh), in Python ints and numpy.  It states the operations -- fold, signed digits, a counting sort by bucket
slot, a load-class order, a list of long runs -- not the kernels: no tiles, no super-bucket passes, no LDS.

  magnitude / digits        one scalar at a time, on Python ints (the statement the rest is checked against)
  fold_scalars / model_keys the same over an array (ints for the fold, numpy for the windows)
  build_dump                a valid stage dump made on the CPU with a plain counting sort
  check_dump                every array of a dump (ark_hip_test_msm_sort_stages, or build_dump) against the model; raises
                            StageMismatch, whose message starts with the name of the array that is wrong
"""
import ctypes as C

import numpy as np

import pyref

KEY_NONE = 0xFFFFFFFF
SCALAR_FIELD = {"BN254_G1": "BN254_FR", "BLS12_381_G1": "BLS12_381_FR", "BLS12_377_G1": "BLS12_377_FR",
                "BLS12_377_G2": "BLS12_377_FR", "BLS12_381_G2": "BLS12_381_FR"}
CURVES = ["BN254_G1", "BLS12_381_G1", "BLS12_377_G1", "BLS12_377_G2", "BLS12_381_G2"]
KNOBS = ("c", "hb", "tile", "heavy", "groups", "big_slices", "compact", "probe")
KNOB_DEFAULTS = dict(c=0, hb=-1, tile=0, heavy=0, groups=0, big_slices=1, compact=1, probe=1)
HEADER = ("c", "W", "narrow", "n_carried", "compacted", "ngroups", "HB", "LB", "tile", "ntiles", "nthist", "stage_cap", "big_on",
          "shift", "HEAVY_CHUNK", "PART_BIG", "max_heavy", "max_items", "noblk", "nsums", "lds_a", "lds_b", "SCAN_SMALL_MAX", "n")
GEOMETRY = ("HB", "LB", "nsuper", "tile", "ntiles", "nthist", "lds_a", "lds_b", "stage_cap", "big_on", "big_region", "noblk",
            "nohist", "nsums", "mean_load", "forced_thresh", "max_heavy", "max_items", "W", "narrow", "accepted", "PART_LDS_WORDS",
            "PART_SCATTER_LDS_MAX", "PART_BIG", "SCAN_SMALL_MAX", "HEAVY_CHUNK", "SCAN_TILE", "ORDER_TILE", "ORDER_BINS", "ngroups")


class StageMismatch(AssertionError):
    def __init__(self, array, what):
        super().__init__("%s: %s" % (array, what))
        self.array = array


def field_modulus(field):
    r = pyref.MODULI[field][0]
    return r, r.bit_length()


# ---- one scalar at a time -----------------------------------------------------------------------------------------------
def magnitude(s, r, bits, mont=0):
    """(v, flip, out_of_range) of the 256-bit word s: out of Montgomery form first when `mont`; s >= 2^bits is out of range and
    counts as 0; s in [r, 2^bits) is s - r; then v = min(s, r - s), flip = the second was taken; 0 stays 0 without a flip."""
    if mont:
        s = s * pow(pyref.R_of(r), -1, r) % r
    out_of_range = s >> bits != 0
    if out_of_range:
        s = 0
    if s >= r:
        s -= r
    t = r - s
    if t < s:
        return t, 1, out_of_range
    return s, 0, out_of_range


def layout(c, bits):
    """msm_window_layout: W windows of c bits, the top `narrow` of them one bit narrower so that the widths sum to bits; or, where
    the deficit cannot be spread one bit per window, uniform widths that cover bits + 1"""
    w = (bits + c - 1) // c
    deficit = w * c - bits
    if deficit > w or c < 3:
        return (bits + c) // c, 0
    return w, deficit


def window_widths(c, W, narrow):
    """msm_window_width for w = 0 .. W - 1"""
    return [c - 1 if w >= W - narrow else c for w in range(W)]


def digits(v, c, W, narrow):
    """Signed digits of v, lowest window first: window w takes its cw bits plus the carry, and gives a carry of one when that is
    at least half of 2^cw (the reference's make_digits rule, as msm.cuh cites it: carry = (digit + radix / 2) >> c); the top window
    takes everything that is left and is not recoded."""
    out, carry, off = [], 0, 0
    for w, cw in enumerate(window_widths(c, W, narrow)):
        if w < W - 1:
            raw = ((v >> off) & ((1 << cw) - 1)) + carry
            carry = 1 if raw >= (1 << (cw - 1)) else 0
            out.append(raw - (carry << cw))
        else:
            out.append((v >> off) + carry)
        off += cw
    return out


def key_of(d, flip):
    """sign ^ flip in bit 31, |d| - 1 below it; no digit: 0xffffffff"""
    if d == 0:
        return KEY_NONE
    return ((1 if d < 0 else 0) ^ flip) << 31 | (abs(d) - 1)


# ---- the same over an array ------------------------------------------------------------------------------------------------
def scalars_to_ints(scalars):
    """(n, 4) uint64 little-endian limbs -> list of Python ints"""
    b = np.ascontiguousarray(scalars, dtype="<u8").tobytes()
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


def ints_to_limbs(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).copy()


def fold_scalars(scalars, field, mont=0, sbytes=0, sbits=0):
    """v as (n, 4) uint64 limbs, flip (n,) uint32, and whether any scalar was out of range.  Narrow unsigned scalars (sbytes != 0):
    no fold, masked to sbits."""
    if sbytes:
        v = np.zeros((len(scalars), 4), dtype=np.uint64)
        v[:, 0] = np.asarray(scalars).astype(np.uint64) & np.uint64((1 << sbits) - 1)
        return v, np.zeros(len(scalars), dtype=np.uint32), False
    r, bits = field_modulus(field)
    rinv = pow(pyref.R_of(r), -1, r)
    half = r >> 1   # r - s < s  <=>  s > (r - 1) / 2
    vs, flips, bad = [], [], False
    for s in scalars_to_ints(scalars):
        if mont:
            s = s * rinv % r
        if s >> bits:
            bad, s = True, 0
        if s >= r:
            s -= r
        if s > half:
            vs.append(r - s)
            flips.append(1)
        else:
            vs.append(s)
            flips.append(0)
    return ints_to_limbs(vs), np.array(flips, dtype=np.uint32), bad


def model_keys(v, flip, c, W, narrow):
    """keys[W][n] (uint32) of the folded magnitudes v (limbs) with their flips"""
    n = len(v)
    vv = np.concatenate([v, np.zeros((n, 1), dtype=np.uint64)], axis=1)
    keys = np.empty((W, n), dtype=np.uint32)
    carry = np.zeros(n, dtype=np.int64)
    off = 0
    for w, cw in enumerate(window_widths(c, W, narrow)):
        take = cw if w < W - 1 else 63   # the top window: everything that is left (its digit must still fit: checked below)
        q, sh = off // 64, off % 64
        lo = vv[:, min(q, 4)] >> np.uint64(sh)
        if sh and q + 1 <= 4:
            lo = lo | (vv[:, q + 1] << np.uint64(64 - sh))
        raw = (lo & np.uint64((1 << take) - 1)).astype(np.int64) + carry
        if w < W - 1:
            carry = (raw >= (1 << (cw - 1))).astype(np.int64)
            d = raw - (carry << cw)
        else:
            d = raw
            for limb in range(4):   # nothing may be left above the 63 bits taken
                above = off + 63 - 64 * limb
                if above < 64 and np.any(vv[:, limb] >> np.uint64(max(above, 0))):
                    raise StageMismatch("model", "a magnitude reaches past the top window")
        if np.any(np.abs(d) > (1 << (cw - 1))):
            raise StageMismatch("model", "digit of window %d beyond half of 2^%d" % (w, cw))
        neg = (d < 0).astype(np.uint32)
        key = ((neg ^ flip) << np.uint32(31)) | (np.abs(d) - 1).astype(np.uint32)
        keys[w] = np.where(d == 0, np.uint32(KEY_NONE), key)
        off += cw
    return keys


def slot_of_bucket(wl, b, HB, LB):
    """sort slot of bucket b of the group's window wl: the low HB bits of b pick the super-bucket"""
    return (wl << (HB + LB)) | ((b & ((1 << HB) - 1)) << LB) | (b >> HB)


def slot_to_bucket(slot, HB, LB):
    """msm_slot_to_bucket as msm_sort.cuh documents it: slot = (w << B) | (low HB bits << LB) | (high LB bits)"""
    B = HB + LB
    w, inn = slot >> B, slot & ((1 << B) - 1)
    low, high = inn >> LB, inn & ((1 << LB) - 1)
    return (w << B) | (high << HB) | low


def sort_within(group, value):
    """`value` (uint32) ordered by group, ascending inside every group: one sort of the packed (group, value) words -- a lexsort
    over the two keys, vectorised"""
    packed = (np.asarray(group).astype(np.uint64) << np.uint64(32)) | np.asarray(value).astype(np.uint64)
    packed.sort()
    return (packed & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def order_shift(n_carried, W, nbuckets):
    """class width 2^shift of the order pass: the mean load falls below class 64"""
    mean, shift = n_carried * W // nbuckets, 0
    while (mean >> shift) >= 64:
        shift += 1
    return shift


def heavy_threshold(total, nslots, forced):
    t = max(total // 154000, 64)
    if nslots >= 32768:
        t = max(t, 4 * (total // nslots))
    return forced if forced else t


def heavy_chunk(total, base):
    return 4 * base if total >= 1 << 23 else 2 * base if total >= 1 << 22 else base


class Model:
    """What the stages must produce for `scalars`, up to the freedoms the pipeline has (order inside a bucket, order inside a load
    class, order of the heavy list)."""

    def __init__(self, scalars, field, header, mont=0, sbytes=0, sbits=0, folded=None):
        scalars = np.asarray(scalars)
        self.h = header
        # folded: fold_scalars of the same scalars, computed once for several dumps
        v, flip, self.out_of_range = folded if folded is not None else fold_scalars(scalars, field, mont, sbytes, sbits)
        self.nonzero = np.flatnonzero(v.any(axis=1)).astype(np.uint32)
        self.zeros = len(scalars) - len(self.nonzero)
        if header["compacted"]:
            self.index = self.nonzero
            v, flip = v[self.nonzero], flip[self.nonzero]
            self.cscal = np.ascontiguousarray(scalars[self.nonzero]).view(np.uint32).reshape(len(self.nonzero), -1)
        else:
            self.index = np.arange(len(scalars), dtype=np.uint32)
        self.n_carried = len(self.index)
        self.keys = model_keys(v, flip, header["c"], header["W"], header["narrow"])

    def group(self, g):
        """(counts per slot, expected offsets, expected `sorted` with every bucket's entries ascending) of window group g"""
        h = self.h
        G = h["groups"][g]
        HB, LB = h["HB"], h["LB"]
        keys = self.keys[G["w0"]:G["w0"] + G["Wg"]]
        wl, i = np.nonzero(keys != KEY_NONE)
        k = keys[wl, i]
        b = (k & np.uint32(0x7FFFFFFF)).astype(np.int64)
        slot = slot_of_bucket(wl.astype(np.int64), b, HB, LB)
        if np.any(slot_to_bucket(slot, HB, LB) != ((wl.astype(np.int64) << (HB + LB)) | b)):
            raise StageMismatch("model", "slot_of_bucket and slot_to_bucket disagree")
        value = self.index[i] | (k & np.uint32(0x80000000))
        counts = np.bincount(slot, minlength=G["nslots"]).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        return counts, offsets, sort_within(slot, value)


# ---- a dump made on the CPU --------------------------------------------------------------------------------------------------
def make_header(n, c, W, narrow, HB, ngroups=1, compacted=0, n_carried=None, big_on=0, part_big=1 << 17, heavy_chunk_words=1024,
                tile=8192):
    B = c - 1
    nc = n if n_carried is None else n_carried
    W0 = (W + 1) // 2 if ngroups == 2 else W
    groups = [dict(w0=0, Wg=W0, nslots=W0 << B, nbk_g=W0 << B)]
    if ngroups == 2:
        groups.append(dict(w0=W0, Wg=W - W0, nslots=(W - W0) << B, nbk_g=(W - W0) << B))
    return dict(c=c, W=W, narrow=narrow, n_carried=nc, compacted=compacted, ngroups=ngroups, HB=HB, LB=B - HB, tile=tile,
                ntiles=-(-nc // tile), big_on=big_on, shift=order_shift(nc, W, W << B), HEAVY_CHUNK=heavy_chunk_words,
                PART_BIG=part_big, n=n, groups=groups)


def build_dump(scalars, field, header, mont=0, sbytes=0, sbits=0, heavy=0):
    """A valid dump for `header` (make_header; n_carried is filled in here): a straightforward counting sort of the model's keys"""
    h = dict(header)
    m = Model(scalars, field, h, mont, sbytes, sbits)
    if h["n_carried"] != m.n_carried:
        h.update(make_header(h["n"], h["c"], h["W"], h["narrow"], h["HB"], h["ngroups"], h["compacted"], m.n_carried, h["big_on"],
                             h["PART_BIG"], h["HEAVY_CHUNK"], h["tile"]))
        m = Model(scalars, field, h, mont, sbytes, sbits)
    d = dict(header=h, keys=m.keys.copy(), hctr=np.zeros(16, dtype=np.uint32), sorted=[], offsets=[], order=[], hlist=[], hitems=[])
    if h["compacted"]:
        d["cidx"], d["cscal"] = m.index.copy(), m.cscal.copy()
    d["hctr"][3] = 1 if m.out_of_range else 0
    for g, G in enumerate(h["groups"]):
        counts, offsets, srt = m.group(g)
        full = np.full(G["Wg"] * h["n_carried"], KEY_NONE, dtype=np.uint32)
        full[:len(srt)] = srt
        d["sorted"].append(full)
        d["offsets"].append(offsets.astype(np.uint32))
        cls = np.minimum(counts >> h["shift"], 255)
        d["order"].append(np.argsort(-cls, kind="stable").astype(np.uint32))
        total = int(offsets[-1])
        thr, chunk = heavy_threshold(total, G["nslots"], heavy), heavy_chunk(total, h["HEAVY_CHUNK"])
        runs = np.flatnonzero(counts > thr)
        items = -(-counts[runs] // chunk)
        first = np.concatenate([[0], np.cumsum(items)[:-1]]) if len(runs) else np.zeros(0, dtype=np.int64)
        d["hlist"].append(np.stack([runs, first, items], axis=1).astype(np.uint32).reshape(-1, 3))
        d["hitems"].append(np.array([(b, q) for b, k in zip(runs, items) for q in range(k)], dtype=np.uint32).reshape(-1, 2))
        d["hctr"][4 * g:4 * g + 3] = (int(items.sum()), len(runs), thr)
        if h["big_on"]:
            d["hctr"][8 + g] = int(np.count_nonzero(counts.reshape(-1, 1 << h["LB"]).sum(axis=1) > h["PART_BIG"]))
    return d


# ---- the checker -----------------------------------------------------------------------------------------------------------
def _first(mask):
    return int(np.flatnonzero(mask)[0])


def check_dump(scalars, dump, field, mont=0, sbytes=0, sbits=0, heavy=0, folded=None):
    """Every array of `dump` against the model of `scalars`; returns the Model (its per-group counts serve the regime asserts).
    heavy: the forced heavy-run threshold the dump was made with (0: the rule's)."""
    h = dump["header"]
    m = Model(scalars, field, h, mont, sbytes, sbits, folded)
    nc = h["n_carried"]
    if nc != m.n_carried:
        raise StageMismatch("header", "n_carried %d, the model carries %d of %d scalars" % (nc, m.n_carried, len(scalars)))
    if h["compacted"]:
        cidx = np.asarray(dump["cidx"])
        if len(cidx) != nc or np.any(cidx != m.nonzero):
            raise StageMismatch("cidx", "not the ascending indices of the non-zero scalars (first difference at %d)"
                                % (_first(cidx != m.nonzero) if len(cidx) == nc else -1))
        if np.any(np.asarray(dump["cscal"]) != m.cscal):
            raise StageMismatch("cscal", "compacted scalar %d is not scalar cidx[%d]" % ((_first((dump["cscal"] != m.cscal).any(axis=1)),) * 2))
    keys = np.asarray(dump["keys"])
    if keys.shape != m.keys.shape or np.any(keys != m.keys):
        w, i = [int(x[0]) for x in np.nonzero(keys != m.keys)]
        raise StageMismatch("keys", "window %d, scalar %d: 0x%08x, the model says 0x%08x" % (w, i, keys[w, i], m.keys[w, i]))
    hctr = np.asarray(dump["hctr"])
    if int(hctr[3]) != (1 if m.out_of_range else 0):
        raise StageMismatch("hctr", "range flag %d with %s scalar out of range" % (hctr[3], "a" if m.out_of_range else "no"))
    shift = order_shift(nc, h["W"], h["W"] << (h["c"] - 1))
    if h["shift"] != shift:
        raise StageMismatch("header", "shift %d, the rule gives %d" % (h["shift"], shift))
    m.counts = []
    for g, G in enumerate(h["groups"]):
        where = "group %d: " % g
        nslots = G["nslots"]
        counts, exp_off, exp_sorted = m.group(g)
        m.counts.append(counts)
        total = int(exp_off[-1])
        off = np.asarray(dump["offsets"][g]).astype(np.int64)
        if len(off) != nslots + 1:
            raise StageMismatch("offsets", where + "%d entries for %d slots" % (len(off), nslots))
        if off[0] != 0:
            raise StageMismatch("offsets", where + "offsets[0] = %d" % off[0])
        if np.any(np.diff(off) < 0):
            raise StageMismatch("offsets", where + "decreases at slot %d" % _first(np.diff(off) < 0))
        if off[nslots] != total:
            raise StageMismatch("offsets", where + "sentinel offsets[%d] = %d, the group has %d live keys" % (nslots, off[nslots], total))
        if np.any(off != exp_off):
            s = _first(off != exp_off)
            raise StageMismatch("offsets", where + "slot %d (bucket %d) starts at %d, the model says %d"
                                % (s, slot_to_bucket(s, h["HB"], h["LB"]), off[s], exp_off[s]))
        srt = np.asarray(dump["sorted"][g])
        if len(srt) != G["Wg"] * nc:
            raise StageMismatch("sorted", where + "%d words for %d windows of %d" % (len(srt), G["Wg"], nc))
        if np.any(srt[total:] != KEY_NONE):
            raise StageMismatch("sorted", where + "word %d, past offsets[nslots] = %d, was written" % (total + _first(srt[total:] != KEY_NONE), total))
        slot_of_pos = np.repeat(np.arange(nslots, dtype=np.int64), counts)
        got = sort_within(slot_of_pos, srt[:total])   # ascending inside every bucket, on both sides
        if np.any(got != exp_sorted):
            p = _first(got != exp_sorted)
            s = int(slot_of_pos[p])
            raise StageMismatch("sorted", where + "slot %d (bucket %d): holds 0x%08x where the model has 0x%08x"
                                % (s, slot_to_bucket(s, h["HB"], h["LB"]), got[p], exp_sorted[p]))
        order = np.asarray(dump["order"][g]).astype(np.int64)
        if len(order) != G["nbk_g"] or order.max() >= G["nbk_g"] or np.any(np.bincount(order, minlength=G["nbk_g"]) != 1):
            raise StageMismatch("order", where + "not a permutation of the group's %d buckets" % G["nbk_g"])
        cls = np.minimum(counts >> shift, 255)[order]
        if np.any(np.diff(cls) > 0):
            p = _first(np.diff(cls) > 0)
            raise StageMismatch("order", where + "load class rises from %d to %d at position %d" % (cls[p], cls[p + 1], p + 1))
        thr, chunk = heavy_threshold(total, nslots, heavy), heavy_chunk(total, h["HEAVY_CHUNK"])
        nitems, nruns, got_thr = (int(x) for x in hctr[4 * g:4 * g + 3])
        if got_thr != thr:
            raise StageMismatch("hctr", where + "threshold %d, the rule gives %d for %d entries in %d slots" % (got_thr, thr, total, nslots))
        hl = np.asarray(dump["hlist"][g]).astype(np.int64).reshape(-1, 3)
        heavy_slots = np.flatnonzero(counts > thr)
        if len(hl) != nruns:
            raise StageMismatch("hlist", where + "%d entries, hctr counts %d" % (len(hl), nruns))
        if len(np.unique(hl[:, 0])) != len(hl):
            raise StageMismatch("hlist", where + "a run is listed twice")
        if len(hl) != len(heavy_slots) or np.any(np.sort(hl[:, 0]) != heavy_slots):
            raise StageMismatch("hlist", where + "lists %d runs, %d are longer than %d: %s"
                                % (len(hl), len(heavy_slots), thr, sorted(set(hl[:, 0].tolist()) ^ set(heavy_slots.tolist()))[:4]))
        want_items = -(-counts[hl[:, 0]] // chunk)
        if np.any(hl[:, 2] != want_items):
            p = _first(hl[:, 2] != want_items)
            raise StageMismatch("hlist", where + "run of slot %d: items %d, ceil(%d / %d) = %d"
                                % (hl[p, 0], hl[p, 2], counts[hl[p, 0]], chunk, want_items[p]))
        by_first = hl[np.argsort(hl[:, 1], kind="stable")]
        ends = by_first[:, 1] + by_first[:, 2]
        if len(hl) and (by_first[0, 1] != 0 or np.any(by_first[1:, 1] != ends[:-1])):
            raise StageMismatch("hlist", where + "the runs' item ranges do not tile [0, %d)" % nitems)
        if (int(ends[-1]) if len(hl) else 0) != nitems:
            raise StageMismatch("hctr", where + "%d chunk items counted, the runs hold %d" % (nitems, int(ends[-1]) if len(hl) else 0))
        hi = np.asarray(dump["hitems"][g]).astype(np.int64).reshape(-1, 2)
        if len(hi) != nitems:
            raise StageMismatch("hitems", where + "%d pairs, hctr counts %d" % (len(hi), nitems))
        want = np.stack([np.repeat(by_first[:, 0], by_first[:, 2]),
                         np.arange(nitems) - np.repeat(by_first[:, 1], by_first[:, 2])], axis=1)
        if np.any(hi != want):
            p = _first((hi != want).any(axis=1))
            raise StageMismatch("hitems", where + "item %d is (%d, %d), its run says (%d, %d)" % (p, hi[p, 0], hi[p, 1], want[p, 0], want[p, 1]))
        big = int(np.count_nonzero(counts.reshape(-1, 1 << h["LB"]).sum(axis=1) > h["PART_BIG"])) if h["big_on"] else 0
        if int(hctr[8 + g]) != big:
            raise StageMismatch("hctr", where + "%d super-buckets left to the sliced pass B, %d hold more than %d entries"
                                % (hctr[8 + g], big, h["PART_BIG"]))
    return m


def same_buckets(a, b):
    """Two dumps of the same scalars under different knobs hold the same multiset in every bucket: (window, bucket, entry) triples,
    whatever the slot order, the window groups and the order inside a bucket"""
    def triples(d):
        h = d["header"]
        out = []
        for g, G in enumerate(h["groups"]):
            off = np.asarray(d["offsets"][g]).astype(np.int64)
            slot = np.repeat(np.arange(G["nslots"], dtype=np.int64), np.diff(off))
            bucket = slot_to_bucket(slot, h["HB"], h["LB"]) + (G["w0"] << (h["c"] - 1))
            out.append((bucket.astype(np.uint64) << np.uint64(32)) | np.asarray(d["sorted"][g])[:off[-1]].astype(np.uint64))
        t = np.concatenate(out)
        t.sort()
        return t
    ta, tb = triples(a), triples(b)
    if ta.shape != tb.shape or np.any(ta != tb):
        raise StageMismatch("sorted", "the two runs do not hold the same entries per bucket")


# ---- the hooks ------------------------------------------------------------------------------------------------------------
def _knob_record(knobs):
    bad = set(knobs) - set(KNOBS)
    assert not bad, bad
    k = dict(KNOB_DEFAULTS, **knobs)
    return (C.c_int32 * 8)(*[int(k[name]) for name in KNOBS])


def sort_geometry(curve, n, c, W=0, narrow=0, shared=False, **knobs):
    """ark_hip_test_msm_sort_geometry (host only) as a dict"""
    from algebra_amd import _lib
    out = (C.c_uint64 * 32)()
    rc = _lib.test_lib().ark_hip_test_msm_sort_geometry(CURVES.index(curve), n, c, W, narrow, int(shared), _knob_record(knobs), out)
    assert rc == 0, rc
    return dict(zip(GEOMETRY, [int(x) for x in out]))


def gpu_dump(curve, scalars, mont=0, sbytes=0, sbits=0, **knobs):
    """ark_hip_test_msm_sort_stages: a header-only call sizes the arrays, the second call fills them"""
    from algebra_amd import _lib
    T = _lib.test_lib()
    scalars = np.ascontiguousarray(scalars)
    n = len(scalars)
    rec, hdr = _knob_record(knobs), (C.c_uint64 * 32)()
    args = (CURVES.index(curve), scalars.ctypes.data_as(C.c_void_p), 0, n, mont, sbytes, sbits, rec, hdr)
    rc = T.ark_hip_test_msm_sort_stages(*args, None, None)
    assert rc == 0, rc
    h = dict(zip(HEADER, [int(x) for x in hdr]))
    h["groups"] = [dict(zip(("w0", "Wg", "nslots", "nbk_g"), [int(x) for x in hdr[24 + 4 * g:28 + 4 * g]])) for g in range(h["ngroups"])]
    assert h["n"] == n
    W, nc, nb = h["W"], h["n_carried"], h["W"] << (h["c"] - 1)
    sizes = [W * nc, nc, nc * 8, W * nc, nb + h["ngroups"], nb, 16, 3 * h["max_heavy"], 2 * h["max_items"]]
    arrays = [np.zeros(max(s, 1), dtype=np.uint32) for s in sizes]
    ptrs = (C.c_void_p * 9)(*[a.ctypes.data for a in arrays])
    caps = (C.c_size_t * 9)(*sizes)
    rc = T.ark_hip_test_msm_sort_stages(*args, ptrs, caps)
    assert rc == 0, rc
    h2 = [int(x) for x in hdr]
    assert [h2[k] for k in range(len(HEADER))] == [h[name] for name in HEADER], "the two calls planned differently"
    keys, cidx, cscal, srt, off, order, hctr, hlist, hitems = arrays
    B = h["c"] - 1
    d = dict(header=h, keys=keys[:W * nc].reshape(W, nc), hctr=hctr, sorted=[], offsets=[], order=[], hlist=[], hitems=[])
    if h["compacted"]:
        d["cidx"], d["cscal"] = cidx[:nc], cscal[:nc * 8].reshape(nc, 8)
    e0 = i0 = 0
    for g, G in enumerate(h["groups"]):
        s0 = G["w0"] << B
        d["sorted"].append(srt[G["w0"] * nc:(G["w0"] + G["Wg"]) * nc])
        d["offsets"].append(off[s0 + g:s0 + g + G["nslots"] + 1])
        d["order"].append(order[s0:s0 + G["nbk_g"]])
        ni, ne = int(hctr[4 * g]), int(hctr[4 * g + 1])
        d["hlist"].append(hlist[3 * e0:3 * (e0 + ne)].reshape(-1, 3))
        d["hitems"].append(hitems[2 * i0:2 * (i0 + ni)].reshape(-1, 2))
        e0, i0 = e0 + ne, i0 + ni
    return d
