"""The MSM's integer stages without a GPU:
  * the geometry of the partition sort (csrc/msm_plan.hpp: msm_sort_geometry, msm_part_split, msm_heavy_geometry, through
    ark_hip_test_msm_sort_geometry) over every curve, window size and size class, against the identities the kernels rely on;
  * the reference of tests/msm_sort_ref.py against itself: the digit identity sum d_w 2^off_w = v and |d_w| <= 2^(cw - 1) on
    Python ints, which does not depend on how the recoding rule is restated, and the vectorised model against the scalar one;
  * the checker: check_dump accepts a dump made by a plain counting sort and rejects every single mutation of it, naming the
    array -- the evidence that tests/test_gpu_msm_sort_stages.py fails on a subtly wrong kernel."""
import ctypes as C
import random

import numpy as np
import pytest

from algebra_amd import _lib
import msm_sort_ref as R

SIZES = [1, 100, 8191, 8192, 8193, 1 << 15, 1 << 16, 1 << 18, (1 << 18) + 1, 1 << 19, 1 << 22, 1 << 24, 1 << 26, 1 << 27]
FIELDS = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]


# ---- geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", R.CURVES)
def test_sort_geometry_identities(curve):
    bits = R.field_modulus(R.SCALAR_FIELD[curve])[1]
    for c in range(3, 24):
        B = c - 1
        W, narrow = R.layout(c, bits)
        for n in SIZES:
            for hb in (-1, 0, B - 12, B):
                g = R.sort_geometry(curve, n, c, hb=hb)
                where = (curve, c, n, hb, g)
                assert (g["W"], g["narrow"]) == (W, narrow), where
                HB, LB, tile, ntiles = g["HB"], g["LB"], g["tile"], g["ntiles"]
                assert HB + LB == B and 0 <= HB and LB <= 12, where
                if 0 <= hb <= B and B - hb <= 12 and B > 10:
                    assert HB == hb, where   # the knob holds wherever the window allows it
                assert tile in (8192, 16384) and ntiles * tile >= n > (ntiles - 1) * tile, where
                assert g["nsuper"] == W << HB and g["nthist"] == g["nsuper"] * ntiles, where
                assert g["stage_cap"] == g["PART_LDS_WORDS"] - 1024 - (1 << LB) - 16, where
                assert g["lds_b"] == 4 * ((1 << LB) + 1024 + g["stage_cap"]) <= 160 * 1024 - 64, where
                assert g["lds_a"] == (8 << HB) + 8 * tile, where
                assert g["accepted"] == int(n * W < 1 << 32 and g["lds_a"] <= g["PART_SCATTER_LDS_MAX"]), where
                if hb == -1 and n * W < 1 << 32:
                    assert g["accepted"] == 1, where   # the planner's own split always fits the scatter kernel
                assert g["big_on"] == int(n > 2 * g["PART_BIG"]), where
                assert g["big_region"] == g["nsuper"] + 2 * (W << B), where
                # one scan scratch serves pass A's histogram and the order pass's: a word per SCAN_TILE cells of the larger
                nb = W << B
                assert g["noblk"] == -(-nb // g["ORDER_TILE"]) and g["nohist"] == g["noblk"] * g["ORDER_BINS"], where
                assert g["nsums"] >= max(-(-g["nthist"] // g["SCAN_TILE"]), -(-g["nohist"] // g["SCAN_TILE"])), where
                assert g["mean_load"] == n * W // nb and g["max_heavy"] == n * W // 64 + 1, where
                assert g["max_items"] == n * W // g["HEAVY_CHUNK"] + g["max_heavy"] + 1, where


def test_sort_geometry_documented_cells():
    g = R.sort_geometry("BLS12_381_G1", 1 << 24, 20)
    assert (g["HB"], g["LB"], g["tile"]) == (9, 10, 8192)
    g = R.sort_geometry("BLS12_381_G1", 1 << 26, 22)
    assert (g["HB"], g["LB"], g["tile"]) == (11, 10, 16384)
    g = R.sort_geometry("BLS12_381_G1", 1 << 27, 23)
    assert (g["HB"], g["tile"]) == (12, 8192)       # 32 KiB of counters + 128 KiB of pairs do not fit the scatter kernel
    assert R.sort_geometry("BLS12_381_G1", 1 << 20, 23, hb=12)["tile"] == 8192
    assert R.sort_geometry("BLS12_381_G1", 1 << 20, 23, hb=11)["tile"] == 16384
    # the constants the GPU tests' regimes are stated in
    assert (g["PART_BIG"], g["SCAN_SMALL_MAX"], g["HEAVY_CHUNK"], g["SCAN_TILE"]) == (1 << 17, 16384, 1024, 2048)
    # forced heavy threshold and window groups pass through the knob record
    assert R.sort_geometry("BLS12_381_G1", 1 << 16, 12, heavy=64)["forced_thresh"] == 64
    assert R.sort_geometry("BLS12_381_G1", 1 << 19, 16, groups=2)["ngroups"] == 2
    assert R.sort_geometry("BLS12_381_G1", 1 << 19, 16)["ngroups"] == 1
    assert R.sort_geometry("BLS12_381_G1", (1 << 19) - 1, 16, groups=2)["ngroups"] == 1


def test_sort_geometry_hook_rejects_bad_arguments():
    T = _lib.test_lib()
    out, rec = (C.c_uint64 * 32)(), (C.c_int32 * 8)(0, -1, 0, 0, 0, 1, 1, 1)
    assert T.ark_hip_test_msm_sort_geometry(1, 100, 12, 0, 0, 0, rec, out) == 0
    assert T.ark_hip_test_msm_sort_geometry(5, 100, 12, 0, 0, 0, rec, out) != 0
    assert T.ark_hip_test_msm_sort_geometry(1, 0, 12, 0, 0, 0, rec, out) != 0
    assert T.ark_hip_test_msm_sort_geometry(1, 100, 2, 0, 0, 0, rec, out) != 0
    assert T.ark_hip_test_msm_sort_geometry(1, 100, 12, 22, 23, 0, rec, out) != 0
    assert T.ark_hip_test_msm_sort_geometry(1, 100, 12, 0, 0, 0, None, out) != 0
    assert T.ark_hip_test_msm_sort_geometry(1, 100, 12, 0, 0, 0, rec, None) != 0


# ---- the model against itself ----------------------------------------------------------------------------------------------
def edge_values(r, bits, c, W, narrow):
    """the values at which the fold and the carry rule change their answer, as 256-bit words"""
    vals = [0, 1, r - 1, r, r + 1, (r - 1) // 2, (r + 1) // 2, (1 << bits) - 1, 1 << bits, (1 << 256) - 1]
    # every window exactly `half`: each carries into the next -- the longest carry chain (and its neighbours)
    chain, off = 0, 0
    for cw in R.window_widths(c, W, narrow):
        chain |= (1 << (cw - 1)) << off
        off += cw
    chain %= r
    vals += [chain, chain - 1, chain + 1, r - chain, (chain >> 1) % r]
    return vals


def scalar_set(field, c, W, narrow, count, seed):
    r, bits = R.field_modulus(field)
    rng = random.Random(seed)
    vals = edge_values(r, bits, c, W, narrow)
    vals += [rng.randrange(r) for _ in range(count - len(vals))]
    return vals


@pytest.mark.parametrize("field", FIELDS)
def test_digit_identity_full_width(field):
    r, bits = R.field_modulus(field)
    for c in range(3, 24):
        W, narrow = R.layout(c, bits)
        widths = R.window_widths(c, W, narrow)
        assert sum(widths) >= bits and len(widths) == W
        offs = np.concatenate([[0], np.cumsum(widths)[:-1]]).tolist()
        vals = scalar_set(field, c, W, narrow, 2000, c)
        folded = [R.magnitude(s, r, bits) for s in vals]
        for s, (v, flip, bad) in zip(vals, folded):
            assert bad == (s >= 1 << bits)
            t = 0 if bad else s % r
            assert v == min(t, r - t) and flip == int(r - t < t), (field, hex(s))
            d = R.digits(v, c, W, narrow)
            assert sum(dw << o for dw, o in zip(d, offs)) == v, (field, c, hex(s))
            assert all(abs(dw) <= 1 << (cw - 1) for dw, cw in zip(d, widths)), (field, c, hex(s))
            assert d[-1] >= 0
        # the vectorised model is the scalar one
        limbs = R.ints_to_limbs(vals)
        v, flip, bad = R.fold_scalars(limbs, field)
        assert bad and R.scalars_to_ints(v) == [f[0] for f in folded] and flip.tolist() == [f[1] for f in folded]
        keys = R.model_keys(v, flip, c, W, narrow)
        want = [[R.key_of(dw, f[1]) for dw in R.digits(f[0], c, W, narrow)] for f in folded]
        assert keys.T.tolist() == want, (field, c)


def test_fold_from_montgomery_form():
    import pyref
    for field in FIELDS:
        r, bits = R.field_modulus(field)
        vals = [0, 1, r - 1, (r - 1) // 2, (r + 1) // 2, 12345678901234567890 % r]
        mont = R.ints_to_limbs([x * pyref.R_of(r) % r for x in vals])
        v, flip, bad = R.fold_scalars(mont, field, mont=1)
        v0, flip0, _ = R.fold_scalars(R.ints_to_limbs(vals), field)
        assert not bad and np.array_equal(v, v0) and np.array_equal(flip, flip0)
        assert [R.magnitude(int(x), r, bits, 1)[:2] for x in R.scalars_to_ints(mont)] == list(zip(R.scalars_to_ints(v0), flip0.tolist()))


@pytest.mark.parametrize("sbits", [1, 8, 16, 32, 64])
def test_digit_identity_narrow_scalars(sbits):
    """K1n: no fold, masked to sbits; the layout covers sbits + 1 bits, so the top window keeps a spare bit"""
    rng = random.Random(sbits)
    top = (1 << sbits) - 1
    vals = [0, 1, top, top - 1, top >> 1, (top >> 1) + 1] + [rng.randrange(top + 1) for _ in range(300)]
    dtype = {1: np.uint8, 8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}[sbits]
    for c in range(3, 24):
        W, narrow = R.layout(c, sbits + 1)
        widths = R.window_widths(c, W, narrow)
        assert sum(widths) >= sbits + 1
        offs = np.concatenate([[0], np.cumsum(widths)[:-1]]).tolist()
        arr = np.array(vals, dtype=dtype)
        # bits above sbits do not exist: garbage there changes nothing
        if sbits == 1:
            arr = arr | np.uint8(0xA0)
        v, flip, bad = R.fold_scalars(arr, None, sbytes=arr.itemsize, sbits=sbits)
        assert not bad and not flip.any() and v[:, 0].tolist() == vals
        keys = R.model_keys(v, flip, c, W, narrow)
        for i, x in enumerate(vals):
            d = R.digits(x, c, W, narrow)
            assert sum(dw << o for dw, o in zip(d, offs)) == x
            assert all(abs(dw) <= 1 << (cw - 1) for dw, cw in zip(d, widths))
            assert keys[:, i].tolist() == [R.key_of(dw, 0) for dw in d]


def test_slot_map_is_a_bijection():
    for HB, LB in ((0, 2), (0, 10), (3, 7), (9, 10), (10, 12), (12, 10)):
        B = HB + LB
        b = np.arange(1 << B, dtype=np.int64)
        for wl in (0, 3):
            slot = R.slot_of_bucket(wl, b, HB, LB)
            assert np.array_equal(np.sort(slot), (wl << B) + b)
            assert np.array_equal(R.slot_to_bucket(slot, HB, LB), (wl << B) | b)
            assert np.array_equal(slot >> LB, (wl << HB) | (b & ((1 << HB) - 1)))   # the super-bucket: the low HB bits


# ---- the checker catches what it must -----------------------------------------------------------------------------------------
FIELD = "BLS12_381_FR"


def skewed_scalars(n, seed, zeros=0.0):
    """uniform scalars with two values repeated often enough to make heavy runs, optionally a share of zeros, and one scalar = r"""
    r, bits = R.field_modulus(FIELD)
    rng = random.Random(seed)
    a, b = rng.randrange(r), rng.randrange(r)
    vals = []
    for _ in range(n):
        u = rng.random()
        vals.append(0 if u < zeros else a if u < zeros + 0.3 else b if u < zeros + 0.4 else rng.randrange(r))
    vals[7] = r   # zero mod r
    return R.ints_to_limbs(vals)


@pytest.fixture(scope="module")
def valid():
    """scalars and a valid dump: two window groups, compaction, heavy runs of one and of several chunks, big super-buckets"""
    scalars = skewed_scalars(3000, 1, zeros=0.3)
    c = 8
    W, narrow = R.layout(c, 255)
    header = R.make_header(len(scalars), c, W, narrow, HB=3, ngroups=2, compacted=1, big_on=1, part_big=200, heavy_chunk_words=256)
    dump = R.build_dump(scalars, FIELD, header)
    return scalars, dump


def clone(dump):
    out = dict(dump)
    for k, v in dump.items():
        out[k] = [a.copy() for a in v] if isinstance(v, list) else v.copy() if isinstance(v, np.ndarray) else dict(v)
    return out


def test_checker_accepts_a_counting_sort(valid):
    scalars, dump = valid
    m = R.check_dump(scalars, dump, FIELD)
    h = dump["header"]
    assert h["compacted"] and h["n_carried"] == 3000 - m.zeros and m.zeros > 800
    # the dump has what the mutations below need
    for g in range(2):
        assert dump["hctr"][4 * g + 1] >= 2 and dump["hctr"][8 + g] >= 1
        assert (dump["hlist"][g][:, 2] > 1).any()
    # ... and without compaction, with one group and with two, with a forced threshold
    for kw in (dict(), dict(ngroups=2), dict(heavy=100)):
        hd = R.make_header(3000, 8, h["W"], h["narrow"], HB=0, ngroups=kw.get("ngroups", 1))
        d = R.build_dump(scalars, FIELD, hd, heavy=kw.get("heavy", 0))
        R.check_dump(scalars, d, FIELD, heavy=kw.get("heavy", 0))
        if kw.get("heavy"):
            assert d["hctr"][2] == 100
            with pytest.raises(R.StageMismatch, match="^hctr: .*threshold"):
                R.check_dump(scalars, d, FIELD)


def heavy_run(dump, g):
    """(position in hlist, slot) of a run of group g with more than one chunk"""
    p = int(np.flatnonzero(dump["hlist"][g][:, 2] > 1)[0])
    return p, int(dump["hlist"][g][p, 0])


def mut_swap_across_buckets(d, g):
    off = d["offsets"][g].astype(np.int64)
    s = int(np.flatnonzero((np.diff(off)[:-1] > 0) & (np.diff(off)[1:] > 0))[0])   # two neighbouring non-empty buckets
    i, j = off[s + 1] - 1, off[s + 1]
    assert d["sorted"][g][i] != d["sorted"][g][j]
    d["sorted"][g][[i, j]] = d["sorted"][g][[j, i]]


def mut_sign(d, g):
    d["sorted"][g][5] ^= np.uint32(0x80000000)


def mut_index(d, g):
    srt = d["sorted"][g]
    srt[9] = (srt[9] & np.uint32(0x80000000)) | (srt[10] & np.uint32(0x7FFFFFFF))


def mut_offset(d, g):
    off = d["offsets"][g]
    s = int(np.flatnonzero(np.diff(off.astype(np.int64)) > 1)[0])
    off[s + 1] -= 1


def mut_sentinel(d, g):
    d["offsets"][g][-1] += 1


def mut_order_dup(d, g):
    d["order"][g][3] = d["order"][g][4]


def mut_order_swap(d, g):
    h = d["header"]
    cls = np.minimum(np.diff(d["offsets"][g].astype(np.int64)) >> h["shift"], 255)[d["order"][g]]
    assert cls[0] != cls[-1]
    d["order"][g][[0, -1]] = d["order"][g][[-1, 0]]


def mut_heavy_drop(d, g):
    d["hlist"][g] = d["hlist"][g][:-1]
    d["hctr"][4 * g + 1] -= 1


def mut_heavy_dup(d, g):
    d["hlist"][g] = np.concatenate([d["hlist"][g], d["hlist"][g][:1]])
    d["hctr"][4 * g + 1] += 1


def mut_items(d, g):
    p, _ = heavy_run(d, g)
    d["hlist"][g][p, 2] -= 1


def mut_hitems(d, g):
    p, _ = heavy_run(d, g)
    d["hitems"][g][d["hlist"][g][p, 1] + 1, 1] = 0


def mut_cidx(d, g):
    d["cidx"][[20, 21]] = d["cidx"][[21, 20]]


def mut_key_sign(d, g):
    w = d["header"]["groups"][g]["w0"]
    i = int(np.flatnonzero(d["keys"][w] != R.KEY_NONE)[0])
    d["keys"][w, i] ^= np.uint32(0x80000000)


def mut_big(d, g):
    d["hctr"][8 + g] += 1


def mut_past_the_end(d, g):
    d["sorted"][g][-1] = 17


def mut_range_flag(d, g):
    d["hctr"][3] ^= 1


def mut_cscal(d, g):
    d["cscal"][30, 0] ^= 1


MUTATIONS = [
    (mut_swap_across_buckets, "sorted"), (mut_sign, "sorted"), (mut_index, "sorted"), (mut_past_the_end, "sorted"),
    (mut_offset, "offsets"), (mut_sentinel, "offsets"),
    (mut_order_dup, "order"), (mut_order_swap, "order"),
    (mut_heavy_drop, "hlist"), (mut_heavy_dup, "hlist"), (mut_items, "hlist"), (mut_hitems, "hitems"),
    (mut_cidx, "cidx"), (mut_cscal, "cscal"), (mut_key_sign, "keys"), (mut_big, "hctr"), (mut_range_flag, "hctr"),
]


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("mutate,array", MUTATIONS, ids=[m.__name__[4:] for m, _ in MUTATIONS])
def test_checker_rejects_one_mutation(valid, mutate, array, g):
    scalars, dump = valid
    d = clone(dump)
    mutate(d, g)
    with pytest.raises(R.StageMismatch) as e:
        R.check_dump(scalars, d, FIELD)
    assert e.value.array == array and str(e.value).startswith(array + ": "), str(e.value)


def test_checker_sees_a_group_that_starts_one_word_off(valid):
    """group 1's offsets read one word early: the first word then holds group 0's sentinel, not 0"""
    scalars, dump = valid
    d = clone(dump)
    d["offsets"][1] = np.concatenate([d["offsets"][0][-1:], d["offsets"][1][:-1]])
    with pytest.raises(R.StageMismatch, match="^offsets: group 1"):
        R.check_dump(scalars, d, FIELD)


def test_same_buckets_across_layouts(valid):
    scalars, dump = valid
    h = dump["header"]
    other = R.build_dump(scalars, FIELD, R.make_header(3000, 8, h["W"], h["narrow"], HB=7, ngroups=1, compacted=0))
    R.same_buckets(dump, other)
    mut_index(other, 0)
    with pytest.raises(R.StageMismatch, match="^sorted: "):
        R.same_buckets(dump, other)
