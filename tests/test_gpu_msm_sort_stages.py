"""The MSM's integer stages on the device, stage by stage: zero-scalar compaction (K0c), signed-digit recoding (K1 / K1n), the
two-pass partition sort with its sliced pass B (csrc/msm_sort.cuh), the bucket order pass (K3b) and the heavy-run list
(msm_find_heavy_kernel) -- dumped by ark_hip_test_msm_sort_stages, which runs the stage functions msm_enqueue runs, and checked
array by array against the exact reference of tests/msm_sort_ref.py (Python ints for the fold, numpy for the counting sort: no
tolerance anywhere).  Every case asserts from the dump's header and counters that the regime it is named for was reached.
tests/test_msm_sort_host.py shows, without a GPU, that the checker rejects every single wrong word these arrays can hold."""
import random

import numpy as np
import pytest

import msm_sort_ref as R

pytestmark = pytest.mark.gpu

CURVE = "BLS12_381_G1"
FIELD = R.SCALAR_FIELD[CURVE]


# ---- scalars ---------------------------------------------------------------------------------------------------------------
def uniform(field, n, seed):
    """n scalars below r as (n, 4) uint64 limbs; below 2^(bits - 1) < r for the large sets (numpy), any residue for the small"""
    r, bits = R.field_modulus(field)
    if n <= 16384:
        rng = random.Random(seed)
        return R.ints_to_limbs([rng.randrange(r) for _ in range(n)])
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << (bits - 1 - 192)) - 1)
    return a


def edges(field, c, W, narrow, out_of_range):
    r, bits = R.field_modulus(field)
    chain, off = 0, 0
    for cw in R.window_widths(c, W, narrow):   # every window exactly half: the carry chain
        chain |= (1 << (cw - 1)) << off
        off += cw
    chain %= r
    vals = [0, 1, r - 1, (r - 1) // 2, (r + 1) // 2, chain, chain - 1, chain + 1, r - chain, 2, r - 2]
    if out_of_range is not None:
        vals += [r, r + 1, (1 << bits) - 1]          # s in [r, 2^bits): s - r
        if out_of_range:
            vals += [1 << bits]
    return vals


def witness_like(field, n, seed):
    """60 % zeros, 30 % ones, 5 % minus ones, 5 % full width, in exact shares, shuffled; scalar 3 is r itself (zero mod r)"""
    r, _ = R.field_modulus(field)
    a = np.zeros((n, 4), dtype=np.uint64)
    n1, nm, nf = n * 30 // 100, n * 5 // 100, n * 5 // 100
    a[:n1, 0] = 1
    a[n1:n1 + nm] = R.ints_to_limbs([r - 1])[0]
    a[n1 + nm:n1 + nm + nf] = uniform(field, max(nf, 16385), seed)[:nf]
    a = a[np.random.default_rng(seed).permutation(n)]
    a[3] = R.ints_to_limbs([r])[0]
    return a


def run(curve, scalars, mont=0, sbytes=0, sbits=0, folded=None, **knobs):
    """one hook call, checked in full; returns (dump, header, model)"""
    d = R.gpu_dump(curve, scalars, mont, sbytes, sbits, **knobs)
    m = R.check_dump(scalars, d, R.SCALAR_FIELD[curve], mont, sbytes, sbits, heavy=knobs.get("heavy", 0), folded=folded)
    h = d["header"]
    assert (h["HEAVY_CHUNK"], h["PART_BIG"], h["SCAN_SMALL_MAX"]) == (1024, 1 << 17, 16384)
    assert h["ntiles"] == -(-h["n_carried"] // h["tile"]) and h["nthist"] == (h["W"] << h["HB"]) * h["ntiles"]
    return d, h, m


def super_bucket_totals(h, m, g=0):
    return m.counts[g].reshape(-1, 1 << h["LB"]).sum(axis=1)


# ---- every curve's scalar field ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 8191, 8193])
@pytest.mark.parametrize("curve", ["BN254_G1", "BLS12_381_G1", "BLS12_377_G1"])
def test_uniform_scalars(curve, n, mont):
    d, h, m = run(curve, uniform(R.SCALAR_FIELD[curve], n, n + mont), mont)
    assert (h["n"], h["n_carried"], h["compacted"], h["ngroups"], h["big_on"]) == (n, n, 0, 1, 0)
    assert h["ntiles"] == (2 if n > 8192 else 1) and h["tile"] == 8192
    assert d["hctr"][3] == 0


@pytest.mark.parametrize("mont", [0, 1])
@pytest.mark.parametrize("curve", ["BN254_G1", "BLS12_381_G1", "BLS12_377_G1"])
def test_edge_values(curve, mont):
    import pyref
    field = R.SCALAR_FIELD[curve]
    r, bits = R.field_modulus(field)
    n = 257
    h0 = R.gpu_dump(curve, uniform(field, n, 1))["header"]   # (the plan depends on n alone here)
    vals = edges(field, h0["c"], h0["W"], h0["narrow"], None if mont else False)
    if mont:
        vals = [v * pyref.R_of(r) % r for v in vals]
    s = uniform(field, n, 2)
    s[5:5 + len(vals)] = R.ints_to_limbs(vals)
    d, h, m = run(curve, s, mont)
    assert (h["c"], h["W"], h["narrow"]) == (h0["c"], h0["W"], h0["narrow"])
    assert d["hctr"][3] == 0 and m.zeros == (1 if mont else 2)   # 0 (and r): no key in any window
    assert (d["keys"][:, 5] == R.KEY_NONE).all()


@pytest.mark.parametrize("curve", ["BN254_G1", "BLS12_381_G1", "BLS12_377_G1"])
def test_out_of_range_scalar_sets_the_flag(curve):
    field = R.SCALAR_FIELD[curve]
    r, bits = R.field_modulus(field)
    s = uniform(field, 257, 3)
    s[100] = R.ints_to_limbs([1 << bits])[0]
    d, h, m = run(curve, s)
    assert m.out_of_range and d["hctr"][3] == 1
    assert (d["keys"][:, 100] == R.KEY_NONE).all()   # it counts as zero
    s[100] = R.ints_to_limbs([(1 << bits) - 1])[0]   # the largest accepted word: s - r, no flag
    d, h, m = run(curve, s)
    assert d["hctr"][3] == 0


# ---- window sweep ----------------------------------------------------------------------------------------------------------
SPLITS = {3: (0, 2), 11: (0, 10), 12: (1, 10), 14: (3, 10), 20: (9, 10), 21: (9, 11), 22: (9, 12), 23: (10, 12)}


@pytest.fixture(scope="module")
def sweep_scalars():
    s = uniform(FIELD, 4099, 7)
    return s, R.fold_scalars(s, FIELD)


@pytest.mark.parametrize("c", range(3, 24))
def test_window_sweep(sweep_scalars, c):
    s, folded = sweep_scalars
    d, h, m = run(CURVE, s, folded=folded, c=c)
    assert (h["c"], h["W"], h["narrow"]) == (c,) + R.layout(c, 255)
    assert h["HB"] + h["LB"] == c - 1 and h["LB"] <= 12
    if c in SPLITS:
        assert (h["HB"], h["LB"]) == SPLITS[c]
    if c <= 11:
        assert h["HB"] == 0           # few buckets, few scalars: pass A does not split at all
    cells = {3: (85, 0), 18: (15, 15), 20: (13, 5), 21: (13, 0), 23: (12, 0)}   # exact, every window narrow, some, uniform, uniform
    if c in cells:
        assert (h["W"], h["narrow"]) == cells[c]
    g = R.sort_geometry(CURVE, 4099, c)
    assert (h["HB"], h["LB"], h["stage_cap"], h["noblk"]) == (g["HB"], g["LB"], g["stage_cap"], g["noblk"])
    if c >= 15:
        assert h["noblk"] * 256 > h["SCAN_SMALL_MAX"]     # the order pass's scan runs as three kernels
    if c <= 13:
        assert h["noblk"] * 256 <= h["SCAN_SMALL_MAX"] and h["nthist"] <= h["SCAN_SMALL_MAX"]   # ... and here as one workgroup


@pytest.mark.parametrize("c,hb", [(21, 8), (13, 12), (16, 3)])
def test_forced_split(sweep_scalars, c, hb):
    """hb forced to B - 12 (LB = 12) and to B (LB = 0: every bucket its own super-bucket), and inside the range"""
    s, folded = sweep_scalars
    d, h, m = run(CURVE, s, folded=folded, c=c, hb=hb)
    assert (h["c"], h["HB"], h["LB"]) == (c, hb, c - 1 - hb)


# ---- tiles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ntiles", [(11 * 8192 - 5, 11), (8 * 8192, 8), (8 * 8192 + 1, 9)])
def test_tile_edges(n, ntiles):
    """11 tiles: eight go through part_tile_of_block's XCD permutation, three do not, and the last is ragged"""
    d, h, m = run(CURVE, uniform(FIELD, n, n), c=12)
    assert (h["tile"], h["ntiles"]) == (8192, ntiles)


def test_three_kernel_scan_in_pass_a():
    n = (1 << 17) + 77
    d, h, m = run(CURVE, uniform(FIELD, n, 5), c=16, hb=7)
    assert h["ntiles"] == 17 and h["nthist"] == (16 << 7) * 17 > h["SCAN_SMALL_MAX"]


# ---- long runs: direct placement, heavy list ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_valued():
    r, _ = R.field_modulus(FIELD)
    n = 1 << 16
    rng = random.Random(11)
    a, b = rng.randrange(r), rng.randrange(r)
    pick = np.random.default_rng(11).random(n)
    s = uniform(FIELD, n, 12)
    s[pick < 0.88] = R.ints_to_limbs([a])[0]
    s[(pick >= 0.88) & (pick < 0.98)] = R.ints_to_limbs([b])[0]
    return s, R.fold_scalars(s, FIELD)


def test_direct_placement_all_equal():
    r, _ = R.field_modulus(FIELD)
    n = 1 << 16
    s = np.tile(R.ints_to_limbs([random.Random(9).randrange(r)]), (n, 1))
    d, h, m = run(CURVE, s)
    assert h["big_on"] == 0 and d["hctr"][8] == 0
    assert super_bucket_totals(h, m).max() == n > h["stage_cap"]        # placed directly, not staged in LDS
    assert d["hctr"][1] == h["W"] and (d["hlist"][0][:, 2] == n // 1024).all()   # one run per window, 64 chunks each


@pytest.mark.parametrize("heavy", [0, 64, 10000])
def test_direct_placement_two_valued(two_valued, heavy):
    s, folded = two_valued
    d, h, m = run(CURVE, s, folded=folded, heavy=heavy)
    assert h["big_on"] == 0 and d["hctr"][8] == 0
    tot = super_bucket_totals(h, m)
    assert (tot > h["stage_cap"]).any() and ((tot > 0) & (tot <= h["stage_cap"])).any()   # both placements in one launch
    # computed: 22 windows x 2^16 entries in 22 x 2^11 slots -- 4 x the mean run of 31, above the floor of 64
    assert h["groups"][0]["nslots"] == 22 << 11 and d["hctr"][2] == (heavy if heavy else 124)
    items = d["hlist"][0][:, 2]
    assert (items > 16).any()                    # chunk items written by the whole wave
    if heavy < 10000:
        assert (items <= 16).any()               # ... and by the run's own lane
    else:
        assert len(items) == h["W"]              # only the 88 % runs are above a threshold of 10000


# ---- sliced pass B -----------------------------------------------------------------------------------------------------------
def test_sliced_pass_b():
    """Witness-like scalars put 35 % of n (ones and minus ones) into bucket 0 of window 0: more than PART_BIG entries from
    n = 3 x 2^17 + 4099 on (at 2^18 + 4099 that bucket holds 93 000, below the 2^17 the slices start at).  The probe is off, so the
    zeros stay in the pipeline."""
    n = 3 * (1 << 17) + 4099
    s = witness_like(FIELD, n, 21)
    folded = R.fold_scalars(s, FIELD)
    d, h, m = run(CURVE, s, folded=folded, probe=0, c=13)
    assert (h["big_on"], h["compacted"], h["n_carried"], h["ngroups"]) == (1, 0, n, 1)
    assert d["hctr"][8] >= 1 and super_bucket_totals(h, m).max() > h["PART_BIG"]
    d0, h0, m0 = run(CURVE, s, folded=folded, probe=0, c=13, big_slices=0)
    assert h0["big_on"] == 0 and d0["hctr"][8] == 0
    R.same_buckets(d, d0)


# ---- compaction ------------------------------------------------------------------------------------------------------------
def test_compaction():
    n = 1 << 19
    s = witness_like(FIELD, n, 22)
    folded = R.fold_scalars(s, FIELD)
    d, h, m = run(CURVE, s, folded=folded)
    assert h["compacted"] == 1 and h["n_carried"] == n - m.zeros and m.zeros >= n - (n * 30 // 100 + 2 * (n * 5 // 100))
    assert 3 not in d["cidx"][:8]                  # scalar 3 is r: zero mod r
    assert h["big_on"] == 0                        # 210 000 scalars are carried
    d0, h0, m0 = run(CURVE, s, folded=folded, compact=0)
    assert (h0["compacted"], h0["n_carried"], h0["big_on"]) == (0, n, 1)
    assert (h0["c"], h0["W"]) == (h["c"], h["W"])
    R.same_buckets(d, d0)


# ---- two window groups -------------------------------------------------------------------------------------------------------
def test_two_window_groups():
    n = 1 << 19
    s = uniform(FIELD, n, 23)
    folded = R.fold_scalars(s, FIELD)
    d, h, m = run(CURVE, s, folded=folded, groups=2)
    assert h["ngroups"] == 2 and len(d["offsets"]) == 2
    g0, g1 = h["groups"]
    assert (g0["w0"], g0["Wg"], g1["w0"], g1["Wg"]) == (0, (h["W"] + 1) // 2, (h["W"] + 1) // 2, h["W"] // 2)
    assert d["offsets"][1][0] == 0 and d["offsets"][1][-1] == m.counts[1].sum() > 0    # relative to its own `sorted` base
    d1, h1, m1 = run(CURVE, s, folded=folded, groups=1)
    assert h1["ngroups"] == 1 and (h1["c"], h1["W"]) == (h["c"], h["W"])
    R.same_buckets(d, d1)


# ---- narrow entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sbytes,sbits", [(1, 1), (1, 8), (2, 16), (4, 32), (8, 64), (8, 40)])
def test_narrow_scalars(sbytes, sbits):
    n = 70001
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[sbytes]
    s = np.random.default_rng(sbits).integers(0, 1 << (8 * sbytes), size=n, dtype=np.uint64).astype(dtype)
    s[:4] = [0, 1, (1 << sbits) - 1 if sbits < 8 * sbytes else np.iinfo(dtype).max, 1 << (sbits - 1)]
    d, h, m = run(CURVE, s, sbytes=sbytes, sbits=sbits)
    assert h["W"] * h["c"] - h["narrow"] >= sbits + 1 and (h["compacted"], h["ngroups"]) == (0, 1)
    if sbits <= 8:
        assert h["c"] - 1 <= 10 and h["HB"] == 2      # B <= 10: HB = log2(n) - 15, from n alone
        nslots = h["groups"][0]["nslots"]
        assert nslots < 32768 and d["hctr"][2] == 64 and d["hctr"][1] > 0   # long runs, no 4 x mean term in the threshold
        assert m.counts[0].sum() // nslots * 4 > 64
