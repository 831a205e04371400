"""Lookup by value on the device (ark_hip_fr_lookup_device, DenseMultilinearExtension.lookup) index for index and limb for limb
against the dictionary model of tests/lookup_ref.py -- never against the code under test.  The indices are first occurrences and
the counts are canonical Montgomery residues whatever the schedule of the atomics: no tolerance anywhere.

An element is handled as the integer its stored 32 bytes spell; the counts are encoded with sumcheck_ref.encode."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
from algebra_amd._lib import check, lib
import fraction_sum_ref as FR_REF
import lookup_ref as R
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S
import test_gpu_fraction_sum as FS       # prove_and_verify(): the layered proof against the model's verifier
import test_gpu_mle as G                 # enc(), mont_ints(): section 12's constructions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = G.FR
MLE = A.DenseMultilinearExtension
ERR_ARG = -1
GUARD = 67                               # elements behind an output that must stay as they were
TABLE_LENS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097]
NS = [0, 1, 63, 64, 65, 257, 4097]
MODES = ("indices", "counts", "both", "missing")
ints, limbs = mle_ref.ints, mle_ref.limbs


def modulus(fname):
    return pyref.MODULI[fname][0]


@functools.lru_cache(maxsize=None)
def pool(fname):
    """9000 distinct elements as integers, cached: tables take them from the front, absent values come from [8000:]"""
    v = ints(O.gen_scalars(O.FID[fname], 2600, 9000, montgomery=True))
    assert len(set(v)) == len(v)
    return tuple(v)


def witness(fname, table, n, seed, miss=0.1):
    """n cells drawn from the table, about a tenth of them replaced by values that are not in it"""
    rng = np.random.default_rng(seed)
    absent = pool(fname)[8000:]
    pick = rng.integers(0, len(table), size=n)
    out = [table[int(j)] for j in pick]
    for i in np.nonzero(rng.random(n) < miss)[0]:
        out[int(i)] = absent[int(rng.integers(0, len(absent)))]
    return out


def bytes_vec(fname, raw):
    """a DeviceVec holding the bytes `raw` (padded with 0xA5 to whole elements)"""
    raw = raw + b"\xA5" * (-len(raw) % 32)
    return A.DeviceVec.from_host(fname, np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64))


def run_entry(fname, d_table, table_len, d_values, n, mode, wait=True):
    """the raw entry into 0xFF-filled outputs with guard regions behind them -> (idx or None, counts or None, missing or None)"""
    want_idx, want_m = mode in ("indices", "both"), mode in ("counts", "both")
    pattern = O.gen_scalars(O.FID[fname], 81, GUARD, montgomery=True)
    guard = pattern.astype("<u8").tobytes()
    mbuf = bytes_vec(fname, b"\xFF" * (32 * table_len) + guard) if want_m else None
    ibuf = bytes_vec(fname, b"\xFF" * (4 * n) + guard) if want_idx else None
    missing = C.c_uint64(0xDEAD)
    ask_missing = wait or mode == "missing"
    check(lib().ark_hip_fr_lookup_device(d_table.field, d_table.ptr, table_len, d_values.ptr if n else None, n,
                                         ibuf.ptr if want_idx else None, mbuf.ptr if want_m else None,
                                         C.byref(missing) if ask_missing else None), "ark_hip_fr_lookup_device")
    if not ask_missing:
        check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
    idx = m = None
    if want_idx:
        raw = ibuf.to_host().astype("<u8").tobytes()
        idx = np.frombuffer(raw[:4 * n], dtype="<u4")
        assert raw[4 * n:4 * n + len(guard)] == guard, (mode, "the guard region behind the indices was written")
        ibuf.free()
    if want_m:
        got = mbuf.to_host()
        m = got[:table_len]
        assert np.array_equal(got[table_len:table_len + GUARD], pattern), (mode, "the guard region behind the counts was written")
        mbuf.free()
    return idx, m, (missing.value if ask_missing else None)


def check_case(fname, table, values, modes=MODES, wait=True, tag=""):
    """every mode of the raw entry on one table and witness against the model; the inputs are unchanged"""
    p = modulus(fname)
    want_idx, want_m, want_missing = R.lookup(table, values)
    assert want_missing == len(values) - sum(want_m)
    want_idx = np.array(want_idx, dtype=np.uint32)
    want_m = S.encode(want_m, p)
    ta, va = limbs(table), limbs(values if values else [0])
    dt, dv = A.DeviceVec.from_host(fname, ta), A.DeviceVec.from_host(fname, va)
    for mode in modes:
        idx, m, missing = run_entry(fname, dt, len(table), dv, len(values), mode, wait)
        where = (fname, len(table), len(values), mode, tag)
        if idx is not None:
            assert np.array_equal(idx, want_idx), (where, np.nonzero(idx != want_idx)[0][:5])
        if m is not None:
            assert np.array_equal(m, want_m), (where, np.nonzero((m != want_m).any(axis=1))[0][:5])
        if missing is not None:
            assert missing == want_missing, (where, missing, want_missing)
    assert np.array_equal(dt.to_host(), ta) and np.array_equal(dv.to_host(), va), "an input changed"
    dt.free()
    dv.free()
    return want_idx, want_m, want_missing


# ---- 1. sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("table_len", TABLE_LENS)
def test_sizes(fname, table_len):
    table = list(pool(fname)[:table_len])
    for n in NS:
        values = witness(fname, table, n, 1000 * table_len + n)
        _, _, missing = check_case(fname, table, values)
        if n >= 257:
            assert 0 < missing < n
        if n in (65, 4097):                                # the asynchronous form, then a synchronize: the same arrays
            check_case(fname, table, values, modes=("indices", "counts", "both"), wait=False)


# ---- 2. sentinels and edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_sentinels_and_edges(fname):
    p = modulus(fname)
    v = pool(fname)[7000] % (1 << 252)                     # flipping a bit below 2^252 keeps it below every modulus
    table = [pool(fname)[0], 0, p - 1, v] + list(pool(fname)[1:253]) + [pool(fname)[6000]]
    assert len(table) == 257 and len(set(table)) == 257
    near = [v ^ (1 << (32 * k)) for k in range(8)]         # one bit of word k: the other seven words are the table's
    assert all(sum(a != b for a, b in zip(R.words(x), R.words(v))) == 1 for x in near) and not set(near) & set(table)
    values = [table[0], table[-1], 0, p - 1, v] + near + [table[0], table[-1]]
    idx, _, missing = check_case(fname, table, values)
    assert list(idx[:5]) == [0, 256, 1, 2, 3] and all(i == R.MISSING for i in idx[5:13]) and missing == 8
    # a table of one value; a witness of one cell that hits the last entry, and one that misses
    check_case(fname, [p - 1], [p - 1, 0, p - 1])
    check_case(fname, table, [table[-1]])
    check_case(fname, table, [near[7]])


# ---- 3. repeated table values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_repeated_table_values(fname):
    rng = np.random.default_rng(33)
    distinct = pool(fname)[100:163]                        # 63 values repeated 2, 3, .., 64 times
    table = [v for r, v in enumerate(distinct, 2) for _ in range(r)]
    table = [table[int(i)] for i in rng.permutation(len(table))]
    assert len(table) == sum(range(2, 65))
    values = witness(fname, table, 4097, 34)
    idx, m, _ = check_case(fname, table, values)
    first = R.first_occurrence(table)
    firsts = set(first.values())
    assert len(firsts) == 63 and all(i == R.MISSING or int(i) in firsts for i in idx)
    assert not m[[j for j in range(len(table)) if j not in firsts]].any(), "a later occurrence holds a count"
    one = [pool(fname)[500]] * 1000                        # 1000 copies of one value
    idx, m, missing = check_case(fname, one, witness(fname, one, 4097, 35))
    assert set(idx.tolist()) == {0, R.MISSING} and not m[1:].any() and m[0].any() and missing > 0


# ---- 4. hot cells ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_hot_cells(fname):
    n = 4097
    table = list(pool(fname)[:1000])
    absent = pool(fname)[8000:]
    rng = np.random.default_rng(44)
    mix = [table[int(j)] for j in np.where(rng.random(n) < 0.5, rng.integers(0, 256, size=n), rng.integers(0, 1000, size=n))]
    cases = {
        "all equal, entry 0": [table[0]] * n,
        "all equal, the last entry": [table[-1]] * n,
        "all missing": [absent[i % len(absent)] for i in range(n)],
        "all missing, one value": [absent[3]] * n,
        "witness-like mix": mix,
        "only the last cell hits": [absent[i % len(absent)] for i in range(n - 1)] + [table[17]],
        "only the first cell hits": [table[17]] + [absent[i % len(absent)] for i in range(n - 1)],
        "only lane 63 of a full wave hits": [absent[i % len(absent)] for i in range(63)] + [table[5]] + [absent[1]] * 64,
        "two cells alternate": [table[i & 1] for i in range(n)],
        "runs of 5 equal cells": [table[(i // 5) % 1000] for i in range(n)],
    }
    for tag, values in cases.items():
        _, _, missing = check_case(fname, table, values, modes=("both", "counts"), tag=tag)
        if tag.startswith("only"):
            assert missing == len(values) - 1


# ---- 5. collision chains ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_collision_chains(fname):
    """48 of 64 table values share the home slot 2^7 - 2 of the 2^7 slots: the chain wraps past the end.  Every one is found;
    16 absent values with that home slot walk the whole chain and miss.  (tests/test_lookup_host.py finds the same elements.)"""
    T = _lib.test_lib()
    fid = O.FID[fname]
    assert A.lookup_plan(64)[0] == 7
    same = R.colliding(T, fid, fname, 7, 126, 64)
    assert len(same) == 64
    rng = np.random.default_rng(55)
    table = same[:48] + [v for v in pool(fname)[:16] if v not in same]
    assert len(table) == 64
    table = [table[int(i)] for i in rng.permutation(64)]
    values = table + same[48:] + same[:48][::-1] + same[48:]
    idx, m, missing = check_case(fname, table, values)
    assert missing == 32 and (idx[:64] == np.arange(64)).all() and (idx[64:80] == R.MISSING).all()
    # the same chain with every colliding value three times in the table
    table3 = [v for v in same[:20] for _ in range(3)] + list(pool(fname)[:4])
    assert A.lookup_plan(len(table3))[0] == 7
    table3 = [table3[int(i)] for i in rng.permutation(64)]
    check_case(fname, table3, table3 + same[48:])


# ---- 6. aliasing, 7. the asynchronous form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_a_table_looked_up_in_itself_and_the_mirror(fname):
    p = modulus(fname)
    rng = np.random.default_rng(66)
    table = [pool(fname)[int(j)] for j in rng.integers(0, 90, size=257)]       # repeated values
    want_idx, want_m, _ = R.lookup(table, table)
    assert want_idx == [table.index(v) for v in table]
    tv = A.DeviceVec.from_host(fname, limbs(table))
    for wait in (True, False):                             # d_values == d_table, through the raw entry
        idx, m, missing = run_entry(fname, tv, 257, tv, 257, "both", wait)
        assert np.array_equal(idx, np.array(want_idx, dtype=np.uint32)) and np.array_equal(m, S.encode(want_m, p))
        assert missing == (0 if wait else None)
    # the mirror: a DeviceVec, an extension and a DeviceSegment; a vector for 257 cells, an extension for 256
    mv, missing, idx = MLE.lookup(tv, tv, indices=True)
    assert isinstance(mv, A.DeviceVec) and missing == 0 and idx.dtype == np.uint32 and idx.tolist() == want_idx
    assert np.array_equal(mv.to_host(), S.encode(want_m, p))
    mv.free()
    seg = A.DeviceSegment(tv, 1, 256)
    ext = MLE.from_evaluations(fname, 6, limbs(table[10:74]))
    want = R.lookup(table[1:], table[10:74])
    mv, missing, idx = MLE.lookup(seg, ext, indices=True, wait=False)
    check(lib().ark_hip_synchronize(), "ark_hip_synchronize")
    assert isinstance(mv, MLE) and mv.num_vars == 8 and missing is None and idx.tolist() == want[0]
    assert np.array_equal(mv.to_evaluations(), S.encode(want[1], p))
    mv.free()
    want = R.lookup(table[10:74], table[1:])
    mv, missing, idx = MLE.lookup(ext, seg)
    assert isinstance(mv, MLE) and mv.num_vars == 6 and idx is None and missing == want[2] > 0
    assert np.array_equal(mv.to_evaluations(), S.encode(want[1], p))
    mv.free()
    none, missing, idx = MLE.lookup(ext, seg, multiplicities=False)
    assert none is None and idx is None and missing == want[2]
    # an output on an input is refused
    f = lib().ark_hip_fr_lookup_device
    assert f(tv.field, tv.ptr, 257, ext.evaluations.ptr, 64, None, tv.ptr, None) == ERR_ARG
    assert f(tv.field, tv.ptr, 257, ext.evaluations.ptr, 64, C.c_void_p(ext.evaluations.ptr.value + 32 * 63), None, None) == ERR_ARG
    assert np.array_equal(tv.to_host(), limbs(table))
    ext.free()
    tv.free()


# ---- 8. several workgroups -------------------------------------------------------------------------------------------------
def test_mid_size_witness_like_mix():
    fname = "BLS12_381_FR"
    p, fid = modulus(fname), O.FID[fname]
    table_len, n = 1 << 16, 1 << 18
    ta = O.gen_scalars(fid, 2680, table_len, montgomery=True)
    absent = O.gen_scalars(fid, 2681, 64, montgomery=True)
    rng = np.random.default_rng(88)
    pick = np.where(rng.random(n) < 0.5, rng.integers(0, 256, size=n), rng.integers(0, table_len, size=n))
    va = ta[pick]
    out = np.nonzero(rng.random(n) < 0.01)[0]
    va[out] = absent[rng.integers(0, 64, size=out.size)]
    want_idx, want_m, want_missing = R.lookup(ints(ta), ints(va))
    assert want_missing == out.size > 0
    tm, wv = MLE.from_evaluations(fname, 16, ta), A.DeviceVec.from_host(fname, va)
    mv, missing, idx = MLE.lookup(tm, wv, indices=True)
    assert missing == want_missing and np.array_equal(idx, np.array(want_idx, dtype=np.uint32))
    assert np.array_equal(mv.to_evaluations(), S.encode(want_m, p))
    for x in (tm, wv, mv):
        x.free()


# ---- 9. scratch ------------------------------------------------------------------------------------------------------------
def test_lookup_on_poisoned_scratch():
    """tests/lookup_scratch_child.py: the call warm, then with every scratch buffer poisoned (ark_hip_test_scratch_poison), then
    a small table after a larger table's call has left its slots behind: the model's results each time, nothing written past
    what was asked for"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lookup_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "lookup scratch ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- 10. a lookup end to end without an index array -------------------------------------------------------------------------
def test_lookup_end_to_end_from_the_values():
    """sum_i 1 / (gamma + w_i) = sum_j m_j / (gamma + t_j) with m from lookup(t, w): no index array anywhere.  Both layered
    proofs are accepted and the roots agree as fractions; with one witness cell outside the table, missing == 1 and they do not"""
    fname = "BLS12_381_FR"
    p = modulus(fname)
    t, idx, gamma, outside = FR_REF.lookup_case(p)      # tests/test_fraction_sum_host.py checks the seeds on the model
    one = G.mont_ints([1], p).reshape(-1, 4)
    g = G.enc(gamma, p)
    tm = MLE.from_evaluations(fname, 6, S.encode(t, p))
    tden = MLE.linear_combination([tm], one, g)
    tcanon = [(gamma + v) % p for v in t]
    for altered in (False, True):
        w = [t[i] for i in idx]
        if altered:
            w[77] = outside
        wm = MLE.from_evaluations(fname, 9, S.encode(w, p))
        m, missing, _ = MLE.lookup(tm, wm)
        mcanon = FR_REF.counts([int(i) for k, i in enumerate(idx) if not (altered and k == 77)], 64)
        assert missing == (1 if altered else 0) and isinstance(m, MLE) and m.num_vars == 6
        assert np.array_equal(m.to_evaluations(), S.encode(mcanon, p))
        _, (pt, qt) = FS.prove_and_verify(fname, m, tden, mcanon, tcanon)
        wden = MLE.linear_combination([wm], one, g)
        wcanon = [(gamma + v) % p for v in w]
        _, (pw, qw) = FS.prove_and_verify(fname, None, wden, None, wcanon)
        assert (pw * qt % p == pt * qw % p) == (not altered), altered
        for x in (wm, m, wden):
            x.free()
    for x in (tm, tden):
        x.free()


def test_three_column_lookup_end_to_end():
    """three columns on both sides, compressed with theta by linear_combination BEFORE the join: t_j = T0 + theta T1 +
    theta^2 T2 and the same for the witness rows, then m = lookup(t, w) and the two fractional sums"""
    fname = "BLS12_381_FR"
    p = modulus(fname)
    t0, idx, gamma, outside = FR_REF.lookup_case(p)
    rng = np.random.default_rng(FR_REF.LOOKUP_SEEDS[2] + 1)
    draw = lambda: int.from_bytes(rng.bytes(40), "little") % p   # noqa: E731
    cols = [t0, [draw() for _ in range(64)], [draw() for _ in range(64)]]
    theta = draw()
    coeffs = G.mont_ints([1, theta, theta * theta], p).reshape(-1, 4)
    one = G.mont_ints([1], p).reshape(-1, 4)
    g = G.enc(gamma, p)
    compress = lambda c: [(a + theta * b + theta * theta * d) % p for a, b, d in zip(*c)]   # noqa: E731
    tcols = [MLE.from_evaluations(fname, 6, S.encode(c, p)) for c in cols]
    tm = MLE.linear_combination(tcols, coeffs)
    tc = compress(cols)
    assert len(set(tc)) == 64 and np.array_equal(tm.to_evaluations(), S.encode(tc, p))
    tden = MLE.linear_combination([tm], one, g)
    tcanon = [(gamma + v) % p for v in tc]
    for altered in (False, True):
        wcols = [[c[i] for i in idx] for c in cols]
        if altered:
            wcols[1][77] = outside                         # one column of one row: the row is no row of the table
        wc = compress(wcols)
        assert (wc[77] in tc) == (not altered)
        wms = [MLE.from_evaluations(fname, 9, S.encode(c, p)) for c in wcols]
        wm = MLE.linear_combination(wms, coeffs)
        m, missing, found = MLE.lookup(tm, wm, indices=True)
        want_idx, mcanon, want_missing = R.lookup(tc, wc)
        assert missing == want_missing == (1 if altered else 0) and found.tolist() == want_idx
        assert np.array_equal(m.to_evaluations(), S.encode(mcanon, p))
        _, (pt, qt) = FS.prove_and_verify(fname, m, tden, mcanon, tcanon)
        wden = MLE.linear_combination([wm], one, g)
        _, (pw, qw) = FS.prove_and_verify(fname, None, wden, None, [(gamma + v) % p for v in wc])
        assert (pw * qt % p == pt * qw % p) == (not altered), altered
        for x in wms + [wm, m, wden]:
            x.free()
    for x in tcols + [tm, tden]:
        x.free()
