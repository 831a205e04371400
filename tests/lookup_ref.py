"""The model of ark_hip_fr_lookup_device on Python integers, and the search for elements with a given home slot.

An element is the integer its 32 bytes spell (the Montgomery residue as it is stored): the entry compares stored words and so
does the model.  `lookup` is a first-occurrence dictionary; `lookup_naive` is the quadratic search it is checked against."""
import ctypes as C

import numpy as np

import pyref

MISSING = 0xFFFFFFFF


def first_occurrence(table):
    first = {}
    for j, v in enumerate(table):
        first.setdefault(v, j)
    return first


def lookup(table, values):
    """-> (idx, m, missing): idx[i] = the smallest j with table[j] == values[i] or MISSING; m[j] = #{i : idx[i] = j};
    missing = #{i : idx[i] = MISSING}"""
    first = first_occurrence(table)
    idx = [first.get(v, MISSING) for v in values]
    m = [0] * len(table)
    missing = 0
    for j in idx:
        if j == MISSING:
            missing += 1
        else:
            m[j] += 1
    return idx, m, missing


def lookup_naive(table, values):
    idx = []
    for v in values:
        j = 0
        while j < len(table) and table[j] != v:
            j += 1
        idx.append(j if j < len(table) else MISSING)
    m = [sum(1 for i in idx if i == j) for j in range(len(table))]
    return idx, m, sum(1 for i in idx if i == MISSING)


def words(v):
    """the eight 32-bit words of an element, least significant first"""
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def home_slot(test_lib, fid, v, capacity_log):
    """ark_hip_test_lookup_slot: the home slot the kernels give the element"""
    el = (C.c_uint64 * 4)(*[(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)])
    slot = C.c_uint32(0xDEADBEEF)
    rc = test_lib.ark_hip_test_lookup_slot(fid, el, capacity_log, C.byref(slot))
    assert rc == 0, rc
    return slot.value


COLLIDE_SEED = 2601
COLLIDE_BUDGET = 1 << 15      # candidates: at capacity 2^7 one in 128 lands on a given slot, 256 expected


def random_elements(fname, count, seed):
    """`count` distinct fixed-seed residues below the field's modulus"""
    p = pyref.MODULI[fname][0]
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < count:
        v = int.from_bytes(rng.bytes(40), "little") % p
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def colliding(test_lib, fid, fname, capacity_log, slot, count, budget=COLLIDE_BUDGET, seed=COLLIDE_SEED):
    """the first `count` of `budget` fixed-seed random elements whose home slot is `slot` (fewer if the budget holds fewer)"""
    out = []
    for v in random_elements(fname, budget, seed):
        if home_slot(test_lib, fid, v, capacity_log) == slot:
            out.append(v)
            if len(out) == count:
                break
    return out
