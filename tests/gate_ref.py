"""Big-integer model of the gate expression on device vectors (ark_hip_fr_sum_of_products_device), on Montgomery residues as
the plain integers they are (the product of two stored values x, y is x y / R):

    out[i] = c0 + sum_j c_j prod_q col[tc_jq][(i + rot_jq) mod n]

A term is (coefficient or None for one, [(column index, rotation)]).  Nothing here touches the library."""
import numpy as np

from prefix_scan_ref import Field, ints, limbs  # noqa: F401  (the same field model)
from csr_ref import rand_elems  # noqa: F401


def sum_of_products(f, columns, n, terms, c0=None):
    """the n stored values of the expression; columns: lists of n stored values"""
    p, rinv, one = f.p, f.rinv, f.one
    out = [0 if c0 is None else c0 % p] * n
    for coeff, factors in terms:
        views = []
        for k, rot in factors:
            r = rot % n if n else 0           # Python's % is the mathematical mod
            col = columns[k]
            views.append(col[r:] + col[:r] if r else col)
        c = one if coeff is None else coeff
        for i in range(n):
            pr = c
            for v in views:
                pr = pr * v[i] * rinv % p
            out[i] = (out[i] + pr) % p
    return out


def naive(f, columns, n, terms, c0=None):
    """the same, written independently: every column is rotated as a list first, a row's terms are then computed on
    canonical VALUES and the sum is encoded at the end"""
    def value(x):
        return x * f.rinv % f.p
    out = []
    rotated = []
    for coeff, factors in terms:
        cols = []
        for k, rot in factors:
            col = list(columns[k])
            steps = rot
            while steps < 0:                  # bring the rotation into [0, n) without %
                steps += n * max(1, (-steps) // n)
            while steps >= n:
                steps -= n * max(1, steps // n)
            for _ in range(steps):
                col.append(col.pop(0))
            cols.append(col)
        rotated.append(cols)
    for i in range(n):
        acc = 0 if c0 is None else value(c0)
        for (coeff, _), cols in zip(terms, rotated):
            t = 1 if coeff is None else value(coeff)
            for col in cols:
                t *= value(col[i])
            acc += t
        out.append(f.enc(acc))
    return out


PLANT_EDGES = (0, 1, -2, -1)


def planted(f, n, seed):
    """n random stored values with one, -1, p - 1 and 0 planted at indices 0, 1, n-2, n-1 and both sides of every 64- and
    256-row boundary (for n above 2^16: of the first and the last boundaries): a wrong wrap or an off-by-one reads one of them"""
    col = rand_elems(f, n, seed)
    special = (f.one, f.enc(-1), f.p - 1, 0)
    at = set(i % n for i in PLANT_EDGES) if n else set()
    bounds = list(range(64, n, 64))
    if len(bounds) > 2048:
        bounds = bounds[:1024] + bounds[-1024:]
    for b in bounds:
        at.update((b - 1, b))
    for t, i in enumerate(sorted(at)):
        if 0 <= i < n:
            col[i] = special[(t + seed) % 4]
    return col
