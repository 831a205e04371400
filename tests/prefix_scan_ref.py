"""Big-integer model of the prefix scans on device vectors (ark_hip_fr_prefix_product_device, _sum_device, _ratio_device),
on Montgomery residues as the plain integers they are: an element a is stored as a R mod p, the product of two stored
values x, y is x y / R, the stored one is R, and the stored inverse of x is R^2 / x.  inv0(0) = 0, as ark_hip_fr_div_device
leaves zero divisors.  Nothing here touches the library."""
import numpy as np

import pyref


def ints(a):
    """numpy [n, 4] uint64 -> list of the n integers the limbs spell"""
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def limbs(xs):
    if not len(xs):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


class Field:
    def __init__(self, fname):
        self.name = fname
        self.p = pyref.MODULI[fname][0]
        self.R = pyref.R_of(self.p)
        self.rinv = pow(self.R, -1, self.p)
        self.one = self.R % self.p
        self.r2 = self.R * self.R % self.p

    def mul(self, x, y):
        return x * y * self.rinv % self.p

    def inv0(self, x):
        return self.r2 * pow(x, -1, self.p) % self.p if x else 0

    def enc(self, v):
        return v % self.p * self.R % self.p


def prefix_product(f, a, exclusive):
    """(out, total) for the stored values a"""
    out, run = [0] * len(a), f.one
    for i, x in enumerate(a):
        if exclusive:
            out[i] = run
        run = f.mul(run, x)
        if not exclusive:
            out[i] = run
    return out, run


def prefix_sum(f, a, exclusive):
    out, run = [0] * len(a), 0
    for i, x in enumerate(a):
        if exclusive:
            out[i] = run
        run = (run + x) % f.p
        if not exclusive:
            out[i] = run
    return out, run


def prefix_ratio(f, num, den):
    """(out, last): out[i] = PN_i inv0(PD_i) with PN, PD the exclusive prefix products; last the same at i = n"""
    pn, tn = prefix_product(f, num, True)
    pd, td = prefix_product(f, den, True)
    return [f.mul(x, f.inv0(y)) for x, y in zip(pn, pd)], f.mul(tn, f.inv0(td))


def naive_product(f, a, upto):
    """the stored product of a[0 .. upto), every factor multiplied in afresh: quadratic when called for every index"""
    v = 1
    for x in a[:upto]:
        v = v * (x * f.rinv % f.p) % f.p      # canonical values
    return v * f.R % f.p
