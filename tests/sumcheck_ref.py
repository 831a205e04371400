"""Big-integer model of the sumcheck prover's round (ark_hip_sumcheck_round_device) and of the protocol around it, straight
from the definitions: for tables T_k of 2^m values and terms (c_j, [k ...]),

    g(t) = sum_{b < 2^(m-1)} sum_j c_j prod_{k in term j} ( T_k[2b] + t (T_k[2b+1] - T_k[2b]) ),   t = 0 .. D,

the bind through mle_ref.fix_variables, and a verifier.  Unlike the fold a product is not linear in R, so the model works on
CANONICAL values: `decode` turns Montgomery limbs into integers, `encode` the results back (pyref.to_mont).

A table is a list of integers or, where 2^m values are too many to walk, a `Periodic`: a base block of 2^s values repeated,
plus a dictionary of planted cells; both parts fold exactly."""
import hashlib

import numpy as np

import mle_ref
import pyref


def decode(limbs, p):
    """numpy [n, 4] Montgomery limbs -> canonical integers"""
    rinv = pow(pyref.R_of(p), -1, p)
    return [x * rinv % p for x in mle_ref.ints(limbs)]


def encode(xs, p):
    """canonical integers -> numpy [n, 4] Montgomery limbs"""
    r = pyref.R_of(p)
    return mle_ref.limbs([x % p * r % p for x in xs])


def degree_of(terms):
    return max(len(ix) for _, ix in terms)


def pair_values(lo, hi, terms, p):
    """[sum_j c_j prod_k (lo_k + t (hi_k - lo_k)) for t = 0 .. D] for one pair of rows: lo[k], hi[k] per table"""
    out = []
    for t in range(degree_of(terms) + 1):
        v = [(a + t * (b - a)) % p for a, b in zip(lo, hi)]
        s = 0
        for c, ix in terms:
            pr = c
            for k in ix:
                pr = pr * v[k] % p
            s += pr
        out.append(s % p)
    return out


class Periodic:
    """2^m values: base[i mod 2^s] except at the planted cells"""

    def __init__(self, m, base, cells=None):
        assert len(base) & (len(base) - 1) == 0 and len(base) <= 1 << m
        self.m, self.base, self.cells = m, list(base), dict(cells or {})
        assert all(0 <= i < 1 << m for i in self.cells)

    def __len__(self):
        return 1 << self.m

    def __getitem__(self, i):
        v = self.cells.get(i)
        return self.base[i % len(self.base)] if v is None else v

    def expand(self):
        return [self[i] for i in range(1 << self.m)]

    def fold(self, r, p):
        """fix_variables([r]): the base folds on its own (a one-element base stays), a cell is planted when either parent is"""
        base = mle_ref.fix_variables(self.base, [r], p) if len(self.base) > 1 else list(self.base)
        cells = {}
        for i in self.cells:
            o = i >> 1
            if o not in cells:
                a, b = self[2 * o], self[2 * o + 1]
                cells[o] = (a + r * (b - a)) % p
        return Periodic(self.m - 1, base, cells)


def bind(tables, r, p):
    return [t.fold(r, p) if isinstance(t, Periodic) else mle_ref.fix_variables(t, [r], p) for t in tables]


def round_sums(tables, terms, p):
    """the D + 1 round sums of tables of 2^m values, m >= 1"""
    n = len(tables[0])
    assert n >= 2 and all(len(t) == n for t in tables)
    npairs, d = n // 2, degree_of(terms)
    if not any(isinstance(t, Periodic) for t in tables):
        acc = [0] * (d + 1)
        for b in range(npairs):
            for t, v in enumerate(pair_values([tb[2 * b] for tb in tables], [tb[2 * b + 1] for tb in tables], terms, p)):
                acc[t] += v
        return [a % p for a in acc]
    # periodic: whole periods of pairs from the base blocks, then what the planted pairs change
    bases = [t.base if isinstance(t, Periodic) else list(t) for t in tables]
    period = max(max(len(b) // 2, 1) for b in bases)

    def base_pair(b):
        return [bs[(2 * b) % len(bs)] for bs in bases], [bs[(2 * b + 1) % len(bs)] for bs in bases]
    acc = [0] * (d + 1)
    for b in range(period):
        for t, v in enumerate(pair_values(*base_pair(b), terms, p)):
            acc[t] += v
    acc = [a * (npairs // period) % p for a in acc]
    planted = sorted({i >> 1 for t in tables if isinstance(t, Periodic) for i in t.cells})
    for b in planted:
        now = pair_values([tb[2 * b] for tb in tables], [tb[2 * b + 1] for tb in tables], terms, p)
        was = pair_values(*base_pair(b), terms, p)
        acc = [(a + x - y) % p for a, x, y in zip(acc, now, was)]
    return acc


def final_round(tables, terms, p):
    """what the last call reports for one-element tables: [sum_j c_j prod_k T_k[0], 0, ..., 0]"""
    v = pair_values([t[0] for t in tables], [t[0] for t in tables], terms, p)
    return [v[0]] + [0] * degree_of(terms)


def interpolate(evals, x, p):
    """the value at x of the polynomial of degree <= D through (t, evals[t]), t = 0 .. D (Lagrange)"""
    d = len(evals) - 1
    total = 0
    for i, y in enumerate(evals):
        num, den = 1, 1
        for k in range(d + 1):
            if k != i:
                num = num * (x - k) % p
                den = den * (i - k) % p
        total += y * num * pow(den, -1, p)
    return total % p


def prove(tables, terms, challenge, p):
    """the honest prover on the model: -> (rounds [nu][D + 1], point [nu], per-table final values, final value);
    challenge(i, evals) -> r_(i+1), all canonical"""
    nu = (len(tables[0]) - 1).bit_length()
    rounds, point, cur = [], [], list(tables)
    for i in range(nu):
        g = round_sums(cur, terms, p)
        rounds.append(g)
        r = challenge(i, g) % p
        point.append(r)
        cur = bind(cur, r, p)
    finals = [t[0] for t in cur]
    return rounds, point, finals, final_round(cur, terms, p)[0]


def verify(claim, rounds, point, final_evals, terms, p):
    """The verifier: g_0(0) + g_0(1) is the claimed sum, g_i(r_(i+1)) -- by interpolation over t = 0 .. D -- is
    g_(i+1)(0) + g_(i+1)(1), and the last such value is sum_j c_j prod_k f_k(point), final_evals[k] being f_k(point)."""
    if len(rounds) != len(point):
        return False
    expected = claim % p
    for g, r in zip(rounds, point):
        if len(g) != degree_of(terms) + 1 or (g[0] + g[1]) % p != expected:
            return False
        expected = interpolate(g, r, p)
    return expected == pair_values(final_evals, final_evals, terms, p)[0]


def verify_tables(claim, rounds, point, tables, terms, p):
    """verify with f_k(point) from mle_ref.evaluate of the walked tables"""
    return verify(claim, rounds, point, [mle_ref.evaluate(t, point, p) for t in tables], terms, p)


def hash_challenge(p, seed=b"sumcheck"):
    """A deterministic stand-in for the verifier: r_(i+1) from a hash of the round number and the round's evaluations as
    the Montgomery limbs the device returns.  -> (challenge over limbs -> limbs, challenge over canonical -> canonical)"""
    def of_limbs(i, evals):
        h = hashlib.sha256(seed + bytes([i]) + np.ascontiguousarray(evals, dtype="<u8").tobytes()).digest()
        return int.from_bytes(h + hashlib.sha256(h).digest()[:8], "little") % p

    def device(i, evals):
        return pyref.to_mont(of_limbs(i, evals), p)

    def model(i, evals):
        return of_limbs(i, encode(evals, p))
    return device, model
