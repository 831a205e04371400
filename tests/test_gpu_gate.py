"""Gate expressions on device vectors (ark_hip_fr_sum_of_products_device, csrc/gateexpr.cuh) against the big-integer model of
tests/gate_ref.py, limb for limb: every size class and the plan's seams, every rotation class on columns with planted values,
every term shape, in place, the bytes behind the output and the inputs untouched, the Python mirrors, and a quotient polynomial
of a three-wire circuit computed without leaving the device."""
import ctypes as C

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import gates as G
from algebra_amd._lib import lib
import gate_ref as R

pytestmark = pytest.mark.gpu

FR = ["BN254_FR", "BLS12_381_FR", "BLS12_377_FR"]
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
GUARD = 8                                             # elements behind every vector, holding a pattern
PATTERN = np.arange(1, GUARD * 4 + 1, dtype=np.uint64).reshape(GUARD, 4) * np.uint64(0x0101010101010101)


def rotations(n):
    return [0, 1, -1, n - 1, n, -n, n + 1, 4, 8, I64_MIN, I64_MAX]


class Guarded:
    """n elements on the device followed by GUARD elements of a pattern"""

    def __init__(self, fname, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 4)
        self.n, self.rows = rows.shape[0], rows
        self.vec = A.DeviceVec.from_host(fname, np.concatenate([rows, PATTERN]))
        self.ptr = self.vec.ptr.value

    def read(self):
        got = self.vec.to_host()
        assert np.array_equal(got[self.n:], PATTERN), "the bytes behind the vector changed"
        return got[:self.n]

    def free(self):
        self.vec.free()


def run(fname, columns, n, terms, c0=None, in_place=None, alias=None):
    """One call of the entry on `columns` (lists of stored integers); terms as gate_ref takes them.  Returns the output's
    limbs after checking the guards and that no input changed.  in_place: the column index d_out equals; alias: (k, l) passes
    column l's pointer for column k as well (the model then reads l's values for k)."""
    f = R.Field(fname)
    if alias:
        columns = list(columns)
        columns[alias[0]] = columns[alias[1]]
    dev = [Guarded(fname, R.limbs(c)) for c in columns]
    ptrs = [d.ptr for d in dev]
    if alias:
        ptrs[alias[0]] = ptrs[alias[1]]
    poison = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    out = dev[in_place] if in_place is not None else Guarded(fname, poison)
    one = R.limbs([f.one])[0]
    products = [(one if c is None else R.limbs([c])[0], list(fs)) for c, fs in terms]
    G._call(A.curves.field_id(fname), ptrs, n, products, None if c0 is None else R.limbs([c0])[0], C.c_void_p(out.ptr))
    got = out.read()
    for k, d in enumerate(dev):
        if k != in_place:
            assert np.array_equal(d.read(), d.rows), "column %d changed" % k
    for d in dev + ([out] if in_place is None else []):
        d.free()
    want = R.limbs(R.sum_of_products(f, columns, n, terms, c0))
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s n=%d: %d rows differ, the first at %d" % (fname, n, bad.size, int(bad[0]))
    return got


def coefficient(f, seed):
    return R.rand_elems(f, 1, seed)[0]


# ---- sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(fname, n):
    f = R.Field(fname)
    cols = [R.planted(f, n, 100 + 7 * k + n) for k in range(3)]
    terms = [(None, [(0, 0), (1, 1)]), (coefficient(f, 5), [(2, -1), (0, 4), (1, 0)]), (f.enc(-1), [(2, n + 1)])]
    run(fname, cols, n, terms, coefficient(f, 6))
    run(fname, cols, n, terms[:2])


def seam_columns(f, n, seam, count):
    """numpy-made columns for the large sizes (stored values below 2^252, hence canonical) with the planted values at the ends
    and on both sides of the rows where a lane's second and third row begin"""
    rng = np.random.default_rng(n)
    cols = []
    for k in range(count):
        a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)
        special = R.limbs([f.one, f.enc(-1), f.p - 1, 0])
        for t, i in enumerate(sorted(set(i % n for i in (0, 1, -2, -1, seam - 1, seam, 2 * seam - 1, 2 * seam, 255, 256)))):
            a[i] = special[(t + k) % 4]
        cols.append(R.ints(a))
    return cols


def test_the_seam_of_the_plan():
    """rows_per_lane 1, 2 and 3: the last size whose grid is uncapped, the first beyond it, and the first with a third row"""
    fname = "BLS12_381_FR"
    f = R.Field(fname)
    cap = A.sum_of_products_plan(1 << 40)[0]
    seam = cap * 256
    for n, rpl in ((seam, 1), (seam + 1, 2), (2 * seam + 1, 3)):
        assert A.sum_of_products_plan(n) == (cap, rpl)
        cols = seam_columns(f, n, seam, 2)
        run(fname, cols, n, [(coefficient(f, 9), [(0, 1), (1, 0)]), (None, [(1, -1)])])


# ---- rotations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
@pytest.mark.parametrize("n", [3, 257, 1000])
def test_rotations(fname, n):
    f = R.Field(fname)
    a, b = R.planted(f, n, 31 + n), R.planted(f, n, 32 + n)
    rots = rotations(n)
    # every rotation as a factor next to an unrotated one, in one expression ...
    run(fname, [a, b], n, [(None if j % 2 else coefficient(f, 50 + j), [(0, r), (1, 0)]) for j, r in enumerate(rots)])
    # ... and as the rotated copy: one unit term of one factor, through the entry and through DeviceVec.rotate
    da = A.DeviceVec.from_host(fname, R.limbs(a))
    for r in rots:
        got = run(fname, [a], n, [(None, [(0, r)])])
        k = r % n
        assert np.array_equal(got, R.limbs(a[k:] + a[:k]))
        dr = da.rotate(r)
        assert np.array_equal(dr.to_host(), got), r
        dr.free()
    out = A.DeviceVec(fname, n)
    assert da.rotate(n + 1, out=out) is out and np.array_equal(out.to_host(), R.limbs(a[1 % n:] + a[:1 % n]))
    assert np.array_equal(da.to_host(), R.limbs(a))
    if n > 1:
        with pytest.raises(A.ArkHipError):
            da.rotate(1, out=da)                                               # a rotated copy has no in-place form
    assert da.rotate(-n, out=da) is da and np.array_equal(da.to_host(), R.limbs(a))   # rotation 0 after reduction has
    da.free()
    out.free()


# ---- term shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FR)
def test_term_shapes(fname):
    f = R.Field(fname)
    n = 257
    cols = [R.planted(f, n, 200 + k) for k in range(16)]
    c = coefficient(f, 1)
    for c0 in (None, coefficient(f, 2), 0, f.p - 1):
        run(fname, cols[:2], n, [(None, [(0, 0), (1, 0)])], c0)                # coefficient one
        run(fname, cols[:2], n, [(f.one, [(0, 0), (1, 0)])], c0)               # ... given as the element
        run(fname, cols[:2], n, [(c, [(0, 0), (1, 0)])], c0)                   # a general coefficient
        run(fname, cols[:2], n, [(0, [(0, 0), (1, 0)])], c0)                   # a zero coefficient
        run(fname, cols[:2], n, [(0, [(0, 0)]), (c, [(1, 3)]), (None, [(0, -3)])], c0)
    run(fname, cols[:1], n, [(None, [(0, 0)] * 8)])                            # a column to the 8th power
    run(fname, cols[:1], n, [(c, [(0, 5)] * 8)], c)
    run(fname, cols[:1], n, [(None, [(0, 0), (0, 4)])])                        # one term, the same column at two rotations
    run(fname, cols[:2], n, [(c, [(1, -1), (1, 0), (1, 1), (0, 0)])])
    rng = np.random.default_rng(16)
    rots = rotations(n)
    full = []
    for j in range(16):                                                        # 16 terms x 8 factors over 16 columns
        factors = [(int((j + 3 * q) % 16), rots[int(rng.integers(0, len(rots)))]) for q in range(8)]
        full.append((None if j % 3 == 0 else coefficient(f, 300 + j), factors))
    assert sorted(set(k for _, fs in full for k, _ in fs)) == list(range(16))
    run(fname, cols, n, full, c)
    run(fname, cols, n, full)
    # the same pointer passed as two columns
    run(fname, cols[:3], n, [(c, [(0, 1), (1, 2)]), (None, [(2, 0), (1, 0)])], alias=(1, 0))
    run(fname, cols[:2], n, [(None, [(0, 0), (1, 0)])], alias=(1, 0))


@pytest.mark.parametrize("fname", FR)
def test_in_place(fname):
    f = R.Field(fname)
    c = coefficient(f, 3)
    for n in (1, 65, 1000):
        cols = [R.planted(f, n, 400 + k + n) for k in range(3)]
        run(fname, cols, n, [(c, [(0, 0), (1, 1)]), (None, [(0, 0), (0, 0), (2, -1)])], c, in_place=0)
        run(fname, cols, n, [(None, [(1, n)]), (c, [(1, -n), (0, 7)])], in_place=1)   # rotations that reduce to 0
        run(fname, cols[:1], n, [(None, [(0, 0)])], in_place=0)                  # the copy onto itself
        run(fname, cols, n, [(c, [(0, 0), (1, n), (2, 2)])], in_place=0, alias=(1, 0))   # d_out under two column indices
    a = A.DeviceVec.from_host(fname, R.limbs(R.planted(f, 65, 1)))
    one = R.limbs([f.one])[0]
    with pytest.raises(A.ArkHipError):                                           # refused where a read of it is rotated,
        G._call(a.field, [a.ptr.value, a.ptr.value], 65, [(one, [(0, 2), (1, 0)])], None, a.ptr)   # under either index
    for rot in (1, -1, 66, I64_MAX):
        with pytest.raises(A.ArkHipError) as e:
            G._call(a.field, [a.ptr.value], 65, [(one, [(0, rot)])], None, a.ptr)
        assert e.value.code == -1
    with pytest.raises(A.ArkHipError):
        G._call(a.field, [a.ptr.value], 64, [(one, [(0, 0)])], None, C.c_void_p(a.ptr.value + 32))   # a partial overlap
    a.free()


# ---- the Python mirror -----------------------------------------------------------------------------------------------------
def test_the_builder_reproduces_the_model():
    fname = "BLS12_377_FR"
    f = R.Field(fname)
    n = 300
    cols = [R.planted(f, n, 500 + k) for k in range(3)]
    d = [A.DeviceVec.from_host(fname, R.limbs(c)) for c in cols]
    c, c0 = coefficient(f, 4), coefficient(f, 5)
    s = A.SumOfProducts(fname, n)
    s.add_product([d[0], (d[1], 4), d[0]]).add_product([(d[2], -1)], R.limbs([c])[0]).add_product([(d[1], I64_MIN), d[2]], R.limbs([f.one])[0])
    terms = [(None, [(0, 0), (1, 4), (0, 0)]), (c, [(2, -1)]), (None, [(1, I64_MIN), (2, 0)])]
    out = s.evaluate()
    assert np.array_equal(out.to_host(), R.limbs(R.sum_of_products(f, cols, n, terms)))
    s.set_constant(R.limbs([c0])[0])
    assert s.evaluate(out=out) is out and np.array_equal(out.to_host(), R.limbs(R.sum_of_products(f, cols, n, terms, c0)))
    assert s.evaluate(out=d[0]) is d[0] and np.array_equal(d[0].to_host(), out.to_host())   # column 0 is read at rotation 0 only
    empty = A.SumOfProducts(fname, 0).add_product([A.DeviceVec(fname, 0)]).evaluate()
    assert empty.len == 0
    for v in d + [out]:
        v.free()


def test_n_zero_touches_nothing():
    fname = "BN254_FR"
    out = Guarded(fname, np.zeros((0, 4), dtype=np.uint64))
    one = R.limbs([R.Field(fname).one])[0]
    G._call(A.curves.field_id(fname), [0, 0], 0, [(one, [(0, 3), (1, 0)])], one, C.c_void_p(out.ptr))
    assert lib().ark_hip_synchronize() == 0
    out.read()
    out.free()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_a_quotient_polynomial_without_leaving_the_device():
    """A satisfied three-wire circuit of m = 64 rows with random gates and copy constraints through a permutation:
        q_M a b + q_L a + q_R b + q_O c + q_C  +  alpha (z N - z(wX) D)  +  alpha^2 L_1 (z - 1)
    with N = prod_k (w_k + beta id_k + gamma), D = prod_k (w_k + beta sigma_k + gamma) as columns and z = prefix_ratio(N, D).
    On the base domain the expression is the zero vector; with one wire value changed exactly the rows the model predicts are
    non-zero.  Then the columns go through interpolate and the coset of size 4 m, the expression is evaluated with rotation 4,
    multiplied by the Z_H^-1 column and interpolated: the quotient t has no coefficient from 3 m on, and at a point zeta
    t(zeta) Z_H(zeta) equals the expression computed in big integers from the column polynomials' values at zeta and w zeta."""
    fname = "BLS12_381_FR"
    f = R.Field(fname)
    m, blow = 64, 4
    rng = np.random.default_rng(64)

    def fpow(x, e):
        return f.enc(pow(x * f.rinv % f.p, e, f.p))

    def finv(x):
        return fpow(x, f.p - 2)
    # the witness: an input of a row is random or a copy of an earlier cell; c closes the gate
    pool = iter(R.rand_elems(f, 8 * m, 640))
    qM, qL, qR, qC = ([next(pool) for _ in range(m)] for _ in range(4))
    qO = [f.enc(-1)] * m
    wires = [[0] * m for _ in range(3)]
    cls, classes = [[0] * m for _ in range(3)], 0                               # the class of equal cells a cell belongs to
    for i in range(m):
        for k in (0, 1):
            if i and rng.integers(0, 2):
                kk, ii = int(rng.integers(0, 3)), int(rng.integers(0, i))
                wires[k][i], cls[k][i] = wires[kk][ii], cls[kk][ii]
            else:
                wires[k][i], cls[k][i], classes = next(pool), classes, classes + 1
        a, b = wires[0][i], wires[1][i]
        wires[2][i] = (f.mul(f.mul(qM[i], a), b) + f.mul(qL[i], a) + f.mul(qR[i], b) + qC[i]) % f.p
        cls[2][i], classes = classes, classes + 1
    cells = [(k, i) for k in range(3) for i in range(m)]
    sigma = {cell: cell for cell in cells}
    for v in range(classes):                                                    # one cycle through every class
        members = [cell for cell in cells if cls[cell[0]][cell[1]] == v]
        for x, y in zip(members, members[1:] + members[:1]):
            sigma[x] = y
    assert sum(1 for cell in cells if sigma[cell] != cell) > m // 2
    ident = {cell: f.enc(cell[0] * m + cell[1] + 1) for cell in cells}
    alpha, beta, gamma = R.rand_elems(f, 3, 641)
    num, den = [f.one] * m, [f.one] * m
    for k in range(3):
        for i in range(m):
            num[i] = f.mul(num[i], (wires[k][i] + f.mul(beta, ident[(k, i)]) + gamma) % f.p)
            den[i] = f.mul(den[i], (wires[k][i] + f.mul(beta, ident[sigma[(k, i)]]) + gamma) % f.p)
    dn, dd = A.DeviceVec.from_host(fname, R.limbs(num)), A.DeviceVec.from_host(fname, R.limbs(den))
    dz, last = dn.prefix_ratio(dd)
    assert np.array_equal(last, R.limbs([f.one])[0])                            # the permutation closes
    z = R.ints(dz.to_host())
    assert z[0] == f.one and len(set(z)) > m // 2
    L1 = [f.one] + [0] * (m - 1)
    names = ["qM", "a", "b", "qL", "qR", "qO", "c", "qC", "z", "N", "D", "L1"]
    base = dict(zip(names, [qM, wires[0], wires[1], qL, qR, qO, wires[2], qC, z, num, den, L1]))
    a2 = f.mul(alpha, alpha)

    def terms(step):
        ix = {nm: k for k, nm in enumerate(names)}
        return [(None, [(ix["qM"], 0), (ix["a"], 0), (ix["b"], 0)]), (None, [(ix["qL"], 0), (ix["a"], 0)]),
                (None, [(ix["qR"], 0), (ix["b"], 0)]), (None, [(ix["qO"], 0), (ix["c"], 0)]), (None, [(ix["qC"], 0)]),
                (alpha, [(ix["z"], 0), (ix["N"], 0)]), (f.p - alpha, [(ix["z"], step), (ix["D"], 0)]),
                (a2, [(ix["L1"], 0), (ix["z"], 0)]), (f.p - a2, [(ix["L1"], 0)])]

    def expression(vecs, step):
        s = A.SumOfProducts(fname, vecs[names[0]].len)
        for coeff, factors in terms(step):
            s.add_product([(vecs[names[k]], r) for k, r in factors], None if coeff is None else R.limbs([coeff])[0])
        assert len(s.columns) == 12 and len(s.products) == 9
        return s.evaluate()

    dev = {nm: A.DeviceVec.from_host(fname, R.limbs(base[nm])) for nm in names}
    e = expression(dev, 1)
    assert not e.to_host().any()                                                # satisfied: zero on every row, the wrap included
    e.free()
    # one wire value changed: the model names the rows
    row = 37
    bad = dict(base)
    bad["a"] = list(base["a"])
    bad["a"][row] = (bad["a"][row] + f.one) % f.p
    want = R.sum_of_products(f, [bad[nm] for nm in names], m, terms(1))
    assert [i for i in range(m) if want[i]] == [row]                            # the gate of that row; z, N, D are columns here
    keep = dev["a"]
    dev["a"] = A.DeviceVec.from_host(fname, R.limbs(bad["a"]))
    e = expression(dev, 1)
    assert np.array_equal(e.to_host(), R.limbs(want))
    e.free()
    dev["a"].free()
    dev["a"] = keep
    # the quotient: columns -> coefficients -> the coset of size 4 m
    H = A.Radix2EvaluationDomain.new(fname, m)
    g = f.enc(7)
    coset = A.Radix2EvaluationDomain.new(fname, blow * m).get_coset(R.limbs([g])[0])
    w = R.ints(H.group_gen().reshape(1, 4))[0]
    w4 = R.ints(coset.group_gen().reshape(1, 4))[0]
    assert fpow(w4, blow) == w and fpow(w, m) == f.one and fpow(w, m // 2) != f.one
    polys, ext = {}, {}
    for nm in names:
        polys[nm] = dev[nm].clone().interpolate(H)                              # m coefficients
        ext[nm] = polys[nm].clone().evaluate_over_domain(coset)                 # 4 m evaluations at g w4^i
    t = expression(ext, blow)                                                   # "the next row" is 4 indices on
    gm, u = fpow(g, m), fpow(w4, m)                                             # Z_H(g w4^i) = g^m (w4^m)^i - 1: four values
    zh = [(f.mul(gm, fpow(u, i % blow)) - f.one) % f.p for i in range(blow * m)]
    assert all(zh[:blow])
    zhinv = A.DeviceVec.from_host(fname, R.limbs([finv(x) for x in zh]))
    t *= zhinv
    t.interpolate(coset)
    tc = R.ints(t.to_host())
    assert not any(tc[3 * m:])
    assert not any(tc[2 * m - 2:])              # degrees: q_M a b < 3 m - 2, all of it divisible by Z_H of degree m
    assert sum(1 for x in tc if x) > m
    zeta = R.rand_elems(f, 1, 642)[0]
    at = {}
    for nm in names:
        at[nm] = R.ints(polys[nm].evaluate(R.limbs([zeta])[0]).reshape(1, 4))[0]
    z_next = R.ints(polys["z"].evaluate(R.limbs([f.mul(zeta, w)])[0]).reshape(1, 4))[0]
    mul = f.mul
    expr = (mul(mul(at["qM"], at["a"]), at["b"]) + mul(at["qL"], at["a"]) + mul(at["qR"], at["b"]) + mul(at["qO"], at["c"]) + at["qC"]
            + mul(alpha, (mul(at["z"], at["N"]) - mul(z_next, at["D"])) % f.p)
            + mul(a2, mul(at["L1"], (at["z"] - f.one) % f.p))) % f.p
    t_zeta = R.ints(t.evaluate(R.limbs([zeta])[0]).reshape(1, 4))[0]
    assert mul(t_zeta, (fpow(zeta, m) - f.one) % f.p) == expr and expr != 0
    for v in list(dev.values()) + list(polys.values()) + list(ext.values()) + [dn, dd, dz, t, zhinv]:
        v.free()
