"""Big-integer model of DenseMultilinearExtension (poly/src/evaluations/multivariate/multilinear/dense.rs), the reference's
own loops on Python integers.  Everything works modulo p on plain integers; a table of Montgomery residues a R can be fed
as it is with the POINT in canonical form, because the fold is linear in the table: (a R) + r ((b R) - (a R)) = (a + r (b - a)) R."""
import numpy as np


def swap_bits(x, a, b, n):
    """multilinear/mod.rs:90-96"""
    a_bits = (x >> a) & ((1 << n) - 1)
    b_bits = (x >> b) & ((1 << n) - 1)
    local = a_bits ^ b_bits
    return x ^ ((local << a) | (local << b))


def fix_variables(table, point, p):
    """dense.rs:224-257: binds the first len(point) variables; index bit 0 is the first variable"""
    assert len(point) <= (len(table) - 1).bit_length() and len(table) & (len(table) - 1) == 0
    poly = list(table)
    for r in point:
        poly = [(poly[2 * b] + r * (poly[2 * b + 1] - poly[2 * b])) % p for b in range(len(poly) // 2)]
    return poly


def evaluate(table, point, p):
    """dense.rs:460-465"""
    assert len(table) == 1 << len(point)
    return fix_variables(table, point, p)[0]


def evaluate_data_array(data, point, p):
    """the reference's test helper (dense.rs:476-492): a (1 - r) + b r"""
    assert len(data) == 1 << len(point)
    a = list(data)
    for i, r in enumerate(point, 1):
        for b in range(1 << (len(point) - i)):
            a[b] = (a[b << 1] * (1 - r) + a[(b << 1) + 1] * r) % p
    return a[0]


def relabel(table, a, b, k):
    """dense.rs:76-92 on a copy"""
    out = list(table)
    if a > b:
        a, b = b, a
    if a == b or k == 0:
        return out
    nv = (len(table) - 1).bit_length()
    assert b + k <= nv, "invalid relabel argument"
    assert a + k <= b, "overlapped swap window is not allowed"
    for i in range(len(out)):
        j = swap_bits(i, a, b, k)
        if i < j:
            out[i], out[j] = out[j], out[i]
    return out


def eq(index, point, p):
    """prod_j (index bit j ? r_j : 1 - r_j): the weight of table entry `index` in the value at `point`"""
    w = 1
    for j, r in enumerate(point):
        w = w * (r if (index >> j) & 1 else 1 - r) % p
    return w


def ints(a):
    """numpy [n, 4] uint64 -> the n integers the limbs spell"""
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def limbs(xs):
    if not len(xs):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)
