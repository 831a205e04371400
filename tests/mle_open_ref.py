"""Big-integer model of the multilinear-opening entries, on Python integers modulo p, beside
tests/mle_ref.py whose conventions it keeps (index bit 0 is the first variable).

The quotients and the value are linear in the table, so a table of Montgomery residues a R can be fed as it is with the POINT
in canonical form (mle_ref's remark).  The eq table is NOT linear in anything: its model works on canonical values, and
`eq_table_mont` converts to Montgomery residues at the end."""
import mle_ref


def eq_table(point, scale, p):
    """[scale * prod_i (bit i of b ? point[i] : 1 - point[i]) for b < 2^len(point)], by doubling: the table of the variables
    from i on gives the one from i - 1 on, entry b becoming entries 2b (times 1 - r) and 2b + 1 (times r)"""
    t = [scale % p]
    for r in reversed(point):
        nxt = [0] * (2 * len(t))
        for b, v in enumerate(t):
            hi = v * r % p
            nxt[2 * b] = (v - hi) % p
            nxt[2 * b + 1] = hi
        t = nxt
    return t


def eq_table_mont(point, scale, p, R):
    return [v * R % p for v in eq_table(point, scale, p)]


def segment_offset(num_vars, i):
    """element offset of q_i in the output of 2^num_vars - 1 elements"""
    return (1 << num_vars) - (1 << (num_vars - i))


def segment_len(num_vars, i):
    return 1 << (num_vars - 1 - i)


def quotients(table, point, p):
    """(f(point), [q_0, .., q_{nu-1}]): q_i[b] = f_i[2b+1] - f_i[2b], f_0 = table, f_{i+1} = f_i with its first variable
    bound to point[i]"""
    assert len(table) == 1 << len(point)
    f, qs = list(table), []
    for r in point:
        qs.append([(f[2 * b + 1] - f[2 * b]) % p for b in range(len(f) // 2)])
        f = mle_ref.fix_variables(f, [r], p)
    return f[0], qs


def opening_identity_rhs(qs, point, x, p):
    """sum_i (x_i - point_i) q_i(x_{i+1}, ..): what f(x) - f(point) must equal"""
    total = 0
    for i, q in enumerate(qs):
        total += (x[i] - point[i]) * mle_ref.evaluate(q, x[i + 1:], p)
    return total % p
