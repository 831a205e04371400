"""Big-integer model of the sparse matrices on the device (ark_hip_fr_csr_*): row sums of Montgomery products on the stored
residues as the plain integers they are (the product of two stored values x, y is x y / R), a stable transposition, and a
restatement of the row plan's rule with its invariants.  Nothing here touches the library."""
import numpy as np

from prefix_scan_ref import Field, ints, limbs  # noqa: F401  (the same field model)


def rand_elems(f, n, seed):
    """n uniformly random stored values as integers (the seed fixes them)"""
    raw = np.random.default_rng(seed).bytes(40 * n)
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") % f.p for i in range(n)]


def mul(f, rows, row_ptr, col_idx, vals, x):
    """y = M x on stored values: vals and x lists of integers, y a list of `rows` integers.  Dense-free; duplicates add."""
    y = []
    for r in range(rows):
        acc = 0
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            acc += vals[j] * x[int(col_idx[j])]
        y.append(acc * f.rinv % f.p)
    return y


def transpose(rows, cols, row_ptr, col_idx, vals):
    """(row_ptr, col_idx, vals) of M^T by a STABLE counting sort over the columns: inside a row of M^T the entries keep
    ascending original row order (and, for duplicates, their order inside the row).  vals: any indexable (list or array)."""
    nnz = int(row_ptr[rows])
    t_ptr = [0] * (cols + 1)
    for j in range(nnz):
        t_ptr[int(col_idx[j]) + 1] += 1
    for c in range(cols):
        t_ptr[c + 1] += t_ptr[c]
    at = t_ptr[:-1].copy() if cols else []
    t_idx, src = [0] * nnz, [0] * nnz
    for r in range(rows):
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            d = at[int(col_idx[j])]
            at[int(col_idx[j])] += 1
            t_idx[d], src[d] = r, j
    if isinstance(vals, np.ndarray):
        t_vals = vals[np.array(src, dtype=np.int64)] if nnz else vals[:0]
    else:
        t_vals = [vals[j] for j in src]
    return np.array(t_ptr, dtype=np.uint32), np.array(t_idx, dtype=np.uint32), t_vals


def dense(f, rows, cols, row_ptr, col_idx, vals):
    """the matrix as rows x cols canonical VALUES (not stored residues), duplicates added"""
    m = [[0] * cols for _ in range(rows)]
    for r in range(rows):
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            c = int(col_idx[j])
            m[r][c] = (m[r][c] + vals[j] * f.rinv) % f.p
    return m


def bilinear(f, rows, row_ptr, col_idx, vals, u, v):
    """u^T M v on stored values: sum val * u[row] * v[col]"""
    acc = 0
    for r in range(rows):
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            acc += f.mul(f.mul(vals[j], v[int(col_idx[j])]), u[r])
    return acc % f.p


def inner(f, a, b):
    return sum(x * y for x, y in zip(a, b)) * f.rinv % f.p


def plan(rows, row_ptr, tile, max_rows):
    """The rule of csrc/csr_plan.hpp restated: (stream, long) with stream a list of (first row, one past the last row) and long a
    list of (row, chunks), plus the order in which they were emitted as a list of ("s", index) / ("l", index)."""
    stream, long_rows, order = [], [], []
    first, n_rows, nnz = 0, 0, 0

    def close(end):
        nonlocal n_rows, nnz
        if n_rows:
            order.append(("s", len(stream)))
            stream.append((first, end))
        n_rows, nnz = 0, 0
    for r in range(rows):
        ln = int(row_ptr[r + 1]) - int(row_ptr[r])
        if ln > tile:
            close(r)
            order.append(("l", len(long_rows)))
            long_rows.append((r, -(-ln // tile)))
            continue
        if n_rows and (nnz + ln > tile or n_rows == max_rows):
            close(r)
        if not n_rows:
            first = r
        n_rows += 1
        nnz += ln
    close(rows)
    return stream, long_rows, order


def check_plan(rows, row_ptr, tile, max_rows, stream, long_rows, order):
    """the invariants: the blocks cover the rows exactly once and in order; a stream block has at most `tile` nonzeros and
    `max_rows` rows and no long row inside; every long row is alone and really long; chunks = ceil(nnz / tile)"""
    at = 0
    for kind, i in order:
        if kind == "s":
            r0, r1 = stream[i]
            assert r0 == at and r1 > r0, (r0, r1, at)
            assert r1 - r0 <= max_rows, (r0, r1)
            assert int(row_ptr[r1]) - int(row_ptr[r0]) <= tile, (r0, r1)
            assert all(int(row_ptr[r + 1]) - int(row_ptr[r]) <= tile for r in range(r0, r1))
            at = r1
        else:
            r, chunks = long_rows[i]
            ln = int(row_ptr[r + 1]) - int(row_ptr[r])
            assert r == at and ln > tile and chunks == -(-ln // tile), (r, ln, chunks)
            at = r + 1
    assert at == rows, (at, rows)
    assert len(order) == len(stream) + len(long_rows)
    return len(stream), len(long_rows), sum(c for _, c in long_rows)
