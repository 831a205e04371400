"""The models of the polynomial operations on device vectors (ark_hip_poly_divide_linear_device, _divide_by_vanishing_device,
ark_hip_domain_lagrange_coefficients_device): the reference's own loops on Python integers and on the oracle's additions.
Shared by tests/test_gpu_poly_ops.py and tests/async_cases.py.  Nothing here touches the library."""
import numpy as np

import oracle_lib as O
import pyref


def limbs(xs):
    if not xs:
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def synthetic_division(cm, zc, p):
    """coefficients as integers (Montgomery residues), canonical point -> (quotient list, remainder), same form"""
    q = [0] * max(len(cm) - 1, 0)
    s = 0
    for i in range(len(cm) - 1, -1, -1):
        if i < len(q):
            q[i] = s
        s = (cm[i] + zc * s) % p
    return q, s


def vanishing_reference(fid, a, m):
    """dense.rs:168-211 restated on numpy arrays with the oracle's additions"""
    n = a.shape[0]
    if n < m:
        return np.zeros((0, 4), dtype=np.uint64), a.copy()
    q = a[m:].copy()
    for i in range(1, n // m):
        seg = a[m * (i + 1):]
        if seg.shape[0]:
            q[:seg.shape[0]] = O.field_op(fid, "add", q[:seg.shape[0]], seg).reshape(-1, 4)
    r = a[:m].copy()
    k = min(m, q.shape[0])
    if k:
        r[:k] = O.field_op(fid, "add", r[:k], q[:k]).reshape(-1, 4)
    return q, r


def lagrange_reference(fname, log_n, h, tau):
    """L_i(tau) = Z_H(tau) v_i / (tau - h g^i), v_i = g^i / (m h^(m-1)) (domain/mod.rs:157-222), canonical integers; one batch
    inversion for all the denominators"""
    p = pyref.MODULI[fname][0]
    m = 1 << log_n
    g = pyref.root_of_unity(fname, log_n)
    zh = (pow(tau, m, p) - pow(h, m, p)) % p
    assert zh, "tau lies in the domain"
    den, pw = [0] * m, 1
    for i in range(m):
        den[i] = (tau - h * pw) % p
        pw = pw * g % p
    pre, run = [0] * m, 1
    for i in range(m):
        pre[i] = run
        run = run * den[i] % p
    inv = pow(run, -1, p)
    out = [0] * m
    k = zh * pow(m * pow(h, m - 1, p), -1, p) % p
    gp = pow(g, m - 1, p) if m > 1 else 1
    gi = pow(g, -1, p)
    for i in range(m - 1, -1, -1):
        out[i] = k * gp % p * (inv * pre[i] % p) % p
        inv = inv * den[i] % p
        gp = gp * gi % p
    return out


def mont_list(xs, p):
    r = pyref.R_of(p)
    return limbs([x * r % p for x in xs])
