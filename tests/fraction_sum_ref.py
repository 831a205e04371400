"""Big-integer model of the fractional-sum entries and of the layered proof around them, on Python
integers modulo p, on top of tests/grand_product_ref.py, tests/mle_open_ref.py and tests/sumcheck_ref.py whose conventions it
keeps (index bit 0 is the first variable, the tree pairs over the LAST variable, canonical values).

The tree carries fractions (N, D): N_nu = num (None: all ones), D_nu = den,
    N_k[i] = N_{k+1}[i] D_{k+1}[i + 2^k] + N_{k+1}[i + 2^k] D_{k+1}[i],   D_k[i] = D_{k+1}[i] D_{k+1}[i + 2^k],
(N_0[0], D_0[0]) = (P, Q) with P / Q = sum_b num[b] / den[b]; each tree's buffer has grand_product_ref's layout.

A layer's sumcheck proves N_k(r_k) + lambda D_k(r_k) = sum_x eq(r_k, x) (n0 d1 + n1 d0 + lambda d0 d1)(x) over the halves of
the levels above; where those are the leaves of a sum with ones for numerators it is eq d1 + eq d0 + lambda eq d0 d1."""
import hashlib

import numpy as np

import grand_product_ref as GP
import mle_open_ref
import pyref
import sumcheck_ref as S

level_offset, level_len, eq_points = GP.level_offset, GP.level_len, GP.eq_points
LAMBDA = "lambda"                 # the round a challenge is asked for when it is the layer's batching challenge


def terms(lam):
    """tables eq, n0, d1, n1, d0 in the order the prover first uses them"""
    return [(1, [0, 1, 2]), (1, [0, 3, 4]), (lam, [0, 4, 2])]


def terms_ones(lam):
    """tables eq, d1, d0: the leaves of a sum with ones for numerators"""
    return [(1, [0, 1]), (1, [0, 2]), (lam, [0, 2, 1])]


def levels(num, den, p):
    """([N_nu, .., N_0], [D_nu, .., D_0]); num None: ones"""
    assert len(den) & (len(den) - 1) == 0 and (num is None or len(num) == len(den))
    ns, ds = [[1] * len(den) if num is None else list(num)], [list(den)]
    while len(ds[-1]) > 1:
        n, d, h = ns[-1], ds[-1], len(ds[-1]) // 2
        ns.append([(n[i] * d[i + h] + n[i + h] * d[i]) % p for i in range(h)])
        ds.append([d[i] * d[i + h] % p for i in range(h)])
    return ns, ds


def tree(num, den, p):
    """((P, Q), the 2^nu - 1 elements of the numerator tree's buffer, of the denominator tree's)"""
    ns, ds = levels(num, den, p)
    return (ns[-1][0], ds[-1][0]), [v for lv in ns[1:] for v in lv], [v for lv in ds[1:] for v in lv]


def counts(indices, table_len):
    """m[j] = #{i : indices[i] = j}; an index >= table_len is skipped"""
    m = [0] * table_len
    for i in indices:
        if i < table_len:
            m[i] += 1
    return m


def prove(num, den, challenge, p):
    """the honest prover on the model: -> ((P, Q), layers, point); layers[k] = (None | (rounds, rho), values), values =
    (n0, n1, d0, d1) or (d0, d1) where the numerators are the implicit ones.  challenge(layer, round | None | LAMBDA, values)"""
    nu = (len(den) - 1).bit_length()
    ns, ds = levels(num, den, p)
    root = (ns[-1][0], ds[-1][0])
    if nu == 0:
        return root, [], []
    values = tuple(ds[nu - 1])
    if not (num is None and nu == 1):
        values = tuple(ns[nu - 1]) + values
    point = [challenge(0, None, list(values)) % p]
    layers = [(None, values)]
    for k in range(1, nu):
        lam = challenge(k, LAMBDA, []) % p
        nup, dup, h = ns[nu - k - 1], ds[nu - k - 1], 1 << k
        eq = mle_open_ref.eq_table(point, 1, p)
        ask = lambda i, g, k=k: challenge(k, i, g)   # noqa: E731
        if num is None and k + 1 == nu:
            _rounds, rho, finals, _ = S.prove([eq, dup[h:], dup[:h]], terms_ones(lam), ask, p)
            values = (finals[2], finals[1])
        else:
            _rounds, rho, finals, _ = S.prove([eq, nup[:h], dup[h:], nup[h:], dup[:h]], terms(lam), ask, p)
            values = (finals[1], finals[3], finals[4], finals[2])
        tau = challenge(k, None, list(values)) % p
        point = rho + [tau]
        layers.append(((_rounds, rho), values))
    return root, layers, point


def verify(num_vars, has_num, root, layers, challenge, p):
    """The verifier of the whole layered proof: -> (accepted, point r_nu, the claim about num(r_nu) -- 1 when the numerators
    are ones --, the claim about den(r_nu)).  Layer 0: P = n0 d1 + n1 d0 and Q = d0 d1.  Layer k: the batched claim
    N_k(r_k) + lambda D_k(r_k) through sumcheck_ref's verifier with its own challenges, the last round against
    eq(r_k, rho) (n0 d1 + n1 d0 + lambda d0 d1); the next claims are the lines through the halves at tau."""
    bad = (False, None, None, None)
    P, Q = root[0] % p, root[1] % p
    if len(layers) != num_vars:
        return bad
    if num_vars == 0:
        return True, [], P, Q
    point = claim_n = claim_d = None
    for k in range(num_vars):
        sc, values = layers[k]
        implicit = not has_num and k + 1 == num_vars         # the level above is the leaves, whose numerators are ones
        if len(values) != (2 if implicit else 4):
            return bad
        n0, n1, d0, d1 = (1, 1) + tuple(values) if implicit else values
        if k == 0:
            if sc is not None or (n0 * d1 + n1 * d0) % p != P or d0 * d1 % p != Q:
                return bad
        else:
            if sc is None:
                return bad
            rounds, rho = sc
            if len(rounds) != k or len(rho) != k:
                return bad
            lam = challenge(k, LAMBDA, []) % p
            if any(r % p != challenge(k, i, g) % p for i, (g, r) in enumerate(zip(rounds, rho))):
                return bad                                   # the prover's point is not the transcript's
            e = eq_points(point, rho, p)
            if implicit:
                ok = S.verify(claim_n + lam * claim_d, rounds, rho, [e, d1, d0], terms_ones(lam), p)
            else:
                ok = S.verify(claim_n + lam * claim_d, rounds, rho, [e, n0, d1, n1, d0], terms(lam), p)
            if not ok:
                return bad
            point = list(rho)
        tau = challenge(k, None, list(values)) % p
        point = (point or []) + [tau]
        claim_n, claim_d = (n0 + tau * (n1 - n0)) % p, (d0 + tau * (d1 - d0)) % p
    return True, point, claim_n, claim_d


def _tag(rnd):
    return 255 if rnd is None else 254 if rnd == LAMBDA else rnd


def hash_challenge(p, seed=b"fraction-sum"):
    """A deterministic stand-in for the verifier, as grand_product_ref.hash_challenge: the element from a hash of the layer,
    the round (255 for the layer's tau, 254 for its lambda) and the values as the Montgomery limbs the device returns.
    -> (challenge over limbs -> limbs, challenge over canonical -> canonical)"""
    def of_limbs(layer, rnd, values):
        h = hashlib.sha256(seed + bytes([layer, _tag(rnd)]) + np.ascontiguousarray(values, dtype="<u8").tobytes()).digest()
        return int.from_bytes(h + hashlib.sha256(h).digest()[:8], "little") % p

    def device(layer, rnd, values):
        return pyref.to_mont(of_limbs(layer, rnd, values), p)

    def model(layer, rnd, values):
        return of_limbs(layer, rnd, S.encode(values, p) if len(values) else np.zeros((0, 4), dtype=np.uint64))
    return device, model


def decode_proof(proof, p):
    """a device FractionalSumProof (Montgomery limbs) -> ((P, Q), layers, point) in the model's canonical form"""
    layers = []
    for sc, values in proof.layers:
        layers.append((None if sc is None else ([S.decode(g, p) for g in sc.rounds], S.decode(sc.point, p)), tuple(S.decode(values, p))))
    return tuple(S.decode(np.asarray(proof.root).reshape(2, 4), p)), layers, S.decode(proof.point, p)


LOOKUP_SEEDS = (41, 42, 43)      # table values, lookup indices, gamma


def lookup_case(p):
    """t: 2^6 distinct canonical values; idx: 2^9 indices into it; gamma; and a value outside the table"""
    rng = np.random.default_rng(LOOKUP_SEEDS[0])
    t = []
    while len(t) < 64:
        v = int.from_bytes(rng.bytes(40), "little") % p
        if v not in t:
            t.append(v)
    idx = np.random.default_rng(LOOKUP_SEEDS[1]).integers(0, 64, size=512, dtype=np.uint32)
    grng = np.random.default_rng(LOOKUP_SEEDS[2])
    gamma = int.from_bytes(grng.bytes(40), "little") % p
    outside = int.from_bytes(grng.bytes(40), "little") % p
    return t, idx, gamma, outside
