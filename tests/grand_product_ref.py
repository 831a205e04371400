"""Big-integer model of the grand-product entries and of the layered proof around them, on Python
integers modulo p, on top of tests/mle_ref.py and tests/sumcheck_ref.py whose conventions it keeps (index bit 0 is the first
variable).  A product is not linear in R, so the model works on CANONICAL values (sumcheck_ref.decode / encode).

The tree pairs over the LAST variable: L_nu = the table, L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k], L_0 = [P]; in the buffer of
2^nu - 1 elements level j = L_{nu-j} lies at element 2^nu - 2^(nu-j+1), the layout of the opening quotients."""
import hashlib

import numpy as np

import mle_open_ref
import pyref
import sumcheck_ref as S

TERMS = [(1, [0, 1, 2])]          # the one product eq * left * right of a layer's sumcheck


def level_offset(num_vars, j):
    """element offset of level j (1 <= j <= num_vars) in the tree buffer"""
    return (1 << num_vars) - (1 << (num_vars - j + 1))


def level_len(num_vars, j):
    return 1 << (num_vars - j)


def levels(table, p):
    """[L_nu = table, L_{nu-1}, .., L_0 = [P]]: entry j is level j"""
    assert len(table) & (len(table) - 1) == 0
    out = [list(table)]
    while len(out[-1]) > 1:
        up, h = out[-1], len(out[-1]) // 2
        out.append([up[i] * up[i + h] % p for i in range(h)])
    return out


def tree(table, p):
    """(P, the 2^nu - 1 elements of the tree buffer)"""
    lv = levels(table, p)
    return lv[-1][0], [v for level in lv[1:] for v in level]


def lincomb(tables, coeffs, c0, p):
    """[c0 + sum_k coeffs[k] tables[k][i]]: the fingerprints"""
    return [(c0 + sum(c * t[i] for c, t in zip(coeffs, tables))) % p for i in range(len(tables[0]))]


def eq_points(a, b, p):
    """eq(a, b) = prod_i (a_i b_i + (1 - a_i)(1 - b_i))"""
    w = 1
    for x, y in zip(a, b):
        w = w * (x * y + (1 - x) * (1 - y)) % p
    return w


def prove(table, challenge, p):
    """the honest prover on the model: -> (P, layers, point); layers[k] = (None | (rounds, rho), (left, right)), canonical.
    challenge(layer, round or None, values) -> element"""
    nu = (len(table) - 1).bit_length()
    lv = levels(table, p)
    product = lv[-1][0]
    if nu == 0:
        return product, [], []
    pair = (lv[nu - 1][0], lv[nu - 1][1])
    point = [challenge(0, None, list(pair)) % p]
    layers = [(None, pair)]
    for k in range(1, nu):
        up, h = lv[nu - k - 1], 1 << k           # L_(k+1)
        tables = [mle_open_ref.eq_table(point, 1, p), up[:h], up[h:]]
        rounds, rho, finals, _ = S.prove(tables, TERMS, lambda i, g, k=k: challenge(k, i, g), p)
        pair = (finals[1], finals[2])
        tau = challenge(k, None, list(pair)) % p
        point = rho + [tau]
        layers.append(((rounds, rho), pair))
    return product, layers, point


def verify(num_vars, product, layers, challenge, p):
    """The verifier of the whole layered proof: -> (accepted, point r_nu, the claim about f(r_nu)).  It checks L_1[0] L_1[1] =
    P, every layer's sumcheck through sumcheck_ref's verifier with its own challenges -- the last round against
    eq(r_k, rho) left right --, and forms each next claim left + tau (right - left)."""
    bad = (False, None, None)
    if len(layers) != num_vars:
        return bad
    if num_vars == 0:
        return True, [], product % p
    sc, (left, right) = layers[0]
    if sc is not None or left * right % p != product % p:
        return bad
    tau = challenge(0, None, [left, right]) % p
    point, claim = [tau], (left + tau * (right - left)) % p
    for k in range(1, num_vars):
        sc, (left, right) = layers[k]
        if sc is None:
            return bad
        rounds, rho = sc
        if len(rounds) != k or len(rho) != k:
            return bad
        if any(r % p != challenge(k, i, g) % p for i, (g, r) in enumerate(zip(rounds, rho))):
            return bad                             # the prover's point is not the transcript's
        if not S.verify(claim, rounds, rho, [eq_points(point, rho, p), left, right], TERMS, p):
            return bad
        tau = challenge(k, None, [left, right]) % p
        point, claim = list(rho) + [tau], (left + tau * (right - left)) % p
    return True, point, claim


def hash_challenge(p, seed=b"grand-product"):
    """A deterministic stand-in for the verifier, as sumcheck_ref.hash_challenge: the element from a hash of the layer, the
    round (255 for the layer's tau) and the values as the Montgomery limbs the device returns.
    -> (challenge over limbs -> limbs, challenge over canonical -> canonical)"""
    def of_limbs(layer, rnd, values):
        tag = bytes([layer, 255 if rnd is None else rnd])
        h = hashlib.sha256(seed + tag + np.ascontiguousarray(values, dtype="<u8").tobytes()).digest()
        return int.from_bytes(h + hashlib.sha256(h).digest()[:8], "little") % p

    def device(layer, rnd, values):
        return pyref.to_mont(of_limbs(layer, rnd, values), p)

    def model(layer, rnd, values):
        return of_limbs(layer, rnd, S.encode(values, p))
    return device, model


def decode_proof(proof, p):
    """a device GrandProductProof (Montgomery limbs) -> (P, layers, point) in the model's canonical form"""
    layers = []
    for sc, pair in proof.layers:
        l, r = S.decode(pair, p)
        layers.append((None if sc is None else ([S.decode(g, p) for g in sc.rounds], S.decode(sc.point, p)), (l, r)))
    return S.decode(np.asarray(proof.product).reshape(1, 4), p)[0], layers, S.decode(proof.point, p)

