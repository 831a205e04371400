"""The model of the Merkle commitments (include/ark_hip.h): hashlib's SHA3-256 over byte strings built from
Python integers.  No code of the library is used.

    leaf(i) = H( u32_le(count) | u32_le(elem_bytes) | ser(col_0[i]) | .. | ser(col_{count-1}[i]) )
    node    = H( u32_le(0xFFFFFFFF) | u32_le(0) | left | right )
    tree    2n - 1 digests, node t at index t, root 0, children 2t + 1 and 2t + 2, leaf i at n - 1 + i

A one-word element is serialised as its stored word (little-endian, 4 or 8 bytes); an Fr element, given as its Montgomery residue,
as the canonical value x * R^-1 mod p in 32 little-endian bytes."""
import hashlib
import random

SMALL = {   # name: (id, element bytes, modulus)
    "GOLDILOCKS": (0, 8, 2**64 - 2**32 + 1),
    "BABYBEAR": (1, 4, 2**31 - 2**27 + 1),
    "KOALABEAR": (2, 4, 2**31 - 2**24 + 1),
}
FR = {      # name: (id, modulus)
    "BN254_FR": (1, 21888242871839275222246405745257275088548364400416034343698204186575808495617),
    "BLS12_381_FR": (3, 52435875175126190479447740508185965837690552500527637822603658699938581184513),
    "BLS12_377_FR": (5, 8444461749428370424248824938781546531375899335154063827935233455917409239041),
}
R256 = 1 << 256
RINV = {name: pow(R256, -1, p) for name, (_, p) in FR.items()}   # out of Montgomery form: x * R^-1 mod p
NODE_HEADER = (0xFFFFFFFF).to_bytes(4, "little") + (0).to_bytes(4, "little")


def H(data):
    return hashlib.sha3_256(data).digest()


def rng(seed):
    return random.Random(seed)


def elem_bytes(field):
    return SMALL[field][1] if field in SMALL else 32


def modulus(field):
    return SMALL[field][2] if field in SMALL else FR[field][1]


def ser(field, x):
    """the bytes of one element given in memory form"""
    if field in SMALL:
        return int(x).to_bytes(SMALL[field][1], "little")
    return (int(x) * RINV[field] % FR[field][1]).to_bytes(32, "little")


def leaf_message(field, row):
    return len(row).to_bytes(4, "little") + elem_bytes(field).to_bytes(4, "little") + b"".join(ser(field, x) for x in row)


def leaf(field, row):
    return H(leaf_message(field, row))


def node(left, right):
    return H(NODE_HEADER + left + right)


def tree(field, columns):
    """columns: count lists of n = 2^k integers -> the 2n - 1 digests"""
    n = len(columns[0])
    assert n and not n & (n - 1) and all(len(c) == n for c in columns)
    t = [None] * (2 * n - 1)
    for i in range(n):
        t[n - 1 + i] = leaf(field, [c[i] for c in columns])
    for j in range(n - 2, -1, -1):
        t[j] = node(t[2 * j + 1], t[2 * j + 2])
    return t


def path(t, index):
    """the siblings of leaf `index` from the leaf level upwards"""
    n = (len(t) + 1) // 2
    j, out = n - 1 + index, []
    while j:
        out.append(t[j + 1] if j & 1 else t[j - 1])
        j = (j - 1) // 2
    return out


def verify(field, root, n, index, row, pth):
    k = n.bit_length() - 1
    if len(pth) != k or not 0 <= index < n:
        return False
    cur = leaf(field, row)
    for sib in pth:
        cur = node(sib, cur) if index & 1 else node(cur, sib)
        index >>= 1
    return cur == root


def leaf_permutations(count, eb):
    """Keccak permutations of one leaf: the message and at least the suffix byte, in blocks of 136"""
    return (8 + count * eb) // 136 + 1


def random_columns(field, r, count, n):
    p = modulus(field)
    return [[r.randrange(p) for _ in range(n)] for _ in range(count)]


def words64(x):
    """an Fr element as its four little-endian 64-bit words"""
    return [(int(x) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
