"""Host-side checks of the Merkle commitments (no GPU): the model of tests/merkle_ref.py against FIPS 202 known answers, the host
entries of the library (ark_hip_merkle_node / _leaf_* / _verify_* / _plan) against the model on both sides of every rate seam,
every argument error before a device is looked for, the names in the header, bindings and mirrors, and one pinned root."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib, merkle
import merkle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SIZE, ERR_NO_DEVICE = -1, -2, -5
SMALL, FR = list(R.SMALL), list(R.FR)
# counts whose message lengths lie on both sides of each 136-byte rate seam (8 + 4 count, 8 + 8 count, 8 + 32 count), including
# those that leave four or eight bytes in the block (31 / 15) and those whose padding takes a block of its own (32 / 16 / 4, 66 / 33)
COUNTS = {
    "BABYBEAR": [1, 2, 3] + list(range(29, 36)) + list(range(63, 68)) + [131, 132, 133],
    "KOALABEAR": [1, 2, 3] + list(range(29, 36)) + list(range(63, 68)) + [131, 132, 133],
    "GOLDILOCKS": [1] + list(range(14, 19)) + list(range(31, 36)),
    "BN254_FR": [1, 3, 4, 5, 8, 9, 20, 21, 22],
    "BLS12_381_FR": [1, 3, 4, 5, 8, 9, 20, 21, 22],
    "BLS12_377_FR": [1, 3, 4, 5, 8, 9, 20, 21, 22],
}


def fr_rows(values):
    return np.array([R.words64(v) for v in values], dtype=np.uint64)


def lib_leaf(field, row):
    return A.merkle_leaf_small(field, row) if field in R.SMALL else A.merkle_leaf_fr(field, fr_rows(row))


def lib_verify(field, root, n, index, row, path):
    row = row if field in R.SMALL else fr_rows(row)
    return A.MerkleTree.verify(field, root, n, index, row, np.frombuffer(b"".join(path), dtype=np.uint8))


def test_model_sha3_against_fips_202_known_answers():
    assert R.H(b"").hex() == "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"
    assert R.H(b"abc").hex() == "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532"
    assert R.NODE_HEADER == bytes([255, 255, 255, 255, 0, 0, 0, 0]) and len(R.NODE_HEADER + bytes(64)) == 72


def test_node_against_the_model():
    r = R.rng(1)
    for _ in range(50):
        a, b = r.randbytes(32), r.randbytes(32)
        assert A.merkle_node(a, b) == R.node(a, b)
    assert A.merkle_node(bytes(32), bytes(32)) == R.node(bytes(32), bytes(32))
    assert A.merkle_node(b"\xff" * 32, bytes(32)) != A.merkle_node(bytes(32), b"\xff" * 32)


@pytest.mark.parametrize("field", SMALL + FR)
def test_leaf_against_the_model_across_the_rate_seams(field):
    r = R.rng(2)
    p, eb = R.modulus(field), R.elem_bytes(field)
    lengths = set()
    for count in COUNTS[field]:
        for row in ([r.randrange(p) for _ in range(count)], [p - 1] * count, [0] * count):
            assert lib_leaf(field, row) == R.leaf(field, row), (field, count)
        lengths.add((8 + count * eb) % 136)
        assert A.merkle_plan(1, count, eb)["leaf_permutations"] == R.leaf_permutations(count, eb) == len(R.leaf_message(field, [0] * count)) // 136 + 1
    # the seams are really straddled: a message that ends with the block, one that leaves 4 (4-byte fields) or 8 bytes
    assert 0 in lengths and (136 - eb if eb < 32 else 104) in lengths, (field, lengths)


@pytest.mark.parametrize("field", FR)
def test_fr_leaves_of_the_special_elements(field):
    p = R.modulus(field)
    for row in ([0], [1], [p - 1], [R.R256 % p], [0, 1, p - 1, R.R256 % p]):
        assert lib_leaf(field, row) == R.leaf(field, row), (field, row)
    # the Montgomery residue R mod p is the canonical value 1: the leaf hashes 1, not the stored words
    one = (1).to_bytes(32, "little")
    assert R.ser(field, R.R256 % p) == one
    assert lib_leaf(field, [R.R256 % p]) == R.H((1).to_bytes(4, "little") + (32).to_bytes(4, "little") + one)


@pytest.mark.parametrize("field", ["BABYBEAR", "GOLDILOCKS", "BLS12_381_FR"])
def test_verify_accepts_model_openings_and_rejects_every_edit(field):
    r = R.rng(3)
    count = 3
    for n in (1, 2, 8, 1024):
        cols = R.random_columns(field, r, count, n)
        t = R.tree(field, cols)
        root = t[0]
        for index in sorted({0, n - 1, n // 2}):
            row = [c[index] for c in cols]
            pth = R.path(t, index)
            assert R.verify(field, root, n, index, row, pth)
            assert lib_verify(field, root, n, index, row, pth), (field, n, index)
            bad_row = list(row)
            bad_row[1] ^= 1
            assert not lib_verify(field, root, n, index, bad_row, pth)
            for lev in range(len(pth)):
                bad = list(pth)
                bad[lev] = bytes([pth[lev][0] ^ 0x10]) + pth[lev][1:]
                assert not lib_verify(field, root, n, index, row, bad), (field, n, index, lev)
            assert not lib_verify(field, root[:31] + bytes([root[31] ^ 0x80]), n, index, row, pth)
            if n > 1:
                assert not lib_verify(field, root, n, (index + 1) % n, row, pth)
                assert not lib_verify(field, root, n, index, row[:-1], pth), "a wrong count"
                assert not lib_verify(field, root, n, index, row, pth[:-1]), "a path of another n (the mirror refuses the length)"
                # the C entry itself with a smaller n and the path it would read
                half = n // 2
                assert not lib_verify(field, root, half, index % half, row, pth[:-1])
            assert not lib_verify(field, root, 2 * n, index, row, pth + [bytes(32)])


def test_plan_closed_forms_and_monotone_launches():
    prev = 0
    for log in range(33):
        n = 1 << log
        for eb, counts in ((4, (1, 2, 31, 32, 33, 64, 65, 1000, 2**32 - 2)), (8, (1, 15, 16, 17, 33, 300)), (32, (1, 4, 5, 9, 100))):
            for count in counts:
                pl = A.merkle_plan(n, count, eb)
                assert pl["tree_bytes"] == (2 * n - 1) * 32
                assert pl["leaf_permutations"] == (8 + count * eb) // 136 + 1
                assert pl["leaf_blocks"] == max(1, n // 256)
                assert 0 <= pl["tail_level"] <= 8 and 1 <= pl["levels_per_launch"] <= 9
        pl = A.merkle_plan(n, 1, 4)
        T, m = pl["tail_level"], pl["levels_per_launch"]
        want = 1 if log == 0 else 2 + -(-max(0, log - 1 - T) // m)
        assert pl["launches"] == want and pl["launches"] >= prev, (log, pl)
        assert (pl["node_blocks"] == 0) == (log - 1 <= T)
        if pl["node_blocks"]:
            assert pl["node_blocks"] == max(1, (n // 2) // 256)
        prev = pl["launches"]
    assert A.merkle_plan(1 << 20, 1, 4)["launches"] < 20, "a tree does not end in log n launches"


def test_argument_errors_come_before_any_device():
    """every ARK_HIP_ERR_ARG the header lists, with no GPU in reach: a call that got past its checks would answer
    ARK_HIP_ERR_NO_DEVICE on a CPU-only host, or touch the fake pointers on a GPU host"""
    L = _lib.lib()
    out8 = (C.c_uint64 * 8)()
    dig = (C.c_uint8 * 32)()
    ok = C.c_int(7)
    row = (C.c_uint64 * 8)()
    idx = (C.c_uint64 * 2)(0, 1)
    data, tree = C.c_void_p(0x100000), C.c_void_p(0x800000)
    rows_out, paths_out = (C.c_uint8 * 4096)(), (C.c_uint8 * 4096)()
    # plan
    assert L.ark_hip_merkle_plan(8, 1, 4, None) == ERR_ARG
    for n in (0, 3, 6, 1000):
        assert L.ark_hip_merkle_plan(n, 1, 4, out8) == ERR_ARG
    for count in (0, 2**32 - 1, 2**32):
        assert L.ark_hip_merkle_plan(8, count, 4, out8) == ERR_ARG
    for eb in (0, 1, 2, 16, 64):
        assert L.ark_hip_merkle_plan(8, 1, eb, out8) == ERR_ARG
    assert L.ark_hip_merkle_plan(8, 2**32 - 2, 4, out8) == 0
    # host hashing
    for bad in (-1, 3, 99):
        assert L.ark_hip_merkle_leaf_sfp(bad, row, 1, dig) == ERR_ARG
        assert L.ark_hip_merkle_verify_sfp(bad, dig, 1, 0, row, 1, None, C.byref(ok)) == ERR_ARG
        assert L.ark_hip_merkle_commit_sfp_device(bad, data, 1, 8, 8, tree, None) == ERR_ARG
    for bad in (-1, 0, 2, 4, 6, 99):   # the base fields are no scalar fields
        assert L.ark_hip_merkle_leaf_fr(bad, row, 1, dig) == ERR_ARG
        assert L.ark_hip_merkle_verify_fr(bad, dig, 1, 0, row, 1, None, C.byref(ok)) == ERR_ARG
        assert L.ark_hip_merkle_commit_fr_device(bad, data, 1, 8, 8, tree, None) == ERR_ARG
    assert L.ark_hip_merkle_node(None, dig, dig) == L.ark_hip_merkle_node(dig, None, dig) == L.ark_hip_merkle_node(dig, dig, None) == ERR_ARG
    for leaf, f in ((L.ark_hip_merkle_leaf_sfp, 1), (L.ark_hip_merkle_leaf_fr, 3)):
        assert leaf(f, None, 1, dig) == leaf(f, row, 1, None) == leaf(f, row, 0, dig) == leaf(f, row, 2**32 - 1, dig) == ERR_ARG
    for ver, f in ((L.ark_hip_merkle_verify_sfp, 1), (L.ark_hip_merkle_verify_fr, 3)):
        assert ver(f, None, 2, 0, row, 1, dig, C.byref(ok)) == ERR_ARG
        assert ver(f, dig, 2, 0, None, 1, dig, C.byref(ok)) == ERR_ARG
        assert ver(f, dig, 2, 0, row, 1, None, C.byref(ok)) == ERR_ARG
        assert ver(f, dig, 2, 0, row, 1, dig, None) == ERR_ARG
        assert ver(f, dig, 3, 0, row, 1, dig, C.byref(ok)) == ver(f, dig, 0, 0, row, 1, dig, C.byref(ok)) == ERR_ARG
        assert ver(f, dig, 2, 2, row, 1, dig, C.byref(ok)) == ERR_ARG, "an index >= n"
        assert ver(f, dig, 2, 0, row, 0, dig, C.byref(ok)) == ERR_ARG
        assert ver(f, dig, 1, 0, row, 1, None, C.byref(ok)) == 0 and ok.value == 0, "a wrong root is an answer, not an error"
    # commits
    for commit, f, eb in ((L.ark_hip_merkle_commit_sfp_device, 1, 4), (L.ark_hip_merkle_commit_sfp_device, 0, 8),
                          (L.ark_hip_merkle_commit_fr_device, 3, 32)):
        assert commit(f, None, 1, 8, 8, tree, None) == commit(f, data, 1, 8, 8, None, None) == ERR_ARG
        for n in (0, 3, 12):
            assert commit(f, data, 1, 16, n, tree, None) == ERR_ARG
        assert commit(f, data, 0, 8, 8, tree, None) == commit(f, data, 2**32 - 1, 8, 8, tree, None) == ERR_ARG
        assert commit(f, data, 2, 7, 8, tree, None) == ERR_ARG, "stride < n"
        assert commit(f, C.c_void_p(0x100000 + min(eb, 16) // 2), 1, 8, 8, tree, None) == ERR_ARG, "a misaligned matrix"
        assert commit(f, data, 1, 8, 8, C.c_void_p(0x800008), None) == ERR_ARG, "a misaligned tree"
        extent = (2 * 10 + 8) * eb   # three columns, stride 10
        for t in (0x100000, 0x100000 + ((extent - 1) & ~15), 0x100000 - 15 * 32 + 16):
            assert commit(f, data, 3, 10, 8, C.c_void_p(t), None) == ERR_ARG, ("the tree overlaps the matrix", hex(t))
    # open
    op = L.ark_hip_merkle_open_device
    assert op(None, 8, data, 4, 1, 8, idx, 2, rows_out, paths_out) == ERR_ARG
    assert op(tree, 6, data, 4, 1, 8, idx, 2, rows_out, paths_out) == op(tree, 0, data, 4, 1, 8, idx, 2, rows_out, paths_out) == ERR_ARG
    assert op(tree, 8, data, 5, 1, 8, idx, 2, rows_out, paths_out) == ERR_ARG
    assert op(tree, 8, data, 4, 0, 8, idx, 2, rows_out, paths_out) == op(tree, 8, data, 4, 2**32 - 1, 8, idx, 2, rows_out, paths_out) == ERR_ARG
    assert op(tree, 8, data, 4, 1, 7, idx, 2, rows_out, paths_out) == ERR_ARG
    assert op(tree, 8, data, 4, 1, 8, None, 2, rows_out, paths_out) == ERR_ARG
    assert op(tree, 8, data, 4, 1, 8, idx, 2, rows_out, None) == ERR_ARG
    assert op(tree, 8, None, 4, 1, 8, idx, 2, rows_out, paths_out) == ERR_ARG, "out_rows without d_data"
    assert op(tree, 8, data, 4, 1, 8, idx, 2, None, paths_out) == ERR_ARG
    assert op(tree, 8, data, 4, 1, 8, (C.c_uint64 * 2)(0, 8), 2, rows_out, paths_out) == ERR_ARG, "an index >= n"
    assert op(tree, 2, None, 4, 1, 2, (C.c_uint64 * 2)(1, 2), 2, None, paths_out) == ERR_ARG
    assert L.ark_hip_merkle_plan(1 << 41, 1, 4, out8) == ERR_SIZE


def test_without_a_gpu_the_device_entries_say_so():
    L = _lib.lib()
    if L.ark_hip_device_count() > 0:
        pytest.skip("a GPU is visible here")
    data, tree = C.c_void_p(0x100000), C.c_void_p(0x800000)
    idx = (C.c_uint64 * 1)(0)
    out = (C.c_uint8 * 256)()
    assert L.ark_hip_merkle_commit_sfp_device(1, data, 1, 8, 8, tree, None) == ERR_NO_DEVICE
    assert L.ark_hip_merkle_commit_fr_device(3, data, 1, 8, 8, tree, None) == ERR_NO_DEVICE
    assert L.ark_hip_merkle_open_device(tree, 8, None, 4, 1, 8, idx, 1, None, out) == ERR_NO_DEVICE
    assert L.ark_hip_merkle_open_device(tree, 8, None, 4, 1, 8, idx, 0, None, out) == ERR_NO_DEVICE


def test_header_exports_bindings_and_mirrors_name_the_same_entries():
    hdr = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    declared = set(re.findall(r"\b(ark_hip_merkle_[a-z0-9_]+)\s*\(", hdr))
    want = {"ark_hip_merkle_" + s for s in ("commit_sfp_device", "commit_fr_device", "open_device", "leaf_sfp", "leaf_fr", "node", "verify_sfp",
                                            "verify_fr", "plan")}
    assert declared == want
    assert "#define ARK_HIP_MERKLE_DIGEST_BYTES 32" in hdr
    bound = {s for s in _lib.SYMBOLS if s.startswith("ark_hip_merkle_")}
    assert bound == declared and not [s for s in _lib.TEST_SYMBOLS if "merkle" in s]
    for name in declared:
        arity = len(re.search(r"\b%s\s*\(([^;]*?)\);" % name, hdr, re.S).group(1).split(","))
        assert len(_lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(_lib.lib(), name), name
    assert "ark_hip_*" in open(os.path.join(ROOT, "algebra_amd", "csrc", "exports.map")).read()
    py = open(os.path.join(ROOT, "algebra_amd", "merkle.py")).read()
    cpp = open(os.path.join(ROOT, "include", "ark_hip.hpp")).read()
    for mirror, text in (("merkle.py", py), ("ark_hip.hpp", cpp)):
        used = set(re.findall(r"\b(ark_hip_merkle_[a-z0-9_]+)\s*\(", text))
        assert used == declared, (mirror, used ^ declared)
        assert "class MerkleTree" in text
    for owner, text in (("smallfp.py", "SmallDeviceMatrix"), ("smallfp.py", "SmallDeviceVec"), ("poly.py", "DeviceVec"),
                        ("mle.py", "DenseMultilinearExtension")):
        src = open(os.path.join(ROOT, "algebra_amd", owner)).read()
        body = src[src.index("class " + text):]
        assert re.search(r"\n    def commit\(self", body), (owner, text)
    assert merkle.DIGEST_BYTES == 32


def test_pinned_root_of_a_small_babybear_matrix():
    """three columns of eight small integers, as stored words: column j holds 8 j + i + 1.  The literal keeps the definition from
    drifting together with the model."""
    cols = [[8 * j + i + 1 for i in range(8)] for j in range(3)]
    t = R.tree("BABYBEAR", cols)
    assert t[0].hex() == PINNED_ROOT
    assert R.leaf_message("BABYBEAR", [1, 9, 17]) == bytes([3, 0, 0, 0, 4, 0, 0, 0, 1, 0, 0, 0, 9, 0, 0, 0, 17, 0, 0, 0])
    # the library agrees leaf by leaf and node by node, without a device
    lv = [A.merkle_leaf_small("BABYBEAR", [c[i] for c in cols]) for i in range(8)]
    assert lv == t[7:]
    while len(lv) > 1:
        lv = [A.merkle_node(lv[2 * i], lv[2 * i + 1]) for i in range(len(lv) // 2)]
    assert lv[0].hex() == PINNED_ROOT


PINNED_ROOT = "c794521b17097267e84bf5ea8648096eca974d7d6e115b94f228415c4d62b166"
