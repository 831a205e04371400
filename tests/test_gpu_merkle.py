"""The Merkle commitments (ark_hip_merkle_commit_*_device / _open_device) on the GPU against the hashlib model of
tests/merkle_ref.py: whole trees byte for byte at every size across the seams that ark_hip_merkle_plan reports, strided matrices
with guards, long rows, the asynchronous form, openings, a low-degree extension committed and opened without a download, a
multilinear table, poisoned scratch (a child process)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import algebra_amd as A
from algebra_amd import _lib
import merkle_ref as R
import smallfp_ref as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"BABYBEAR": (1, 2, 31, 32, 33), "KOALABEAR": (1, 2, 31, 32, 33), "GOLDILOCKS": (1, 15, 16, 17),
          "BN254_FR": (1, 4, 5), "BLS12_381_FR": (1, 4, 5), "BLS12_377_FR": (1, 4, 5)}
GUARD = 64


def field_id(field):
    return R.SMALL[field][0] if field in R.SMALL else R.FR[field][0]


def words_per_element(field):
    return 1 if field in R.SMALL else 4


def word_dtype(field):
    return np.uint32 if R.elem_bytes(field) == 4 else np.uint64


def sizes():
    """log n: 0 .. four levels past the tail threshold, and the first size with a second multi-level launch"""
    pl = A.merkle_plan(1, 1, 4)
    T, m = pl["tail_level"], pl["levels_per_launch"]
    past = T + 1 + 4
    second = T + 1 + m + 1
    assert second <= 15
    assert A.merkle_plan(1 << second, 1, 4)["launches"] == 4 and A.merkle_plan(1 << (second - 1), 1, 4)["launches"] == 3
    assert A.merkle_plan(1 << (T + 1), 1, 4)["launches"] == 2 and A.merkle_plan(1 << (T + 2), 1, 4)["launches"] == 3
    return list(range(0, past + 1)) + ([second] if second > past else [])


@functools.lru_cache(maxsize=None)
def random_pool(field):
    """40 columns of 2^14 random elements that every matrix of the sweep is cut from"""
    p = R.modulus(field)
    r = R.rng(28 + field_id(field))
    bits = p.bit_length() + 8
    return [[r.getrandbits(bits) % p for _ in range(1 << 14)] for _ in range(40)]


@functools.lru_cache(maxsize=None)
def base_columns(field, count, n):
    """count columns of n elements (memory form, Python integers): random, with 0 / p - 1 on both sides of every wave (64) and
    workgroup (256) boundary"""
    p = R.modulus(field)
    cols = [list(c[:n]) for c in random_pool(field)[:count]] if count <= 40 and n <= 1 << 14 else R.random_columns(field, R.rng(count), count, n)
    for j, c in enumerate(cols):
        for b in range(64, n, 64):
            c[b - 1], c[b] = (0, p - 1) if (j + b // 64) & 1 else (p - 1, 0)
        c[0], c[n - 1] = p - 1, (0 if n > 1 else p - 1)
    return tuple(tuple(c) for c in cols)


@functools.lru_cache(maxsize=None)
def model_tree(field, count, n):
    return R.tree(field, [list(c) for c in base_columns(field, count, n)])


def to_words(field, cols, stride):
    """[count, stride * words] array of the matrix with the gaps behind every column filled with 0xFF bytes"""
    w, dt = words_per_element(field), word_dtype(field)
    out = np.full((len(cols), stride * w), np.iinfo(dt).max, dtype=dt)
    for j, c in enumerate(cols):
        vals = c if w == 1 else [x for v in c for x in R.words64(v)]
        out[j, :len(c) * w] = np.array(vals, dtype=dt)
    return out


class DeviceBytes:
    def __init__(self, host):
        self.host = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.p = C.c_void_p()
        A._lib.check(_lib.lib().ark_hip_malloc(max(self.host.size, 16), C.byref(self.p)), "ark_hip_malloc")
        if self.host.size:
            A._lib.check(_lib.lib().ark_hip_memcpy_h2d(self.p, self.host.ctypes.data_as(C.c_void_p), self.host.size), "ark_hip_memcpy_h2d")

    def read(self):
        out = np.empty_like(self.host)
        if out.size:
            A._lib.check(_lib.lib().ark_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.p, out.size), "ark_hip_memcpy_d2h")
        return out

    def __del__(self):
        try:
            _lib.lib().ark_hip_free(self.p)
        except Exception:  # noqa: BLE001
            pass


def commit_raw(field, data, count, stride, n, tree, out_root=None):
    L = _lib.lib()
    entry = L.ark_hip_merkle_commit_sfp_device if field in R.SMALL else L.ark_hip_merkle_commit_fr_device
    root = None if out_root is None else out_root.ctypes.data_as(C.c_void_p)
    A._lib.check(entry(field_id(field), data.p, count, stride, n, tree.p, root), "commit")


def check_commit(field, count, n, stride):
    cols = base_columns(field, count, n)
    want = b"".join(model_tree(field, count, n))
    data = DeviceBytes(to_words(field, cols, stride))
    tree = DeviceBytes(np.full(len(want) + GUARD, 0xFF, dtype=np.uint8))
    root = np.zeros(32, dtype=np.uint8)
    commit_raw(field, data, count, stride, n, tree, root)
    got = tree.read()
    assert got[:len(want)].tobytes() == want, (field, count, n, stride, "the tree")
    assert root.tobytes() == want[:32], (field, count, n, stride, "the root")
    assert (got[len(want):] == 0xFF).all(), (field, count, n, stride, "the guard behind the tree")
    assert np.array_equal(data.read(), data.host), (field, count, n, stride, "the matrix and its gaps")


@pytest.mark.parametrize("gap", [0, 3])
@pytest.mark.parametrize("field", list(COUNTS))
def test_whole_trees_across_the_seams(field, gap):
    for log in sizes():
        n = 1 << log
        for count in COUNTS[field]:
            if gap and log % 3 != 1 and count != COUNTS[field][-1]:
                continue   # the strided form at every size for the widest row, at every third size for the others
            check_commit(field, count, n, n + gap)


@pytest.mark.parametrize("field,count,n", [("BABYBEAR", 1000, 64), ("KOALABEAR", 300, 256), ("GOLDILOCKS", 300, 256), ("BLS12_381_FR", 40, 64)])
def test_long_rows(field, count, n):
    assert A.merkle_plan(n, count, R.elem_bytes(field))["leaf_permutations"] >= 9
    check_commit(field, count, n, n + 1)


@pytest.mark.parametrize("knobs", [(0, 0, 1), (1, 0, 1), (0, 3, 2), (1, 8, 9), (1, 5, 3), (0, 8, 4)])
def test_both_permutations_and_other_seams_give_the_same_trees(knobs, monkeypatch):
    """the measurement knobs (the permutation variant, the tail's first level, levels per launch) change how a tree is computed,
    never the tree; the plan follows them"""
    perm, tail, levels = knobs
    monkeypatch.setenv("ARK_HIP_MERKLE_PERM", str(perm))
    monkeypatch.setenv("ARK_HIP_MERKLE_TAIL_LOG", str(tail))
    monkeypatch.setenv("ARK_HIP_MERKLE_LEVELS", str(levels))
    pl = A.merkle_plan(1 << 12, 1, 4)
    assert (pl["permutation"], pl["tail_level"], pl["levels_per_launch"]) == knobs
    assert pl["launches"] == 2 + -(-(11 - tail) // levels)
    for field, count in (("BABYBEAR", 33), ("GOLDILOCKS", 16), ("BLS12_377_FR", 5)):
        for log in (0, 1, 5, 9, 12):
            check_commit(field, count, 1 << log, (1 << log) + 3)


def test_two_asynchronous_commits_then_one_wait():
    n = 1 << 11
    ca, cb = base_columns("BABYBEAR", 2, n), base_columns("GOLDILOCKS", 15, n)
    da, db = DeviceBytes(to_words("BABYBEAR", ca, n)), DeviceBytes(to_words("GOLDILOCKS", cb, n))
    ta, tb = (DeviceBytes(np.zeros((2 * n - 1) * 32, dtype=np.uint8)) for _ in range(2))
    commit_raw("BABYBEAR", da, 2, n, n, ta)
    commit_raw("GOLDILOCKS", db, 15, n, n, tb)
    A._lib.check(_lib.lib().ark_hip_synchronize(), "ark_hip_synchronize")
    assert ta.read().tobytes() == b"".join(model_tree("BABYBEAR", 2, n))
    assert tb.read()[:32].tobytes() == model_tree("GOLDILOCKS", 15, n)[0]
    # the mirror's asynchronous form reads the root from the tree
    v = A.SmallDeviceVec.from_host("BABYBEAR", np.array(ca[0], dtype=np.uint32))
    t = v.commit(wait=False)
    assert t.root == model_tree_of_one("BABYBEAR", ca[0])[0]


def model_tree_of_one(field, col):
    return R.tree(field, [list(col)])


@pytest.mark.parametrize("field,count,log", [("BABYBEAR", 5, 10), ("GOLDILOCKS", 3, 9), ("BN254_FR", 2, 9), ("KOALABEAR", 1, 0)])
def test_open_rows_and_paths(field, count, log):
    n = 1 << log
    cols = base_columns(field, count, n)
    t = model_tree(field, count, n)
    small = field in R.SMALL
    if small:
        mat = A.SmallDeviceMatrix.from_host(field, np.array(cols, dtype=word_dtype(field)))
        tree = mat.commit()
    else:
        flat = np.array([R.words64(v) for c in cols for v in c], dtype=np.uint64)
        tree = A.MerkleTree.commit_fr(field, (A.DeviceVec.from_host(field, flat), count))
    assert tree.root == t[0] and tree.to_host().tobytes() == b"".join(t)
    r = R.rng(77 + log)
    for q in (0, 1, 63, 64, 65, 300):
        idx = [r.randrange(n) for _ in range(q)]
        if q >= 63:
            idx[:6] = [0, n - 1, n - 1, 0, n // 2, n // 2]
            idx[10:30] = sorted(idx[10:30], reverse=True)
        elif q == 1:
            idx = [n - 1]
        rows, paths = tree.open(idx)
        assert paths.shape == (q, log, 32) and rows.shape[:2] == (q, count)
        for i, ix in enumerate(idx):
            want_row = [c[ix] for c in cols]
            got_row = rows[i].tolist() if small else [sum(int(w) << (64 * j) for j, w in enumerate(e)) for e in rows[i]]
            assert got_row == want_row, (field, q, i, ix)
            assert paths[i].tobytes() == b"".join(R.path(t, ix)), (field, q, i, ix)
            assert A.MerkleTree.verify(field, tree.root, n, ix, rows[i], paths[i]), (field, q, i, ix)
            if i == 0 and log:
                assert not A.MerkleTree.verify(field, tree.root, n, ix ^ 1, rows[i], paths[i])
    # paths only
    idx = [n - 1, 0, n // 3]
    rows, paths = tree.open(idx, rows=False)
    assert rows is None and [p.tobytes() for p in paths] == [b"".join(R.path(t, ix)) for ix in idx]


def test_extension_committed_and_opened_without_a_download():
    """8 BabyBear columns of 2^10 coefficients -> their evaluations on the coset of 2^12 -> commit -> 16 transcript-chosen rows:
    the rows are the model's Horner values at the coset points and their paths lead to the root.  The matrix never leaves the
    device."""
    f = SF.FIELDS["BABYBEAR"]
    big = 1 << 12
    coeffs = np.random.default_rng(2812).integers(0, f.p, size=(8, 1 << 10), dtype=np.uint64).astype(np.uint32)
    mat = A.SmallDeviceMatrix.from_host("BABYBEAR", coeffs, stride=big)
    model_dom = f.get_coset(f.domain_new(big), f.gen)
    mat.fft_in_place(A.SmallRadix2EvaluationDomain.new("BABYBEAR", big).get_coset(f.gen), num_coeffs=1 << 10)
    tree = mat.commit()
    ts = A.Transcript("BLS12_381_FR", tree.root)
    idx = [int(ts.challenge()[0]) % big for _ in range(16)]
    assert len(set(idx)) > 8
    rows, paths = tree.open(idx)
    for i, ix in enumerate(idx):
        point = f.domain_element(model_dom, ix)
        assert rows[i].tolist() == [f.horner(coeffs[c].tolist(), point) for c in range(8)], (i, ix)
        assert A.MerkleTree.verify("BABYBEAR", tree.root, big, ix, rows[i], paths[i])
        assert R.verify("BABYBEAR", tree.root, big, ix, rows[i].tolist(), [p.tobytes() for p in paths[i]])


def test_multilinear_table_committed_and_two_entries_opened():
    field, nv = "BLS12_381_FR", 12
    p = R.modulus(field)
    r = R.rng(12)
    vals = [r.getrandbits(300) % p for _ in range(1 << nv)]
    vals[0], vals[-1] = p - 1, R.R256 % p
    mle = A.DenseMultilinearExtension.from_evaluations(field, nv, np.array([R.words64(v) for v in vals], dtype=np.uint64))
    tree = mle.commit()
    t = R.tree(field, [vals])
    assert tree.root == t[0]
    idx = [(1 << nv) - 1, 1234]
    rows, paths = tree.open(idx)
    for i, ix in enumerate(idx):
        assert rows[i].tolist() == [R.words64(vals[ix])]
        assert paths[i].tobytes() == b"".join(R.path(t, ix))
        assert A.MerkleTree.verify(field, t[0], 1 << nv, ix, rows[i], paths[i])


def test_poisoned_scratch():
    """DESIGN.md section 16 for the staging buffer of ark_hip_merkle_open_device, in a fresh child process against libark_hip_test.so"""
    env = dict(os.environ, ARK_HIP_LIB=os.path.join(ROOT, "algebra_amd", "libark_hip_test.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "merkle_scratch_child.py")], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok") == 3, out.stdout
