"""Times the Merkle commitments (ark_hip_merkle_commit_*_device, ark_hip_merkle_open_device) on device-resident matrices:

  BabyBear and Goldilocks: count x n = 64 x 2^20, 256 x 2^18, 1 x 2^24, and the 4x extension of 64 x 2^18 followed by its commit;
  BLS12-381 Fr: 1 x 2^24 and 8 x 2^20;
  open of 64 and 4096 indices,

next to three yardsticks measured in the same run: (a) the device-to-host copy of the matrix into pinned memory -- the floor of the
host route, whose hashing is not counted; (b) a device copy of the matrix; (c) the transform that produced it.

Both permutations are timed interleaved (ARK_HIP_MERKLE_PERM = 0: keccak_f1600 as the transcript has it, 1: merkle_f1600), and on
one node-bound tree the two seams of the node levels are swept (ARK_HIP_MERKLE_TAIL_LOG, ARK_HIP_MERKLE_LEVELS).  The one condition
(DESIGN.md section 28): at every case of at least 2^24 elements in total, commit (the default permutation) is faster than the
device-to-host copy of the same matrix by more than the two recorded spreads.

Every timed result is checked first: both permutations give one root; at 64 sampled indices the opened row equals the host copy of
the matrix, hashlib's leaf of it is the tree's leaf, and the opened path leads to the root through hashlib's nodes.

Timing: the wall clock around `reps` queued calls between two ark_hip_synchronize(), after warm-up calls, repeated ROUNDS times with
the variants interleaved; the JSON keeps the median and the spread (max - min).

    python tools/bench_merkle.py [--out profiles/merkle.json] [--quick]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import algebra_amd as A  # noqa: E402
from algebra_amd._lib import check, lib  # noqa: E402
import merkle_ref as M  # noqa: E402
import smallfp_ref as R  # noqa: E402

ROUNDS = 5
FR = "BLS12_381_FR"
# vector instructions of one compiled round in the gfx950 ISA of csrc/merkle.cuh's leaf kernels (hipcc --save-temps; every one of
# them a 32-bit operation on half a lane except the 29 64-bit shifts of variant 0)
VALU_PER_ROUND = {0: 288, 1: 260}


def rounds(variants, reps, warm=2):
    L = lib()
    out = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warm):
            fn()
    check(L.ark_hip_synchronize(), "sync")
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            check(L.ark_hip_synchronize(), "sync")
            out[name].append((time.perf_counter() - t0) * 1e3 / reps)
    return {k: (round(statistics.median(v), 5), round(max(v) - min(v), 5)) for k, v in out.items()}


def with_env(fn, **env):
    """fn with the measurement knobs set for the duration of the call (the library reads them on every call)"""
    def run():
        for k, v in env.items():
            os.environ[k] = str(v)
        try:
            return fn()
        finally:
            for k in env:
                del os.environ[k]
    return run


class Pinned:
    def __init__(self, nbytes):
        self.p = C.c_void_p()
        check(lib().ark_hip_host_alloc(nbytes, C.byref(self.p)), "host_alloc")

    def free(self):
        check(lib().ark_hip_host_free(self.p), "host_free")


def check_tree(field, tree, host, count, n, stride, rng):
    """64 sampled openings against the host copy of the matrix and hashlib"""
    small = field in M.SMALL
    idx = [0, n - 1] + [int(i) for i in rng.integers(0, n, size=62)]
    rows, paths = tree.open(idx)
    root = tree.root
    leaves = np.empty((len(idx), 32), dtype=np.uint8)
    for i, ix in enumerate(idx):
        if small:
            want = [int(host[c * stride + ix]) for c in range(count)]
            assert rows[i].tolist() == want, (field, "row", ix)
        else:
            want = [sum(int(w) << (64 * j) for j, w in enumerate(host[c * stride + ix])) for c in range(count)]
            assert [sum(int(w) << (64 * j) for j, w in enumerate(e)) for e in rows[i]] == want, (field, "row", ix)
        assert M.verify(field, root, n, ix, want, [p.tobytes() for p in paths[i]]), (field, "path", ix)
        check(lib().ark_hip_memcpy_d2h(leaves[i].ctypes.data_as(C.c_void_p), C.c_void_p(tree.device_ptr + 32 * (n - 1 + ix)), 32), "d2h")
        assert leaves[i].tobytes() == M.leaf(field, want), (field, "leaf", ix)


def commit_case(name, field, data_vec, host, count, n, stride, transform, rng, reps):
    """one matrix: both permutations against the three yardsticks"""
    L = lib()
    small = field in M.SMALL
    eb = M.elem_bytes(field)
    nbytes = count * stride * eb
    trees = {}
    for perm in (0, 1):
        make = (lambda: A.MerkleTree.commit_small(data_vec, n=n)) if small else (lambda: A.MerkleTree.commit_fr(field, (data_vec, count)))
        trees[perm] = with_env(make, ARK_HIP_MERKLE_PERM=perm)()
    assert trees[0].root == trees[1].root, (name, "the two permutations disagree")
    for t in trees.values():
        check_tree(field, t, host, count, n, stride, rng)
    tree = trees[1]
    trees[0].free()
    ptr = (data_vec.vec._p if hasattr(data_vec, "vec") else data_vec._p) if small else data_vec.ptr
    fid = tree.field
    entry = L.ark_hip_merkle_commit_sfp_device if small else L.ark_hip_merkle_commit_fr_device

    def commit():
        check(entry(fid, ptr, count, stride, n, tree._tree, None), "commit")

    pin = Pinned(nbytes)
    other = C.c_void_p()
    check(L.ark_hip_malloc(nbytes, C.byref(other)), "malloc")
    variants = {
        "commit_perm0": with_env(commit, ARK_HIP_MERKLE_PERM=0),
        "commit_perm1": with_env(commit, ARK_HIP_MERKLE_PERM=1),
        "commit": commit,
        "d2h": lambda: check(L.ark_hip_memcpy_d2h(pin.p, ptr, nbytes), "d2h"),
        "d2d": lambda: check(L.ark_hip_memcpy_d2d(other, ptr, nbytes), "d2d"),
    }
    if transform:
        variants["transform"] = transform
    t = rounds(variants, reps)
    pin.free()
    check(L.ark_hip_free(other), "free")
    pl = A.merkle_plan(n, count, eb)
    perms = n * pl["leaf_permutations"] + (n - 1)
    row = {"case": name, "field": field, "count": count, "log_n": n.bit_length() - 1, "elements": count * n, "matrix_bytes": count * n * eb,
           "leaf_permutations": pl["leaf_permutations"], "permutations": perms, "launches": pl["launches"], "reps": reps, "rounds": ROUNDS,
           "default_permutation": pl["permutation"]}
    for k, (med, spread) in t.items():
        row[k + "_ms"], row[k + "_spread_ms"] = med, spread
    row["hashed_gb_per_s"] = round(136 * perms / (row["commit_ms"] * 1e-3) / 1e9, 1)
    row["lane_instructions_per_s"] = float("%.3g" % (perms * 24 * VALU_PER_ROUND[pl["permutation"]] / (row["commit_ms"] * 1e-3)))
    row["d2h_over_commit"] = round(row["d2h_ms"] / row["commit_ms"], 2)
    row["commit_over_d2d"] = round(row["commit_ms"] / row["d2d_ms"], 2)
    row["perm1_faster_beyond_spread"] = bool(row["commit_perm0_ms"] - row["commit_perm1_ms"] > row["commit_perm0_spread_ms"] + row["commit_perm1_spread_ms"])
    row["margin_ms"] = round(row["d2h_ms"] - row["commit_ms"] - row["d2h_spread_ms"] - row["commit_spread_ms"], 5)
    row["counts_for_the_condition"] = bool(count * n >= 1 << 24)
    row["faster_than_d2h_beyond_spread"] = bool(row["margin_ms"] > 0)
    print(json.dumps(row), flush=True)
    return row, tree


def open_case(tree, name, rng):
    out = []
    for q in (64, 4096):
        idx = rng.integers(0, tree.n, size=q, dtype=np.uint64)
        t = rounds({"open": lambda: tree.open(idx), "open_paths": lambda: tree.open(idx, rows=False)}, 20)
        out.append({"case": name, "q": q, "open_ms": t["open"][0], "open_spread_ms": t["open"][1], "open_paths_ms": t["open_paths"][0],
                    "open_paths_spread_ms": t["open_paths"][1]})
        print(json.dumps(out[-1]), flush=True)
    return out


def small_cases(f, quick, rng):
    dt = np.uint64 if f.bytes == 8 else np.uint32
    shapes = [(8, 12), (16, 10), (1, 14)] if quick else [(64, 20), (256, 18), (1, 24)]
    rows, opens = [], []
    for count, log in shapes:
        n = 1 << log
        host = rng.integers(0, f.p, size=count * n, dtype=np.uint64).astype(dt)
        mat = A.SmallDeviceMatrix(f.name, count, n)
        mat.vec.free()
        mat.vec = A.SmallDeviceVec.from_host(f.name, host)
        dom = A.SmallRadix2EvaluationDomain.new(f.name, n)
        row, tree = commit_case("%d x 2^%d" % (count, log), f.name, mat, host, count, n, n,
                                lambda: dom.fft_batch_in_place(mat.vec._p, count), rng, 3 if not quick else 10)
        rows.append(row)
        if count == shapes[0][0] and log == shapes[0][1]:
            opens = open_case(tree, "%s %d x 2^%d" % (f.name, count, log), rng)
        tree.free()
        mat.vec.free()
    # the 4x extension of `cols` columns, then its commit: evaluations on 2^slog -> the coset of 2^blog, in place
    cols, slog, blog = (8, 10, 12) if quick else (64, 18, 20)
    bn = 1 << blog
    host = np.zeros((cols, bn), dtype=dt)
    host[:, :1 << slog] = rng.integers(0, f.p, size=(cols, 1 << slog), dtype=np.uint64).astype(dt)
    mat = A.SmallDeviceMatrix.from_host(f.name, host)
    small, big = A.SmallRadix2EvaluationDomain.new(f.name, 1 << slog), A.SmallRadix2EvaluationDomain.new(f.name, bn).get_coset(f.gen)
    mat.low_degree_extend(small, big)
    ext = mat.vec.to_host()

    def lde():   # the timed transform runs on data that is no longer a set of evaluations: its work does not depend on the data
        mat.low_degree_extend(small, big)

    tree0 = mat.commit()
    check_tree(f.name, tree0, ext, cols, bn, bn, rng)
    tree0.free()

    def lde_commit():
        mat.low_degree_extend(small, big)
        check(lib().ark_hip_merkle_commit_sfp_device(f.sid, mat.vec._p, cols, bn, bn, tree._tree, None), "commit")

    row, tree = commit_case("4x extension of %d x 2^%d" % (cols, slog), f.name, mat, mat.vec.to_host(), cols, bn, bn, lde, rng, 3 if not quick else 10)
    t = rounds({"lde_then_commit": lde_commit}, 3)
    row["lde_then_commit_ms"], row["lde_then_commit_spread_ms"] = t["lde_then_commit"]
    rows.append(row)
    tree.free()
    mat.vec.free()
    return rows, opens


def fr_cases(quick, rng):
    p = M.modulus(FR)
    rows = []
    for count, log in ([(1, 12), (4, 10)] if quick else [(1, 24), (8, 20)]):
        n = 1 << log
        host = rng.integers(0, 1 << 62, size=(count * n, 4), dtype=np.uint64)
        host[:, 3] %= np.uint64(p >> 192)   # every element below p
        vec = A.DeviceVec.from_host(FR, host)
        dom = A.Radix2EvaluationDomain.new(FR, n)
        L = lib()

        def transform():
            for c in range(count):
                check(L.ark_hip_fft_in_place_device(dom.field, C.byref(dom._s), C.c_void_p(vec.ptr.value + c * n * 32)), "fft")

        row, tree = commit_case("%d x 2^%d" % (count, log), FR, vec, host, count, n, n, transform, rng, 3 if not quick else 10)
        rows.append(row)
        tree.free()
        vec.free()
    return rows


def seam_sweep(quick, rng):
    """one node-bound tree (BabyBear, one column): the commit under every pair of the two seams"""
    log = 14 if quick else 20
    n = 1 << log
    f = R.FIELDS["BABYBEAR"]
    vec = A.SmallDeviceVec.from_host("BABYBEAR", rng.integers(0, f.p, size=n, dtype=np.uint64).astype(np.uint32))
    tree = vec.commit()
    want = tree.root
    L = lib()

    def commit():
        check(L.ark_hip_merkle_commit_sfp_device(f.sid, vec._p, 1, n, n, tree._tree, None), "commit")

    variants = {}
    for tail in (0, 4, 6, 8):
        for levels in (1, 2, 4, 9):
            env = dict(ARK_HIP_MERKLE_TAIL_LOG=tail, ARK_HIP_MERKLE_LEVELS=levels)
            with_env(commit, **env)()
            check(L.ark_hip_synchronize(), "sync")
            got = np.empty(32, dtype=np.uint8)
            check(L.ark_hip_memcpy_d2h(got.ctypes.data_as(C.c_void_p), tree._tree, 32), "d2h")
            assert got.tobytes() == want, (tail, levels)
            variants["tail%d_levels%d" % (tail, levels)] = with_env(commit, **env)
    t = rounds(variants, 10 if not quick else 20)
    out = {"case": "BABYBEAR 1 x 2^%d" % log, "reps": 10, "rounds": ROUNDS,
           "commit_ms": {k: v[0] for k, v in t.items()}, "spread_ms": {k: v[1] for k, v in t.items()}}
    print(json.dumps(out), flush=True)
    tree.free()
    vec.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle.json"))
    ap.add_argument("--quick", action="store_true", help="small matrices: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    rng = np.random.default_rng(28)
    out = {"date": datetime.date.today().isoformat(), "version": lib().ark_hip_version().decode(),
           "timing": "wall clock per call over `reps` queued calls between two ark_hip_synchronize(), after warm-up; median and spread "
                     "(max - min) of `rounds` interleaved rounds; device-resident data; d2h into pinned host memory",
           "quick": bool(args.quick), "valu_per_round": {str(k): v for k, v in VALU_PER_ROUND.items()}, "plan_defaults": A.merkle_plan(1 << 20, 1, 4),
           "cases": [], "open": []}
    out["seams"] = seam_sweep(args.quick, rng)
    for name in ("BABYBEAR", "GOLDILOCKS"):
        rows, opens = small_cases(R.FIELDS[name], args.quick, rng)
        out["cases"] += rows
        out["open"] += opens
    out["cases"] += fr_cases(args.quick, rng)
    judged = [c for c in out["cases"] if c["counts_for_the_condition"]]
    out["condition"] = "at every case of at least 2^24 elements in total, commit is faster than the device-to-host copy of the matrix by more than the two spreads"
    out["margins_ms"] = {"%s %s" % (c["field"], c["case"]): c["margin_ms"] for c in judged}
    out["accepted"] = bool(judged) and all(c["faster_than_d2h_beyond_spread"] for c in judged)
    out["perm1_kept"] = all(c["perm1_faster_beyond_spread"] for c in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out, "accepted:", out["accepted"], "perm1 faster everywhere:", out["perm1_kept"])


if __name__ == "__main__":
    main()
