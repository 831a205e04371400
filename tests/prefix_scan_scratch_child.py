"""Child process of tests/test_gpu_prefix_scan.py::test_small_calls_on_poisoned_scratch, run with
ARK_HIP_LIB=algebra_amd/libark_hip_test.so so that the Python mirror and the hooks are one library instance (the protocol and
the helpers are those of tests/scratch_reuse_child.py).

The prefix scans keep the tile totals and carries of every level in Context::poly_work, which only grows and is never cleared.
Each entry runs warm, then with every scratch buffer filled with the poison word, then poisoned again after a larger call on
the same context: the results are those of the big-integer model every time, no buffer moved, and nothing was written past
what the call asked for."""
import numpy as np

import scratch_reuse_child as H          # asserts the library instance, brings poison() and assert_clean()
import algebra_amd as A
import oracle_lib as O
import prefix_scan_ref as R

FNAME = "BLS12_381_FR"
F = R.Field(FNAME)


def rand(n, seed):
    a = O.gen_scalars(O.FID[FNAME], seed, n, montgomery=True)
    a[~a.any(axis=1)] = R.limbs([F.one])[0]
    return a


def scan_case(op, n, seed, checked=True):
    a = rand(n, seed)
    da = A.DeviceVec.from_host(FNAME, a)
    model = R.prefix_product if op == "product" else R.prefix_sum
    if checked:
        want = [(R.limbs(w), R.limbs([t])[0]) for w, t in (model(F, R.ints(a), ex) for ex in (False, True))]

    def run():
        ok = True
        for ex in (False, True):
            out, total = (da.prefix_product if op == "product" else da.prefix_sum)(exclusive=ex)
            got = out.to_host()
            out.free()
            ok = ok and (not checked or (np.array_equal(got, want[ex][0]) and np.array_equal(total, want[ex][1])))
        return ok
    return run


def ratio_case(n, seed, checked=True, zero_at=None):
    num, den = rand(n, seed), rand(n, seed + 1)
    if zero_at is not None:
        den[zero_at] = 0
    dn, dd = A.DeviceVec.from_host(FNAME, num), A.DeviceVec.from_host(FNAME, den)
    if checked:
        w, t = R.prefix_ratio(F, R.ints(num), R.ints(den))
        want, want_last = R.limbs(w), R.limbs([t])[0]

    def run():
        out, last = dn.prefix_ratio(dd)
        got = out.to_host()
        out.free()
        return not checked or (np.array_equal(got, want) and np.array_equal(last, want_last))
    return run


def main():
    T = A.prefix_scan_plan("product", 0)[0]
    TR = A.prefix_scan_plan("ratio", 0)[0]
    small, big = 3 * T + 5, T * T + 1     # two levels: the carries in poly_work are read; three levels and a larger poly_work
    for op in ("product", "sum"):
        H.protocol("prefix %s at 3 T + 5 after T^2 + 1" % op, scan_case(op, small, 0x21), big=scan_case(op, big, 0x23, checked=False),
                   reach=("poly_work",))
    H.protocol("prefix ratio at 3 T + 5 after T^2 + 1", ratio_case(3 * TR + 5, 0x31), big=ratio_case(TR * TR + 1, 0x33, checked=False),
               reach=("poly_work",))
    H.protocol("prefix ratio with a zero denominator", ratio_case(3 * TR + 5, 0x41, zero_at=TR + 3),
               big=ratio_case(TR * TR + 1, 0x43, checked=False), reach=("poly_work",))
    H.protocol("prefix ratio of one tile", ratio_case(65, 0x51), reach=("poly_work",))
    print("prefix-scan scratch ok", flush=True)


if __name__ == "__main__":
    main()
