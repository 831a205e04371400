"""Child process of tests/test_gpu_lookup.py::test_lookup_on_poisoned_scratch, run with
ARK_HIP_LIB=algebra_amd/libark_hip_test.so so that the Python mirror and the hooks are one library instance (the protocol and
the helpers are those of tests/scratch_reuse_child.py).

ark_hip_fr_lookup_device hashes its table into slots in Context::poly_work, which only grows and is never cleared: a slot that
an earlier call left behind is a table index, possibly past this call's table.  The call runs warm, then with every scratch
buffer filled with the poison word, then poisoned again after a call on a larger table, and then straight after that larger
call with its slots still in place: the results are those of the dictionary model every time, no buffer moved, and nothing was
written past what the call asked for."""
import numpy as np

import scratch_reuse_child as H          # asserts the library instance, brings poison() and assert_clean()
import algebra_amd as A
import lookup_ref as R
import mle_ref
import oracle_lib as O
import pyref
import sumcheck_ref as S

FNAME = "BLS12_381_FR"
P = pyref.MODULI[FNAME][0]
MLE = A.DenseMultilinearExtension


def case(table_len, n, seed, checked=True):
    fid = O.FID[FNAME]
    ta = O.gen_scalars(fid, seed, table_len, montgomery=True)
    absent = O.gen_scalars(fid, seed + 1, 16, montgomery=True)
    rng = np.random.default_rng(seed)
    va = ta[rng.integers(0, table_len, size=n)]
    out = np.nonzero(rng.random(n) < 0.1)[0]
    va[out] = absent[rng.integers(0, 16, size=out.size)]
    dt, dv = A.DeviceVec.from_host(FNAME, ta), A.DeviceVec.from_host(FNAME, va)
    if checked:
        idx, m, missing = R.lookup(mle_ref.ints(ta), mle_ref.ints(va))
        want_idx, want_m = np.array(idx, dtype=np.uint32), S.encode(m, P)
        assert 0 < missing < n

    def run():
        mv, got_missing, got_idx = MLE.lookup(dt, dv, indices=True)
        got_m = getattr(mv, "evaluations", mv).to_host()   # an extension when the table's length is a power of two
        mv.free()
        return not checked or (got_missing == missing and np.array_equal(got_idx, want_idx) and np.array_equal(got_m, want_m))
    return run


def main():
    small, big = case(1000, 4097, 0x26), case(1 << 14, 1 << 14, 0x28, checked=False)
    assert A.lookup_plan(1000)[1] < A.lookup_plan(1 << 14)[1]
    H.protocol("lookup of 4097 cells in 1000 after 2^14 in 2^14", small, big=big, reach=("poly_work",))
    # the larger table's slots themselves, not the poison, lie where the small call hashes
    assert big() and small(), "stale slots of a larger table reached the result"
    H.assert_clean("lookup straight after a larger table", reach=("poly_work",))
    tiny = case(3, 65, 0x2A)
    assert big() and tiny(), "stale slots of a larger table reached the result of a table of 3"
    print("lookup scratch ok", flush=True)


if __name__ == "__main__":
    main()
