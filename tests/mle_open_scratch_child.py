"""Child process of tests/test_gpu_mle_open.py::test_small_calls_on_poisoned_scratch, run with
ARK_HIP_LIB=algebra_amd/libark_hip_test.so so that the Python mirror and the hooks are one library instance (the protocol and
the helpers are those of tests/scratch_reuse_child.py).

The eq table and the quotients keep their intermediate tables in Context::poly_work, which only grows and is never cleared.
A small call of each runs after a larger one on the same context, then again with every scratch buffer filled with the
poison word: the results are those of the big-integer model both times, no buffer moved, and nothing was written past what
the call asked for."""
import numpy as np

import scratch_reuse_child as H          # asserts the library instance, brings poison() and assert_clean()
import algebra_amd as A
import mle_open_ref as R
import mle_ref
import oracle_lib as O
import pyref

FNAME = "BLS12_381_FR"
P = pyref.MODULI[FNAME][0]
RM = pyref.R_of(P)
MLE = A.DenseMultilinearExtension


def canon_and_mont(seed, count):
    mont = O.gen_scalars(O.FID[FNAME], seed, max(count, 1), montgomery=True)[:count]
    vals = mle_ref.ints(mont)                                   # canonical residues: random values < p
    return vals, mle_ref.limbs([v * RM % P for v in vals]).reshape(-1, 4)


def eq_case(nv, seed):
    ptc, pt = canon_and_mont(seed, nv)
    (scv,), sc = canon_and_mont(seed + 1, 1)
    want = mle_ref.limbs(R.eq_table_mont(ptc, scv, P, RM))

    def run():
        m = MLE.eq(FNAME, pt, sc[0])
        ok = np.array_equal(m.to_evaluations(), want)
        m.free()
        return ok
    return run


def quotient_case(nv, seed):
    table = O.gen_scalars(O.FID[FNAME], seed, 1 << nv, montgomery=True)
    ptc, pt = canon_and_mont(seed + 1, nv)
    value, qs = R.quotients(mle_ref.ints(table), ptc, P)
    want = [mle_ref.limbs(q) for q in qs]
    m = MLE.from_evaluations(FNAME, nv, table)

    def run():
        got, segs = m.quotients(pt)
        return np.array_equal(got, pyref.to_limbs(value, 4)) and all(np.array_equal(s.to_host(), w) for s, w in zip(segs, want))
    return run


def main():
    # small: two launches, so the intermediate table in poly_work is read; big: three launches and a larger poly_work
    H.protocol("mle eq table 2^11 after 2^19", eq_case(11, 7), big=eq_case(19, 9), reach=("poly_work",))
    H.protocol("mle quotients 2^11 after 2^19", quotient_case(11, 17), big=quotient_case(19, 19), reach=("poly_work",))
    print("mle-open scratch ok", flush=True)


if __name__ == "__main__":
    main()
