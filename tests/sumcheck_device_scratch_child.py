"""Child process of tests/test_gpu_sumcheck_device.py::test_prove_device_on_poisoned_scratch, run with
ARK_HIP_LIB=algebra_amd/libark_hip_test.so so that the Python mirror and the hooks are one library instance (the protocol and
the helpers are those of tests/scratch_reuse_child.py).

ark_hip_sumcheck_prove_device keeps the round sums, the workgroups' partials, the challenge cell, the transcript's state and
the proof in Context::poly_work, which only grows and is never cleared.  The proof at 12 variables with the tail from 8 --
round kernels with two reduction stages, challenge launches, then the tail -- runs warm, then with every scratch buffer
filled with the poison word, then poisoned again after a larger call on the same context: the proof is the host-driven one
every time, no buffer moved, and nothing was written past what the call asked for."""
import numpy as np

import scratch_reuse_child as H          # asserts the library instance, brings poison() and assert_clean()
import algebra_amd as A
import oracle_lib as O

FNAME = "BLS12_381_FR"
SEED = bytes(range(32))


def case(nv, tail, checked=True):
    tabs = [A.DenseMultilinearExtension.from_evaluations(FNAME, nv, O.gen_scalars(O.FID[FNAME], 0x61 + k, 1 << nv, montgomery=True))
            for k in range(3)]
    one = A.DenseMultilinearExtension.eq(FNAME, np.zeros((0, 4), dtype=np.uint64)).to_evaluations()[0].copy()

    def make():
        lp = A.ListOfProducts(FNAME, nv)
        lp.add_product(tabs, one)
        lp.add_product([tabs[2], tabs[0]], tabs[1].to_evaluations()[1])
        return lp
    if checked:
        host, th = make(), A.Transcript(FNAME, SEED)
        want = host.prove(lambda i, evals: th.challenge(evals))
        host.free()

    def run():
        tr = A.Transcript(FNAME, SEED)
        got = make().prove_device(tr, tail)
        return not checked or (all(np.array_equal(a, b) for a, b in zip(got.rounds, want.rounds)) and np.array_equal(got.point, want.point) and
                               np.array_equal(got.final_evaluations, want.final_evaluations) and
                               np.array_equal(got.final_value, want.final_value) and tr.state == th.state)
    return run


def main():
    H.protocol("prove_device at 12 variables, tail from 8, after 16 variables", case(12, 8), big=case(16, 8, checked=False), reach=("poly_work",))
    H.protocol("prove_device at 12 variables without a tail", case(12, 0), reach=("poly_work",))
    print("sumcheck-device scratch ok", flush=True)


if __name__ == "__main__":
    main()
