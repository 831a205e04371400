"""Completeness of the asynchrony-contract suite, on the host (no GPU): every `*_device` entry include/ark_hip.h declares is in
the case table of tests/async_cases.py or in its exclusion list with a reason, every case can tell a stale output from the
right one, and every host argument of parts B and C has a replacement of the same shape that differs from it.  A new entry
that is in neither list fails here."""
import os

import numpy as np

import async_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_device_entry_has_a_case_or_a_reason():
    header = open(os.path.join(ROOT, "include", "ark_hip.h")).read()
    declared = AC.declared_entries(header)
    assert len(declared) >= 70 and "ark_hip_fr_add_device" in declared and "ark_hip_memset_device" in declared
    covered = {c.entry for c in AC.CASES}
    assert covered <= declared, covered - declared
    assert set(AC.EXCLUDED) <= declared, set(AC.EXCLUDED) - declared
    assert not covered & set(AC.EXCLUDED), covered & set(AC.EXCLUDED)
    missing = declared - covered - set(AC.EXCLUDED)
    assert not missing, "no case and no exclusion for: %s" % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 10 and "\n" not in r for r in AC.EXCLUDED.values())
    from algebra_amd import _lib
    assert all(c.entry in _lib.SYMBOLS for c in AC.CASES)


def test_the_parts_cover_what_the_contract_names():
    """the producers of part A, the host inputs of part B, the pairs of part C and the waiting forms of part D, entry by entry"""
    def entries(part):
        return {c.entry[len("ark_hip_"):-len("_device")] if c.entry.endswith("_device") else c.entry[len("ark_hip_"):]
                for c in AC.cases_of(part)}
    a = {"fr_add", "fr_sub", "fr_mul", "fr_neg", "fr_scale", "fr_div", "fr_inverse", "fr_axpy", "fr_lincomb", "memcpy_d2d", "memset",
         "fr_count_indices", "fr_lookup", "fr_sum_of_products", "fr_csr_mul", "fft_in_place", "ifft_in_place",
         "fft_in_place_degree_aware", "fft_batch_in_place", "fft_axis", "fft_shard_local", "fft_shard_cross", "fft_sharded",
         "poly_divide_linear", "poly_divide_by_vanishing", "domain_lagrange_coefficients", "fr_prefix_product", "fr_prefix_sum",
         "fr_prefix_ratio", "mle_fix_variables", "mle_relabel", "mle_eq_table", "mle_quotients", "mle_product_tree", "mle_fraction_tree"}
    assert entries("A") == a, entries("A") ^ a
    b = {"fr_scale", "fr_axpy", "fr_lincomb", "fr_sum_of_products", "poly_divide_linear", "domain_lagrange_coefficients",
         "mle_fix_variables", "mle_eq_table", "mle_quotients", "fft_in_place", "ifft_in_place", "fft_in_place_degree_aware",
         "fft_batch_in_place", "fft_axis", "fft_shard_local", "fft_shard_cross", "fft_sharded", "sw_fold"}
    assert entries("B") == b, entries("B") ^ b
    c = {"fft_axis", "fft_shard_cross", "fft_in_place", "ifft_in_place", "fr_scale", "mle_eq_table", "fr_lincomb", "sw_fold"}
    assert entries("C") == c, entries("C") ^ c
    d = {"poly_evaluate", "poly_divide_linear", "fr_inner_product", "fr_prefix_product", "fr_prefix_sum", "fr_prefix_ratio",
         "mle_evaluate", "mle_quotients", "mle_product_tree", "mle_fraction_tree", "fr_lookup", "sumcheck_round", "merkle_commit_fr"}
    assert entries("D") == d, entries("D") ^ d
    axis = {c.name for c in AC.cases_of("C") if c.entry == "ark_hip_fft_axis_device"}
    assert axis == {"fft_axis G=%d cols=%d" % (g, n) for g in (2, 4, 8, 16) for n in (300, 4097)}
    fields = {c.fname for c in AC.cases_of("A") if c.entry in ("ark_hip_fr_add_device", "ark_hip_fr_axpy_device",
                                                                 "ark_hip_fr_lincomb_device", "ark_hip_fr_sum_of_products_device")}
    assert fields == set(AC.FIELDS)
    b_fields = {c.fname for c in AC.cases_of("B") if c.entry in ("ark_hip_fr_scale_device", "ark_hip_fr_axpy_device",
                                                                   "ark_hip_fr_lincomb_device", "ark_hip_fr_sum_of_products_device")}
    assert b_fields == set(AC.FIELDS)                # their host arguments die on every field's kernels
    assert all(c.fname == AC.FR for part in "CD" for c in AC.cases_of(part))
    assert {g.split(":")[1] for g in AC.GROUPS if g.startswith("A:")} == {c.group for c in AC.cases_of("A")}


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def test_every_case_tells_the_stale_output_from_the_right_one():
    for c in AC.CASES:
        b = c.make(0)
        assert set(b.outs) <= set(b.dev) and (b.outs or b.wait), c.name
        for o in b.outs:
            want = b.expected(o)
            if b.compare:
                assert not np.array_equal(b.compare(want.view(np.uint64)), b.compare(_bytes(b.dev[o]).view(np.uint64))), (c.name, o)
            else:
                assert not np.array_equal(want, _bytes(b.dev[o])), (c.name, o)
        if "A" in c.parts:
            out, off, count = b.consume
            seg = slice(32 * off, 32 * (off + count))
            assert out in b.outs and 0 < count <= AC.N and 32 * (off + count) <= _bytes(b.dev[out]).size, c.name
            assert not np.array_equal(b.expected(out)[seg], _bytes(b.dev[out])[seg]), (c.name, "the consumed segment")
        if "D" in c.parts:
            assert b.wait and len(b.wait[1]()) == b.wait[0] and b.wait[1]() != bytes([0xA5]) * b.wait[0], c.name


def test_every_host_input_of_parts_b_and_c_has_a_replacement_of_the_same_shape():
    for part in "BC":
        for c in AC.cases_of(part):
            b, alt = c.make(0), c.make(part)
            assert b.host or b.ptrs, c.name
            assert set(alt.host) == set(b.host) and set(alt.ptrs) == set(b.ptrs), c.name
            changed = 0
            for k in b.host:
                assert alt.host[k].shape == b.host[k].shape and alt.host[k].dtype == b.host[k].dtype, (c.name, k)
                changed += not np.array_equal(alt.host[k], b.host[k])
            for k in b.ptrs:
                assert len(alt.ptrs[k]) == len(b.ptrs[k]) and set(alt.ptrs[k]) <= set(alt.dev), (c.name, k)
                for x, y in zip(b.ptrs[k], alt.ptrs[k]):
                    assert alt.dev[y].shape == b.dev[x].shape, (c.name, k)
                changed += alt.ptrs[k] != b.ptrs[k]
            differs = b.compare is not None or any(not np.array_equal(alt.expected(o), b.expected(o)) for o in b.outs)
            if part == "B":      # everything that is host memory dies, and a library that read it late computes something else
                assert all(not np.array_equal(alt.host[k], b.host[k]) for k in b.host), c.name
                assert changed and alt.outs == b.outs and differs, c.name
            else:                # the second call has other constants, or the other direction: another result
                # (the root of the 2-point transform is -1, its own inverse: that pair of part C repeats one constant)
                assert differs or c.name.startswith("fft_axis G=2 "), c.name
