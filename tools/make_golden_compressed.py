#!/usr/bin/env python3
"""The reference's known answers for compressed BLS12-381 points as fixtures under tests/golden/ (a sibling of
tools/make_golden.py, whose outputs it does not touch).

Sources (data files, not code; checked by the reference at curves/bls12_381/src/curves/tests/mod.rs):
  curves/bls12_381/src/curves/tests/g1_compressed_valid_test_vectors.dat   compressed k*G1, k = 0..999, 48 bytes each
  curves/bls12_381/src/curves/tests/g2_compressed_valid_test_vectors.dat   compressed k*G2, k = 0..999, 96 bytes each
They are the compressed forms of the tables tests/golden/bls12_381_g{1,2}_multiples.npz hold uncompressed.

Output:  tests/golden/bls12_381_g1_compressed.npz   bytes uint8 [1000, 48]
         tests/golden/bls12_381_g2_compressed.npz   bytes uint8 [1000, 96]
"""
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def main(ref):
    t = os.path.join(ref, "bls12_381/src/curves/tests")
    for g, e in (("g1", 48), ("g2", 96)):
        raw = np.fromfile(os.path.join(t, "%s_compressed_valid_test_vectors.dat" % g), dtype=np.uint8)
        assert raw.size == 1000 * e, raw.size
        rows = raw.reshape(1000, e)
        assert (rows[:, 0] & 0x80).all() and rows[0, 0] == 0xC0 and not rows[0, 1:].any()      # compressed; entry 0 = infinity
        np.savez_compressed(os.path.join(OUT, "bls12_381_%s_compressed.npz" % g), bytes=rows)
        print("%s: %d entries, larger bit set on %d" % (g, len(rows), int(((rows[:, 0] >> 5) & 1).sum())))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_compressed.py <reference checkout>/curves")
    main(sys.argv[1])
