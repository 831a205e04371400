"""algebra_amd -- MI355X-native MSM and radix-2 FFT behind the arkworks trait surface.

Host-side mirror (Python, for tests/bench/multi-GPU plumbing) of the two reference interfaces the
HIP library replaces:

    ark_ec::VariableBaseMSM            -> algebra_amd.msm   (msm, msm_unchecked, msm_bigint)
    ark_poly::Radix2EvaluationDomain   -> algebra_amd.domain.Radix2EvaluationDomain
    ark_poly::DenseMultilinearExtension -> algebra_amd.mle.DenseMultilinearExtension
    ark_linear_sumcheck's ListOfProductsOfPolynomials and its prover's rounds -> algebra_amd.sumcheck.ListOfProducts
    (no reference counterpart) SHA3-256 Merkle trees over column batches -> algebra_amd.merkle.MerkleTree
    ark_ff's Fp2 / Fp4 over SmallFp, and (no reference counterpart) the FRI commit phase -> algebra_amd.fri

All arithmetic runs in libark_hip.so (hand-written HIP for gfx950) through the C ABI of
include/ark_hip.h; this package holds no arithmetic and no CPU fallback.
"""
from . import curves  # noqa: F401
from ._lib import ArkHipError, LIB_PATH, lib  # noqa: F401
from .msm import (BatchMulPreprocessing, batch_mul, ChunkedPippenger, HashMapPippenger, MsmJob, MsmLengthMismatch, PreparedBases, into_affine,  # noqa: F401
                  msm, msm_bigint, msm_bigint_async, msm_bigint_multi, msm_chunks, msm_u1, msm_u8, msm_u16, msm_u32,
                  msm_u64, msm_unchecked, normalize_batch, sum_projective, base_cache_config, base_cache_clear,
                  base_cache_stats, base_cache_hash_stats, ResidentBases, pin_bases, msm_plan, msm_plan_widths, MSM_WIDTH_TOP,
                  BaseCheck, check_bases, BaseDecode, compressed_size, decompress_bases, compress_bases)
from .domain import Radix2EvaluationDomain  # noqa: F401
from .poly import DeviceVec, poly_mul, poly_mul_host, prefix_scan_plan  # noqa: F401
from .sparse import CsrMatrix, csr_plan  # noqa: F401
from .points import DevicePoints  # noqa: F401
from .mle import (DenseMultilinearExtension, DeviceSegment, lookup_plan, mle_eq_plan, mle_fold_plan, mle_fold_tiles, mle_fraction_tree_launches,  # noqa: F401
                  mle_fraction_tree_plan, mle_product_tree_launches, mle_product_tree_plan, mle_quotients_plan)
from .sumcheck import ListOfProducts, SumcheckProof, sumcheck_plan, sumcheck_prove_plan  # noqa: F401
from .gates import SumOfProducts, sum_of_products_plan  # noqa: F401
from .transcript import Transcript  # noqa: F401
from .grand_product import GrandProduct, GrandProductProof  # noqa: F401
from .fraction_sum import FractionalSum, FractionalSumProof  # noqa: F401
from .smallfp import (SMALL_FIELDS, SmallDeviceMatrix, SmallDeviceVec, SmallRadix2EvaluationDomain, small_fft_plan,  # noqa: F401
                      small_field_info, small_field_pow)
from .merkle import MerkleTree, merkle_leaf_fr, merkle_leaf_small, merkle_node, merkle_plan  # noqa: F401
from .fri import (FriProver, SmallExtVec, combine_columns, ext_inverse, ext_mul, ext_pow, fri_fold, fri_fold_row,  # noqa: F401
                  fri_folded_domain, fri_plan, fri_verify_query, small_ext_degree, small_ext_info)
