"""The GEMM checker's own tests (no GPU). They live beside the reference and
the cases in tests/gemm_ref.py; this module only brings them under the name
pattern the collection goes by."""
from gemm_ref import (  # noqa: F401
    test_a_read_transposed_fails,
    test_dropped_k_term_fails_in_every_element,
    test_dropped_last_k_step_fails,
    test_err2_and_trp_references_on_the_float64_model,
    test_float64_product_passes_every_case,
    test_mirror_from_the_wrong_side_fails,
    test_omitted_beta_c_fails,
    test_reference_precision,
    test_scaled_reference_takes_the_kernels_branches,
    test_transform_diagonal_at_output_indices_fails,
)
