"""Helpers of the wide (hidden 256 / 512) GRU list-decoding tests (tests/test_rnnl_wide.py, tests/test_rnnl_wide_gpu.py).

The numpy restatement, the fixture loader and the candidate ordering are tests/rnnl_helper.py's; this file carries the
wide fixtures' case table (tests/golden/gen_rnnl_wide.py writes them) and their logit tolerances.

The seeded nets are PyTorch-default draws with the GRU parameters x 3 and the output Linear x 10, so their logits are
~10 x a default net's and the project's 2e-5 logit tolerance is not assumed for them.  Per fixture, E is the measured
max |greedy decode(..., return_logits=True) logit - the reference's greedy logit| over the fixture's words with equal
decisions, on the weight-streaming greedy kernel (gru_wide_kernel, which the list kernel shares its per-column
arithmetic with), and the fixture's tolerance is max(2e-5, 2 E): a difference of two metrics involves two paths.
"""
from rnnl_helper import (DIST_MARGIN, GOLDEN, LOGIT_ATOL, encode_np, list_decode_np, load_fixture,  # noqa: F401
                         seeded_state_dict, sorted_candidates, unpack_pm1, weights_digest)

# fixture -> (the trained fixture its weights come from, or None for a seeded net regenerated from w_seed; list sizes)
SEEDED = {
    "rnnl_polar_16_8_f256_l1": (None, (2, 5)),
    "rnnl_polar_32_16_f512_l2": (None, (4, 8)),
    "rnnl_pac_32_10_f256_l2": (None, (3,)),
}
TRAINED = "rnnl_crisp_64_22_f512"  # w_source = trained_crisp_64_22_f512; msg_L4 on 256 words and the L = 4 curve counts

# E per fixture: measured on one MI355X with the greedy wide kernel of the commit before the wide list kernel
# (npd_gru_decode, fp32; 256 words each, every word decoded as the reference decodes it)
E_MEASURED = {
    "rnnl_polar_16_8_f256_l1": 2.87e-6,   # max |logit| 9.8; all 256 words decoded alike
    "rnnl_polar_32_16_f512_l2": 7.43e-6,  # max |logit| 14.5; all 256 words decoded alike
    "rnnl_pac_32_10_f256_l2": 5.49e-6,    # max |logit| 10.7; all 256 words decoded alike
}
# 2 E <= 1.5e-5 everywhere, so every wide fixture is held to the project's 2e-5
LOGIT_TOL = {name: max(LOGIT_ATOL, 2.0 * e) for name, e in E_MEASURED.items()}

STABLE_MIN = 0.99  # float64-stable share per L
ROBUST_MIN = 0.50  # robust share per L at the fixture's tolerance


def robust_mask(d, L, tol):
    """rnnl_helper.robust_mask at a logit tolerance of `tol`: every prune boundary wider than two metrics' tolerance
    (each a sum of at most K logits held to tol) and the final selection wider than DIST_MARGIN."""
    K = int(d["K"])
    return (d[f"prune_margin_L{L}"] >= 2 * K * tol) & (d[f"dist_margin_L{L}"] >= DIST_MARGIN)
