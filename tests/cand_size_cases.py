"""The (transform size, bit depth) case tables of the GPU tests of the two kernel families that are compiled once per
size and depth -- k_rdo_cand<.., PS = 1> behind r1_rdo_intra_cand_batch and k_compound_fast behind
r1_rdo_compound_cand_batch -- as plain data (no numpy, no torch): tests/test_gpu_rdo_intra.py, tests/test_gpu_depth12.py
and tests/test_gpu_compound.py parametrise over them, and tests/test_cand_size_cases.py (no GPU) holds them against the
instantiations the plan names, so a size that loses its row is noticed without a device."""

# TxSize id -> (width, height)
TX_DIMS = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8),
           (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4), (8, 32), (32, 8),
           (16, 64), (64, 16)]
DEPTHS = (8, 10, 12)

# ---- r1_rdo_intra_cand_batch ----
# The distortion kinds every row below is launched with: dist_kind 0 is QM 1 of the plan, a pixel-domain kind QM 2.
INTRA_KINDS = (3, 0, 2)

# test_gpu_rdo_intra.py::test_intra_cand_equals_two_launch_route_and_oracle, rows (TxSize id, bit depth).
# 4x4: 16 candidates per wave; 8x8 / 16x16: the fan-out with the full intra mask; 4x16 / 16x4: lanes per candidate
# != width; 32x32: the plain kernel (int16 transpose tile at 10-bit); 64x64: split transpose (masked at 8-bit); 16x64
INTRA_CASES_SEEDED = [(0, 8), (0, 10), (1, 8), (1, 10), (1, 12), (2, 8), (2, 10), (2, 12), (13, 8), (13, 10), (14, 8),
                      (14, 10), (3, 8), (3, 10), (4, 8), (4, 10), (17, 8), (17, 10)]
# The rest of the 19 x 3 pairs that test_gpu_depth12.py does not launch.  The 2:1 rectangles (INV_SQRT2 in both
# transform passes, the DC predictor's 2:1 multiplier), w + h = 12, 40, 48 and 96 (edge-filter strength and upsample
# brackets of their own), the blocks taller than wide (P = H lanes per candidate load the edges and stage the source,
# W columns stay live), every 64x32 / 32x64 plan.  These rows carry a flat block at the origin and assert that zero and
# non-zero eob both occur.
INTRA_CASES_EOB = [(ts, bd) for ts in (5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 18) for bd in (8, 10)] + \
                  [(ts, 12) for ts in (5, 6, 9, 10, 11, 12, 15, 16, 18)]
INTRA_CASES = INTRA_CASES_SEEDED + INTRA_CASES_EOB

# test_gpu_depth12.py::test_intra_cand_12_bit_instantiations, TxSize ids at 12 bits: 4x4, 32x32, 64x64, 4x16, 16x4,
# 16x64 and the pair 8x16 / 16x8
DEPTH12_INTRA_SIZES = [0, 3, 4, 13, 14, 17, 7, 8]


def intra_rows():
    """every (TxSize id, bit depth, dist_kind) the two tests above launch r1_rdo_intra_cand_batch with"""
    pairs = INTRA_CASES + [(ts, 12) for ts in DEPTH12_INTRA_SIZES]
    return [(ts, bd, kind) for (ts, bd) in pairs for kind in INTRA_KINDS]


# ---- r1_rdo_compound_cand_batch ----
# test_gpu_compound.py::test_compound_parity_random / _saturated, (width, height) at every depth of COMPOUND_DEPTHS: the
# 19 transform sizes (k_compound_fast, one instantiation per size and depth) and 128x64 / 128x128 (the slab kernel, two
# and four slabs)
COMPOUND_SIZES = TX_DIMS + [(128, 64), (128, 128)]
COMPOUND_DEPTHS = DEPTHS
