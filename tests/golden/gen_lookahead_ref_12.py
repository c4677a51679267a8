#!/usr/bin/env python3
"""tests/golden/lookahead_ref_12.npz: the 12-bit sibling of lookahead_ref.npz -- the 48 x 40
"noise" and 56 x 32 "smooth" frames at 12 bits, both as plain cases (estimate_intra_costs,
estimate_importance_block_difference, the cost loop of estimate_inter_costs,
update_block_importances) and as adversarial cases of update_block_importances, computed by
the REFERENCE'S OWN SOURCE TEXT exactly as gen_lookahead_ref.py does (same keys).  A file and
a seed of its own, so lookahead_ref.npz is never rewritten.

Run in the build container:  python tests/golden/gen_lookahead_ref_12.py
"""
import gen_lookahead_ref

CASES_12 = [(12, 48, 40, "noise"), (12, 56, 32, "smooth")]

if __name__ == "__main__":
    gen_lookahead_ref.main(cases=CASES_12, adv_cases=CASES_12, seed=20261912, name="lookahead_ref_12.npz")
