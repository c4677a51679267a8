#!/usr/bin/env python3
"""tiling_ref.npz: the reference's tile grid for the frame sizes and tile counts of BASELINE.json and a
sweep around them.  TilingInfo::from_target_tiles is EXECUTED (src/tiling/tiler.rs:56-150) inside the
tile-count loop of Sequence::new (src/encoder.rs:248-277, eight lines, restated here).

`cases` rows: (width, height, target tiles, rows, cols, tile_width_sb, tile_height_sb) of the grid the
reference lands on.  tests/test_reference_unit_tests.py::test_tile_rects_equal_the_executed_tiling_info
holds rav1e_amd/workload.py::tile_rects to it."""
import numpy as np

import reflib

SIZES = ((3840, 2160), (1920, 1080), (1280, 720), (4096, 2304), (640, 360), (3840, 2176), (1000, 600))
TILES = (1, 2, 4, 8, 16)


def main():
    c = reflib.crate("tiling/tiler.rs")
    ftt = c.get("from_target_tiles", owner="TilingInfo")

    def reference_tiling(w, h, tiles):
        rl = cl = 0
        while True:
            t = ftt({}, 6, w, h, 60.0, cl, rl, False)
            if t.rows * t.cols >= tiles:
                return t
            if not (rl < t.max_tile_rows_log2 or cl < t.max_tile_cols_log2):
                return t
            if (t.tile_height_sb >= t.tile_width_sb and t.tile_rows_log2 < t.max_tile_rows_log2) or \
                    cl >= t.max_tile_cols_log2:
                rl += 1
            else:
                cl += 1
    rows = []
    for (w, h) in SIZES:
        for tiles in TILES:
            t = reference_tiling(w, h, tiles)
            rows.append((w, h, tiles, t.rows, t.cols, t.tile_width_sb, t.tile_height_sb))
    reflib.save("tiling_ref.npz", {"cases": np.array(rows, np.int32)})


if __name__ == "__main__":
    main()
