#!/usr/bin/env python3
"""tests/golden/scales_ref.npz: the temporal-RDO scale maps, the k-means of their logarithms, the segment deltas
and thresholds, and the per-block scales and segment indices, computed by the REFERENCE'S OWN SOURCE TEXT through
tools/rustlite:

  src/rdo.rs            distortion_scale_for, DistortionScale::{new, inv_mean, mul, blog16, blog64}, From<f64>,
                        spatiotemporal_scale
  src/encoder.rs        CodedFrameData::compute_spatiotemporal_scores / compute_temporal_scores,
                        SegmentationState::update_threshold
  src/util/logexp.rs    blog32_q11, bexp64, blog64          src/util/kmeans.rs   kmeans, scan
  src/segmentation.rs   segmentation_optimize_inner, segment_idx_from_distortion
  src/quantize/mod.rs   ac_q, select_ac_qi

Executed as written, but for (docs/PARITY.md has the same list):
  * distortion_scale_for ends in `.into()`, whose target rustc infers from the return type; the transpiler hands
    the f64 back and this script applies the executed `From<f64> for DistortionScale` to it;
  * `i64: TryInto<T>` of kmeans: the transpiler is told T = i16 while kmeans runs (rustlite.runtime.TRY_INTO_TARGET);
  * segmentation_optimize_inner's six `kmeans(l)` take their K from the annotated tuple type; REWRITE RULE: the
    i-th `kmeans(l)` of that statement becomes `kmeans::<i16, {8 - i}>(l)`, nothing else of the function changes;
  * FrameInvariants / FrameState are stand-ins holding the fields the executed text reads (coded_frame_data,
    base_q_idx, config.bit_depth, config.temporal_rdo(); segmentation);
  * select_segment's `.max(min_segment)` after segment_idx_from_distortion is restated (it needs a TileStateMut).

The one float: pow.  Inputs are kept only where DistortionScale does not move when the host's pow result moves by
+-16 ulp (scales_model.pow_guard, from the inputs alone); a dropped block is redrawn and counted in `pow_dropped`.

Run in the build container:  python tests/golden/gen_scales_ref.py        (a few seconds)
R1_SCALES_CASES=a,b limits the map cases (mutation checks, tests/test_scales_ref.py)."""
import os
import sys
from types import SimpleNamespace

import numpy as np

import reflib as L
from reflib import R

sys.path.insert(0, os.path.join(L.ROOT, "tests"))
import scales_model as M  # noqa: E402

FILES = ("rdo.rs", "util/logexp.rs", "util/kmeans.rs", "quantize/mod.rs", "quantize/tables.rs", "partition.rs",
         "context/block_unit.rs", "context/transform_unit.rs", "context/superblock_unit.rs", "encoder.rs",
         "segmentation.rs")
QUANTIZERS = [(q, bd) for q in (1, 20, 128, 255) for bd in (8, 10, 12)]


def load():
    c = L.crate(*FILES)
    src = open(os.path.join(L.REF_SRC, "segmentation.rs")).read()
    a = src.index("fn segmentation_optimize_inner")
    body = src[a:src.index("#[profiling::function]", a)]
    assert body.count("kmeans(l)") == 6
    for k in range(8, 2, -1):
        body = body.replace("kmeans(l)", "kmeans::<i16, %d>(l)" % k, 1)
    c.load_text("<segmentation.rs:77-160, K of the six kmeans calls written out>",
                "pub mod k_written_out { use super::*; pub " +
                body.replace("fn segmentation_optimize_inner", "fn segmentation_optimize_inner_k") + "}")
    return c


class Ref:
    def __init__(self):
        c = self.c = load()
        self.DS = L.struct(c, "DistortionScale")
        self.dsf = c.get("distortion_scale_for")
        self.frm = c.get("from", owner="DistortionScale")
        self.st_scores = c.get("compute_spatiotemporal_scores", owner="CodedFrameData")
        self.t_scores = c.get("compute_temporal_scores", owner="CodedFrameData")
        self.blog16 = c.get("blog16", owner="DistortionScale")
        self.kmeans = c.get("kmeans")
        self.inner = c.get("segmentation_optimize_inner_k")
        self.st_scale = c.get("spatiotemporal_scale")
        self.sidx = c.get("segment_idx_from_distortion")
        self.ac_q = c.get("ac_q")
        self.SegState = L.struct(c, "SegmentationState")
        self.BO, self.PBO = L.struct(c, "BlockOffset"), L.struct(c, "PlaneBlockOffset")
        self.bsizes = [L.enum(c, "BlockSize", "BLOCK_%dX%d" % wh) for wh in M.BLOCK_DIMS]

    def scale_for(self, importance, intra):
        r = self.dsf({}, float(np.float32(importance)), float(intra))     # `propagate_cost as f64` of an f32
        return r._0 if hasattr(r, "_0") else self.frm({}, r)._0

    def frame(self, intra, importance, activity):
        DS = self.DS
        d = [DS(self.scale_for(p, i)) for p, i in zip(importance, intra)]
        cfd = SimpleNamespace(distortion_scales=R.RSlice(d), spatiotemporal_scores=R.RSlice([]),
                              # CodedFrameData::new fills activity_scales with 1.0; Tune::Psnr leaves them so
                              activity_scales=R.RSlice([DS(int(a)) for a in activity] if activity is not None else
                                                       [DS(1 << 14) for _ in d]))
        ret = (self.st_scores if activity is not None else self.t_scores)({}, cfd)
        return (np.array([s._0 for s in cfd.distortion_scales.tolist()], np.uint32),
                np.array([s._0 for s in cfd.spatiotemporal_scores.tolist()], np.uint32), ret, cfd)

    def centroids(self, scores):
        keys = sorted(self.blog16({}, self.DS(int(s))) for s in scores)
        out = np.zeros((6, 8), np.int16)
        R.TRY_INTO_TARGET = "i16"
        try:
            for r, k in enumerate(range(8, 2, -1)):
                out[r, :k] = self.kmeans({"K": k, "T": "i16"}, R.RSlice(list(keys))).tolist()
        finally:
            R.TRY_INTO_TARGET = None
        return out

    def segmentation(self, scores, base_q_idx, bit_depth):
        """segmentation_optimize_inner (with its own six k-means) + update_threshold"""
        DS = self.DS
        cfd = SimpleNamespace(spatiotemporal_scores=R.RSlice([DS(int(s)) for s in scores]))
        fi = SimpleNamespace(coded_frame_data=R.Some(cfd), base_q_idx=base_q_idx,
                             config=SimpleNamespace(bit_depth=bit_depth))
        seg = self.SegState(False, False, False, False, 0, R.RSlice([R.repeat(False, 8) for _ in range(8)]),
                            R.RSlice([R.repeat(0, 8) for _ in range(8)]), R.RSlice([DS(0) for _ in range(7)]), 0, 0)
        fs = SimpleNamespace(segmentation=seg)
        R.TRY_INTO_TARGET = "i16"
        try:
            self.inner({"T": "u8"}, fi, fs, 1 - base_q_idx)
        finally:
            R.TRY_INTO_TARGET = None
        data = [r[0] for r in seg.data.tolist()]                         # SEG_LVL_ALT_Q = 0
        feats = [r[0] for r in seg.features.tolist()]
        assert feats == [i <= seg.max_segment for i in range(8)], feats
        return (np.array(data, np.int16), np.array([t._0 for t in seg.threshold.tolist()], np.uint32),
                seg.min_segment, seg.max_segment)

    def block(self, cfd, w, h, bo_x, bo_y, bsize, thresholds, min_segment):
        cfd.w_in_imp_b, cfd.h_in_imp_b = w, h
        fi = SimpleNamespace(coded_frame_data=R.Some(cfd), config=SimpleNamespace(temporal_rdo=lambda: True))
        s = self.st_scale({"T": "u8"}, fi, self.PBO(self.BO(bo_x, bo_y)), self.bsizes[bsize])
        sidx = self.sidx({}, R.RSlice([self.DS(int(t)) for t in thresholds]), s)
        return s._0, max(sidx, min_segment)


def draw(rng, n, kind):
    """(intra u32, importance f32) of a map case"""
    intra = rng.integers(200, 60000, n).astype(np.uint32)
    imp = (intra * rng.random(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
    if kind == "zero_intra":
        intra[:] = 0
    elif kind == "zero_imp":
        imp[:] = 0
    elif kind == "clamp_hi":                     # ratios above 2^42: From<f64> saturates at 2^28 - 1
        intra = rng.integers(1, 5, n).astype(np.uint32)
        imp = (2.0 ** rng.uniform(42, 60, n)).astype(np.float32)
        imp[::5] = 3.0                           # ... next to ordinary blocks
    elif kind == "two_clusters":
        imp = np.where(rng.random(n) < 0.5, 0.0, intra * 1000.0 * rng.uniform(0.95, 1.05, n)).astype(np.float32)
    return intra, imp


MAP_CASES = [  # name, w, h, content, activity (None / "rand" / "tiny")
    ("one", 1, 1, "rand", "rand"), ("two", 2, 1, "rand", "rand"), ("two_t", 2, 1, "rand", None),
    ("odd", 13, 7, "rand", "rand"), ("odd_t", 13, 7, "rand", None), ("zero_intra", 13, 7, "zero_intra", "rand"),
    ("zero_imp", 13, 7, "zero_imp", None), ("clamp_hi", 13, 7, "clamp_hi", None),
    ("clamp_lo", 13, 7, "rand", "tiny"), ("two_clusters", 60, 34, "two_clusters", None),
    ("big", 60, 34, "rand", "rand"), ("big_t", 60, 34, "rand", None),
]
SEG_CASES = ("two", "odd", "zero_imp", "two_clusters", "big")      # x QUANTIZERS
BLOCK_CASES = ("odd", "big_t")


def blocks_for(w, h):
    """all 22 sizes at the origin, inside the map (odd 4x4 offsets too), cut by the right edge, the bottom edge,
    and both"""
    out = []
    for bs in range(22):
        for (x, y) in ((0, 0), (5, 3), (2 * (w - 1), 2), (4, 2 * (h - 1) + 1), (2 * (w - 1) + 1, 2 * (h - 1))):
            out.append((x, y, bs))
    return np.array(out, M.BLOCK)


def tie_keys(rng):
    """scores whose keys are a handful of neighbouring integers, so that thresholds (c1 + c2 + 1) >> 1 land ON
    keys; drawn until the model says that dropping the `+ 1` would move a centroid (the executed text then has to
    show the same: tests/test_scales_ref.py)"""
    cand = np.arange(15000, 18000, dtype=np.uint32)
    keys = M.blog16(cand)
    pick = [int(cand[np.nonzero(keys == k)[0][0]]) for k in range(-12, 13)]
    while True:
        s = np.array(rng.choice(pick, 91, p=rng.dirichlet(np.ones(len(pick)) * 0.3)), np.uint32)
        data = np.sort(M.blog16(s))
        if any(M.kmeans_sorted(data, k) != M.kmeans_sorted(data, k, bias=0) for k in range(3, 9)):
            return s


def main():
    ref = Ref()
    only = os.environ.get("R1_SCALES_CASES")
    only = set(only.split(",")) if only else None
    rng = np.random.default_rng(20261018)
    out = {}
    names = []
    for (name, w, h, kind, act) in MAP_CASES:
        n = w * h
        intra, imp = draw(rng, n, kind)
        dropped = 0
        for _ in range(8):                           # the pow guard: redraw what it drops
            bad = ~M.pow_guard(imp, intra)
            if not bad.any():
                break
            dropped += int(bad.sum())
            i2, p2 = draw(rng, n, kind)
            intra[bad], imp[bad] = i2[bad], p2[bad]
        assert M.pow_guard(imp, intra).all() and dropped <= max(1, n // 1000), (name, dropped)
        activity = None
        if act == "rand":
            activity = (16384 * 2.0 ** rng.uniform(-2, 2, n)).astype(np.uint32)
        elif act == "tiny":                          # Mul's lower clamp: products that round to 0
            activity = rng.integers(0, 3, n).astype(np.uint32)
        if only is not None and name not in only:
            continue
        dist, scores, ret, cfd = ref.frame(intra, imp, activity)
        k = "map_" + name
        out[k + "_shape"] = np.array([w, h], np.int32)
        out[k + "_intra"], out[k + "_imp"] = intra, imp
        if activity is not None:
            out[k + "_act"] = activity
        out[k + "_dist"], out[k + "_scores"] = dist, scores
        out[k + "_ret"] = np.array([ret], np.int64)
        out[k + "_pow_dropped"] = np.array([dropped], np.int32)
        out[k + "_centroids"] = ref.centroids(scores)
        names.append(name)
        print(name, w, h, "ret", ret, "dropped", dropped, flush=True)
        if name in SEG_CASES:
            rows = []
            for (q, bd) in QUANTIZERS:
                data, thr, mn, mx = ref.segmentation(scores, q, bd)
                rows.append(np.concatenate([[q, bd, mn, mx], data, thr]).astype(np.int64))
            out[k + "_seg"] = np.array(rows, np.int64)      # q, bd, min_segment, max_segment, data[8], threshold[7]
        if name in BLOCK_CASES:
            blocks = blocks_for(w, h)
            _, thr, _, _ = ref.segmentation(scores, 128, 8)
            res = []
            for mn in (0, 2):
                for b in blocks:
                    res.append(ref.block(cfd, w, h, int(b["bo_x"]), int(b["bo_y"]), int(b["bsize"]), thr, mn))
            out[k + "_blocks"] = blocks
            out[k + "_block_thr"] = thr
            out[k + "_block_out"] = np.array(res, np.int64).reshape(2, len(blocks), 2)   # [min_segment 0 / 2]
    # scores given directly: keys that land exactly on thresholds
    if only is None or "ties" in only:
        for t in range(3):
            s = tie_keys(rng)
            out["km_ties%d_scores" % t] = s
            out["km_ties%d_centroids" % t] = ref.centroids(s)
    out["ac_q"] = np.array([[ref.ac_q({}, q, 0, bd) for q in range(256)] for bd in (8, 10, 12)], np.uint16)
    out["names"] = np.array(names)
    L.save("scales_ref.npz", out)


if __name__ == "__main__":
    main()
