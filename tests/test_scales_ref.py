"""The temporal-RDO scale chain without a GPU: tests/scales_model.py against every array of
tests/golden/scales_ref.npz (the reference's text, executed: tests/golden/gen_scales_ref.py), the two k-means forms
(sorted array as the reference has it / histogram with prefix tables as the device has it) against each other, and
the library's host function r1_segmentation_from_centroids against the executed segmentation_optimize_inner +
update_threshold.  Where the reference tree is present: its own kmeans and logexp unit tests under the transpiler,
and the check that the fixture follows kmeans' text (the rounding of its threshold)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scales_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
sys.path.insert(0, os.path.join(ROOT, "tools"))       # rustlite, for the tests that execute reference text
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "scales_ref.npz"))


def map_case(fx, name):
    k = "map_" + name
    w, h = fx[k + "_shape"]
    act = fx[k + "_act"] if k + "_act" in fx.files else None
    return int(w), int(h), fx[k + "_intra"], fx[k + "_imp"], act


def test_fixture_holds_the_cases(fx):
    names = set(fx["names"].tolist())
    assert names == {"one", "two", "two_t", "odd", "odd_t", "zero_intra", "zero_imp", "clamp_hi", "clamp_lo",
                     "two_clusters", "big", "big_t"}
    for n in names:
        w, h, intra, imp, act = map_case(fx, n)
        assert M.pow_guard(imp, intra).all(), n                      # every kept input passes the +-16 ulp guard
        assert int(fx["map_%s_pow_dropped" % n][0]) <= max(1, w * h // 1000)
    assert (fx["map_clamp_hi_dist"] == M.ds_mul(M.DS_MAX, M.inv_mean(M.distortion_scale_for(
        fx["map_clamp_hi_imp"], fx["map_clamp_hi_intra"]))[1])).sum() > 50      # From<f64> saturated
    d = M.distortion_scale_for(fx["map_clamp_lo_imp"], fx["map_clamp_lo_intra"])
    raw = (d.astype(np.uint64) * fx["map_clamp_lo_act"] + 8192) >> 14
    assert (raw == 0).any()                                          # Mul's lower clamp was hit
    assert len(set(fx["map_zero_imp_scores"].tolist())) == 1


def test_model_equals_the_executed_maps(fx):
    for n in fx["names"].tolist():
        w, h, intra, imp, act = map_case(fx, n)
        dist, scores, (s, im, ret) = M.frame_scales(intra, imp, act)
        assert np.array_equal(dist, fx["map_%s_dist" % n]), n
        assert np.array_equal(scores, fx["map_%s_scores" % n]), n
        assert ret == int(fx["map_%s_ret" % n][0]), n


def test_model_equals_the_executed_kmeans_in_both_forms(fx):
    cases = [("map_%s" % n) for n in fx["names"].tolist()] + ["km_ties%d" % t for t in range(3)]
    for k in cases:
        want = fx[k + "_centroids"]
        assert np.array_equal(M.scale_kmeans(fx[k + "_scores"], sorted_form=True), want), k
        assert np.array_equal(M.scale_kmeans(fx[k + "_scores"], sorted_form=False), want), k


def test_kmeans_forms_agree_on_random_keys():
    rng = np.random.default_rng(7)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        if trial % 3 == 0:      # few distinct values: thresholds land on keys, clusters run empty
            keys = rng.choice(rng.integers(-3000, 3000, int(rng.integers(1, 9))), n)
        elif trial % 3 == 1:
            keys = rng.integers(M.KEY_MIN, M.KEY_MIN + M.KEY_BINS, n)
        else:
            keys = np.round(rng.normal(0, 700, n)).astype(np.int64)
        data = np.sort(keys)
        for k in range(3, 9):
            assert M.kmeans_sorted(data, k) == M.kmeans_hist(keys, k), (trial, k)


def test_all_equal_scores_pick_three_segments(fx):
    """every variance is 0: rposition takes the LAST minimal one, k = 3"""
    seg = fx["map_zero_imp_seg"]
    assert (seg[:, 3] == 2).all()


def seg_rows(fx):
    for n in fx["names"].tolist():
        k = "map_%s_seg" % n
        if k in fx.files:
            for row in fx[k]:
                yield n, fx["map_%s_centroids" % n], row


def test_model_segmentation_equals_the_executed(fx):
    rows = list(seg_rows(fx))
    assert len(rows) == 5 * 12
    for n, cent, row in rows:
        q, bd, mn, mx = (int(v) for v in row[:4])
        got = M.segmentation_from_centroids(fx["ac_q"], cent, q, bd)
        assert (got["min_segment"], got["max_segment"]) == (mn, mx), (n, q, bd)
        assert got["data"] == row[4:12].tolist(), (n, q, bd)
        assert got["threshold"] == row[12:19].tolist(), (n, q, bd)


def test_library_segmentation_from_centroids_equals_the_executed(fx):
    """r1_segmentation_from_centroids through ctypes: a host function, no GPU"""
    import ctypes as C
    from rav1e_amd import _lib
    L = _lib.load()
    for n, cent, row in seg_rows(fx):
        q, bd, mn, mx = (int(v) for v in row[:4])
        out = _lib.R1SegmentationData()
        c = np.ascontiguousarray(cent, np.int16)
        assert L.r1_segmentation_from_centroids(c.ctypes.data, q, bd, C.byref(out)) == 0
        assert (out.min_segment, out.max_segment, out.k, out.position) == (mn, mx, mx + 1, 7 - mx), (n, q, bd)
        assert out.seg_delta[:] == row[4:12].tolist(), (n, q, bd)
        assert out.threshold[:] == row[12:19].tolist(), (n, q, bd)
    out = _lib.R1SegmentationData()
    c = np.zeros(48, np.int16)
    assert L.r1_segmentation_from_centroids(c.ctypes.data, 100, 9, C.byref(out)) == -1      # R1_EINVAL
    assert L.r1_segmentation_from_centroids(c.ctypes.data, 256, 8, C.byref(out)) == -1
    assert L.r1_segmentation_from_centroids(None, 100, 8, C.byref(out)) == -1


def test_model_blocks_equal_the_executed(fx):
    for n in ("odd", "big_t"):
        w, h, intra, imp, act = map_case(fx, n)
        blocks = fx["map_%s_blocks" % n]
        assert len(blocks) == 22 * 5 and set(blocks["bsize"].tolist()) == set(range(22))
        for i, mn in enumerate((0, 2)):
            scale, sidx = M.spatiotemporal_scale_batch(fx["map_%s_dist" % n], act, w, h, blocks,
                                                       fx["map_%s_block_thr" % n], mn)
            want = fx["map_%s_block_out" % n][i]
            assert np.array_equal(scale, want[:, 0]), (n, mn)
            assert np.array_equal(sidx, want[:, 1]), (n, mn)
        assert len(set(fx["map_%s_block_out" % n][0][:, 1].tolist())) >= 2      # more than one segment is met


# ---------------------------------------------------------------- the reference's own tests, under the transpiler
def _crate(rel, text=None):
    from rustlite.transpile import Crate
    c = Crate(REF)
    if text is None:
        c.load(rel, tests=True)
    else:
        c.load_text("<%s, loops thinned>" % rel, text)
    return c


@needs_ref
@pytest.mark.parametrize("name,g", [("three_means", {"K": 3, "T": "i32"}), ("four_means", {"K": 4, "T": "i32"})])
def test_reference_kmeans_unit_tests(name, g):
    """src/util/kmeans.rs:104-123; rustc infers K and T from the expected array, the transpiler is told"""
    from rustlite import runtime as R
    c = _crate("util/kmeans.rs")
    R.TRY_INTO_TARGET = "i32"
    try:
        c.get(name)(g)
    finally:
        R.TRY_INTO_TARGET = None


@needs_ref
@pytest.mark.parametrize("name", ["blog64_vectors", "bexp64_vectors", "blog32_vectors", "bexp_q24_vectors"])
def test_reference_logexp_vectors(name):
    _crate("util/logexp.rs").get(name)({})


@needs_ref
@pytest.mark.parametrize("name", ["blog64_bexp64_round_trip", "blog32_bexp_q24_round_trip",
                                  "blog32_q11_bexp32_q10_round_trip"])
def test_reference_logexp_round_trips(name):
    """src/util/logexp.rs:304-359 with ONE textual change: the loops over 1..=MAX take every 97th value (the whole
    range is a minute of transpiled Python per test), `for a in R {` -> `for a in (R).step_by(97) {`"""
    import re
    src = open(os.path.join(REF, "util/logexp.rs")).read()
    thin, k = re.subn(r"for a in (1\.\.=std::[iu]16::MAX as [iu]\d+) \{", r"for a in (\1).step_by(97) {", src)
    assert k == 3
    _crate("util/logexp.rs", thin.replace("#[cfg(test)]", "")).get(name)({})


@needs_ref
def test_fixture_follows_the_kmeans_text(fx, tmp_path):
    """the threshold's rounding: with `(c1 + c2 + 1) >> 1` of kmeans.rs:35 changed to `(c1 + c2) >> 1` in a scratch
    copy of src/, the generator's centroids for the keys that sit on thresholds change"""
    import shutil
    src = tmp_path / "src"
    shutil.copytree(REF, src)
    text = open(os.path.join(REF, "util/kmeans.rs")).read()
    old = "((c1.into() + c2.into() + 1) >> 1)"
    assert text.count(old) == 1
    (src / "util/kmeans.rs").write_text(text.replace(old, "((c1.into() + c2.into()) >> 1)"))
    gen = os.path.join(ROOT, "tests", "golden", "gen_scales_ref.py")
    env = dict(os.environ, R1_REF_SRC=str(src), R1_GOLDEN_OUT=str(tmp_path), R1_SCALES_CASES="ties")
    subprocess.run([sys.executable, gen], check=True, env=env, cwd=os.path.dirname(gen), stdout=subprocess.DEVNULL,
                   timeout=300)
    m = np.load(tmp_path / "scales_ref.npz")
    assert all(np.array_equal(m["km_ties%d_scores" % t], fx["km_ties%d_scores" % t]) for t in range(3))
    assert any(not np.array_equal(m["km_ties%d_centroids" % t], fx["km_ties%d_centroids" % t]) for t in range(3))
