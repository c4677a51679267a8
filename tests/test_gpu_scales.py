"""csrc/scales.hip on the device, bit-exact: r1_frame_scales, r1_scale_kmeans, r1_segmentation_from_centroids and
r1_spatiotemporal_scale_batch on every case of tests/golden/scales_ref.npz (the reference's text, executed), on
random maps against tests/scales_model.py (which the same fixture pins), chained into r1_dist_scaled_batch, two
calls in flight on two streams, and the argument checks.

The one float of the chain is pow(frac, 1/3): random inputs are kept only where the DistortionScale does not depend
on the last 16 ulp of pow (scales_model.pow_guard, computed from the inputs, never from the device's answer)."""
import os

import numpy as np
import pytest

import scales_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "scales_ref.npz"))


def dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def run_frame(ctx, intra, imp, act, w, h):
    d, s, st = ctx.frame_scales(dev(intra).reshape(h, w), dev(np.asarray(imp, np.float32)).reshape(h, w),
                                dev(act).reshape(h, w) if act is not None else None)
    return d, s, st


def random_map(rng, n, with_act):
    """inputs that pass the pow guard (a block that does not gets importance 0: frac = 1 exactly)"""
    intra = rng.integers(0, 60000, n).astype(np.uint32)
    intra[rng.random(n) < 0.01] = 0
    imp = (intra * rng.random(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    bad = ~M.pow_guard(imp, intra)
    assert bad.sum() <= max(1, n // 1000)
    imp[bad] = 0
    act = (16384 * 2.0 ** rng.uniform(-3, 3, n)).astype(np.uint32) if with_act else None
    return intra, imp, act


def test_fixture_cases_through_the_four_entry_points(ctx, fx):
    for name in fx["names"].tolist():
        k = "map_" + name
        w, h = (int(v) for v in fx[k + "_shape"])
        act = fx[k + "_act"] if k + "_act" in fx.files else None
        d, s, st = run_frame(ctx, fx[k + "_intra"], fx[k + "_imp"], act, w, h)
        cent = ctx.scale_kmeans(s)
        assert np.array_equal(host_u32(d).ravel(), fx[k + "_dist"]), name
        assert np.array_equal(host_u32(s).ravel(), fx[k + "_scores"]), name
        log_sum, inv_mean, ret = ctx.scale_stats(st)
        assert ret == int(fx[k + "_ret"][0]), name
        want_sum, want_im = M.inv_mean(M.distortion_scale_for(fx[k + "_imp"], fx[k + "_intra"]) if act is None else
                                       M.ds_mul(M.distortion_scale_for(fx[k + "_imp"], fx[k + "_intra"]), act))
        assert (log_sum, inv_mean) == (want_sum, want_im), name
        assert np.array_equal(cent.cpu().numpy(), fx[k + "_centroids"]), name
        if k + "_seg" in fx.files:
            for row in fx[k + "_seg"]:
                q, bd, mn, mx = (int(v) for v in row[:4])
                got = ctx.segmentation_from_centroids(cent, q, bd)
                assert (got["min_segment"], got["max_segment"]) == (mn, mx), (name, q, bd)
                assert got["seg_delta"].tolist() == row[4:12].tolist(), (name, q, bd)
                assert got["threshold"].tolist() == row[12:19].tolist(), (name, q, bd)
        if k + "_blocks" in fx.files:
            blocks, thr = fx[k + "_blocks"], fx[k + "_block_thr"]
            a = dev(act).reshape(h, w) if act is not None else None
            for i, mn in enumerate((0, 2)):
                scale, sidx = ctx.spatiotemporal_scale_batch(d, a, blocks, thr, mn)
                want = fx[k + "_block_out"][i]
                assert np.array_equal(host_u32(scale), want[:, 0]), (name, mn)
                assert np.array_equal(sidx.cpu().numpy(), want[:, 1]), (name, mn)


def test_keys_on_thresholds(ctx, fx):
    for t in range(3):
        cent = ctx.scale_kmeans(dev(fx["km_ties%d_scores" % t]))
        assert np.array_equal(cent.cpu().numpy(), fx["km_ties%d_centroids" % t]), t


# 13 x 7: one workgroup, n no multiple of 64; 91 x 3: two workgroups of the per-block kernels; 480 x 270 (4K): 507
# workgroups in the reduction, 64 in the histogram
@pytest.mark.parametrize("w,h", [(13, 7), (91, 3), (480, 270)])
@pytest.mark.parametrize("with_act", [True, False])
def test_random_maps_equal_the_model(ctx, w, h, with_act):
    rng = np.random.default_rng(1000 * w + h + int(with_act))
    n = w * h
    intra, imp, act = random_map(rng, n, with_act)
    if (w, h) == (91, 3):
        imp[::7] *= np.float32(2.0 ** 40)            # keys far outside the histogram's LDS window
        imp[~M.pow_guard(imp, intra)] = 0
    d, s, st = run_frame(ctx, intra, imp, act, w, h)
    cent = ctx.scale_kmeans(s)
    wd, ws, (wsum, wim, wret) = M.frame_scales(intra, imp, act)
    assert np.array_equal(host_u32(d).ravel(), wd)
    assert np.array_equal(host_u32(s).ravel(), ws)
    assert ctx.scale_stats(st) == (wsum, wim, wret)
    assert np.array_equal(cent.cpu().numpy(), M.scale_kmeans(ws))
    # every 16x16 block of the frame (cut at the right / bottom edge where the map is odd), and a mix of all sizes
    xs, ys = np.meshgrid(np.arange(0, 2 * w, 4), np.arange(0, 2 * h, 4))
    blocks = np.zeros(xs.size, M.BLOCK)
    blocks["bo_x"], blocks["bo_y"], blocks["bsize"] = xs.ravel(), ys.ravel(), 6
    blocks = blocks[:4096]
    blocks["bsize"][::3] = rng.integers(0, 22, len(blocks[::3]))
    seg = ctx.segmentation_from_centroids(cent, 128, 8)
    a = dev(act).reshape(h, w) if act is not None else None
    scale, sidx = ctx.spatiotemporal_scale_batch(d, a, blocks, seg["threshold"], 1)
    wscale, wsidx = M.spatiotemporal_scale_batch(wd, act, w, h, blocks, seg["threshold"], 1)
    assert np.array_equal(host_u32(scale), wscale)
    assert np.array_equal(sidx.cpu().numpy(), wsidx)
    scale, sidx = ctx.spatiotemporal_scale_batch(d, a, blocks[:100], None, 3)      # no thresholds: min_segment
    assert np.array_equal(host_u32(scale), wscale[:100]) and (sidx.cpu().numpy() == 3).all()


def test_distortion_scales_feed_dist_scaled_batch(ctx):
    """distortion_scales_out IS the `scales` argument of the distortion entry points: the same r1_dist_scaled_batch
    call with the device-made grid and with the model's grid uploaded"""
    import torch
    from rav1e_amd.api import DIST_CAND, Plane
    rng = np.random.default_rng(5)
    intra, imp, act = random_map(rng, 64, True)
    d, _, _ = run_frame(ctx, intra, imp, act, 8, 8)
    wd, _, _ = M.frame_scales(intra, imp, act)
    org, ref = Plane(64, 64, 8), Plane(64, 64, 8)
    for p in (org, ref):
        p.data.copy_(torch.from_numpy(rng.integers(0, 256, tuple(p.data.shape)).astype(np.uint8)))
    c = np.zeros(40, DIST_CAND)
    c["ox"], c["oy"] = rng.integers(0, 49, 40), rng.integers(0, 49, 40)
    c["rx"], c["ry"] = rng.integers(0, 49, 40), rng.integers(0, 49, 40)
    for kind in (2, 3):
        got = ctx.dist_scaled_batch(kind, org, ref, 16, 16, c, scales=d)
        want = ctx.dist_scaled_batch(kind, org, ref, 16, 16, c, scales=dev(wd).reshape(8, 8))
        plain = ctx.dist_scaled_batch(kind, org, ref, 16, 16, c)
        assert torch.equal(got, want)
        assert not torch.equal(got, plain)           # the grid is in use


def test_two_calls_in_flight_on_two_streams(ctx):
    import torch
    rng = np.random.default_rng(9)
    cases = [random_map(rng, 480 * 270, True), random_map(rng, 480 * 270, False)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = []
    for (intra, imp, act), st in zip(cases, streams):
        with torch.cuda.stream(st):                  # inputs, outputs and scratch are this stream's own
            d, s, stats = run_frame(ctx, intra, imp, act, 480, 270)
            got.append((d, s, stats, ctx.scale_kmeans(s)))
    torch.cuda.synchronize()
    for (intra, imp, act), (d, s, stats, cent) in zip(cases, got):
        wd, ws, wstats = M.frame_scales(intra, imp, act)
        assert np.array_equal(host_u32(d).ravel(), wd) and np.array_equal(host_u32(s).ravel(), ws)
        assert ctx.scale_stats(stats) == wstats
        assert np.array_equal(cent.cpu().numpy(), M.scale_kmeans(ws))


def test_bad_arguments_are_refused(ctx):
    import torch
    L, EINVAL = ctx.lib, -1
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    f = torch.zeros(64, dtype=torch.float32, device="cuda")
    o1, o2 = torch.zeros_like(t), torch.zeros_like(t)
    stats = torch.zeros(24, dtype=torch.uint8, device="cuda")
    big = torch.zeros(int(L.r1_scale_kmeans_scratch_bytes(64)), dtype=torch.uint8, device="cuda")
    cent = torch.zeros(48, dtype=torch.int16, device="cuda")
    p = lambda x: x.data_ptr()     # noqa: E731
    assert L.r1_frame_scales_scratch_bytes(0) < 0 and L.r1_scale_kmeans_scratch_bytes(-3) < 0
    for n in (0, -1):
        assert L.r1_frame_scales(ctx.h, p(t), p(f), None, n, p(o1), p(o2), p(stats), p(big), big.numel(), None) == EINVAL
        assert L.r1_scale_kmeans(ctx.h, p(t), n, p(cent), p(big), big.numel(), None) == EINVAL
    need = int(L.r1_frame_scales_scratch_bytes(64))
    assert L.r1_frame_scales(ctx.h, p(t), p(f), None, 64, p(o1), p(o2), p(stats), p(big), need - 1, None) == EINVAL
    assert L.r1_scale_kmeans(ctx.h, p(t), 64, p(cent), p(big), big.numel() - 1, None) == EINVAL
    blocks = np.zeros(3, M.BLOCK)
    s, i = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda")

    def call(b, n=3):
        return L.r1_spatiotemporal_scale_batch(ctx.h, p(t), None, 8, 8, b.ctypes.data, n, None, 0, p(s), p(i), None)
    assert call(blocks, 0) == EINVAL
    for bad in (22, -1, 255):
        b = blocks.copy()
        b["bsize"][1] = bad
        assert call(b) == EINVAL
    b = blocks.copy()
    b["bo_x"][2] = 16                                # the map is 8 importance blocks wide: 4x4 column 16 is outside
    assert call(b) == EINVAL
    assert call(blocks) == 0
    torch.cuda.synchronize()
