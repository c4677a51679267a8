"""NumPy / Python-int restatement of the reference's temporal-RDO scale chain (TEST INFRASTRUCTURE): what
r1_frame_scales, r1_scale_kmeans, r1_segmentation_from_centroids and r1_spatiotemporal_scale_batch compute.

  distortion_scale_for, DistortionScale::{new, From<f64>, Mul, inv_mean, blog16, blog64}   src/rdo.rs:506-658
  compute_spatiotemporal_scores / compute_temporal_scores                                   src/encoder.rs:744-777
  blog32_q11, bexp64, blog64                                                                src/util/logexp.rs
  kmeans                                                                                    src/util/kmeans.rs
  segmentation_optimize_inner, update_threshold                  src/segmentation.rs:77-160, src/encoder.rs:566-580
  spatiotemporal_scale, segment_idx_from_distortion              src/rdo.rs:464-504, src/segmentation.rs:192-196

tests/golden/scales_ref.npz (the reference's text, executed) pins every function here; the GPU tests and
tools/bench_scales.py then use this model on inputs the fixture does not hold.  Per-block work is vectorised;
what runs once per frame is plain Python integers."""
import numpy as np

SHIFT = 14
DS_MAX = (1 << 28) - 1
ONE = 1 << SHIFT
U64_MAX = (1 << 64) - 1

# BlockSize (src/partition.rs:130-153) -> (width, height) in pixels
BLOCK_DIMS = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64),
              (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64),
              (64, 16)]
BLOCK = np.dtype([("bo_x", "<i4"), ("bo_y", "<i4"), ("bsize", "<i4")])

ATANH_LOG2 = [
    0x32B803473F7AD0F4, 0x2F2A71BD4E25E916, 0x2E68B244BB93BA06, 0x2E39FB9198CE62E4, 0x2E2E683F68565C8F,
    0x2E2B850BE2077FC1, 0x2E2ACC58FE7B78DB, 0x2E2A9E2DE52FD5F2, 0x2E2A92A338D53EEC, 0x2E2A8FC08F5E19B6,
    0x2E2A8F07E51A485E, 0x2E2A8ED9BA8AF388, 0x2E2A8ECE2FE7384A, 0x2E2A8ECB4D3E4B1A, 0x2E2A8ECA94940FE8,
    0x2E2A8ECA6669811D, 0x2E2A8ECA5ADEDD6A, 0x2E2A8ECA57FC347E, 0x2E2A8ECA57438A43, 0x2E2A8ECA57155FB4,
    0x2E2A8ECA5709D510, 0x2E2A8ECA5706F267, 0x2E2A8ECA570639BD, 0x2E2A8ECA57060B92, 0x2E2A8ECA57060008,
    0x2E2A8ECA5705FD25, 0x2E2A8ECA5705FC6C, 0x2E2A8ECA5705FC3E, 0x2E2A8ECA5705FC33, 0x2E2A8ECA5705FC30,
    0x2E2A8ECA5705FC2F, 0x2E2A8ECA5705FC2F]


def _tdiv(a, b):
    """i64 division as Rust has it: toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def q57(v):
    return v << 57


def bexp64(logq57):
    ipart = logq57 >> 57
    if ipart < 0:
        return 0
    if ipart >= 63:
        return 0x7FFFFFFFFFFFFFFF
    z = logq57 - q57(ipart)
    if z != 0:
        z <<= 5
        w = 0x26A3D0E401DD846D
        i = 0
        for stop in (3, 12):            # iterations 4 and 13 run twice
            while True:
                mask = -int(z < 0)
                w += ((w >> (i + 1)) + mask) ^ mask
                z -= (ATANH_LOG2[i] + mask) ^ mask
                if i >= stop:
                    break
                z *= 2
                i += 1
        while i < 32:
            mask = -int(z < 0)
            w += ((w >> (i + 1)) + mask) ^ mask
            z = (z - ((ATANH_LOG2[i] + mask) ^ mask)) * 2
            i += 1
        wlo = 0
        if ipart > 30:
            while True:
                mask = -int(z < 0)
                wlo = _i32(wlo + _i32(((w >> i) + mask) ^ mask))
                z -= (ATANH_LOG2[31] + mask) ^ mask
                if i >= 39:             # iteration 40 runs twice
                    break
                z *= 2
                i += 1
            while i < 61:
                mask = -int(z < 0)
                wlo = _i32(wlo + _i32(((w >> i) + mask) ^ mask))
                z = (z - ((ATANH_LOG2[31] + mask) ^ mask)) * 2
                i += 1
        w = (w << 1) + wlo
    else:
        w = 1 << 62
    if ipart < 62:
        w = ((w >> (61 - ipart)) + 1) >> 1
    return w


def blog64(n):
    if n <= 0:
        return -1
    ipart = n.bit_length() - 1
    w = n >> (ipart - 61) if ipart > 61 else n << (61 - ipart)
    if w & (w - 1) == 0:
        return q57(ipart)
    z = 0
    x, y = w + (1 << 61), w - (1 << 61)
    i = 0
    for end in (3, 12, 39, 61):
        while True:
            mask = -int(y < 0)
            z += ((ATANH_LOG2[min(i, 31)] >> i) + mask) ^ mask
            u = x >> (i + 1)
            x -= ((y >> (i + 1)) + mask) ^ mask
            y -= (u + mask) ^ mask
            if i == end:
                break
            i += 1
    return q57(ipart) + ((z + 8) >> 4)


def blog32_q11(w):
    """vectorised; w: array of u32 values -> int64 array"""
    w = np.asarray(w).astype(np.int64)
    ipart = np.frexp(w.astype(np.float64))[1].astype(np.int64)      # 32 - leading_zeros for w > 0
    sh = ipart - 16
    n = np.where(sh > 0, w >> np.maximum(sh, 0), w << np.maximum(-sh, 0)) - 32768 - 16384
    fpart = ((n * (((n * (((n * (((n * -1402) >> 15) + 2546)) >> 15) - 5216)) >> 15) + 15745)) >> 15) - 6797
    return np.where(w == 0, -1, (ipart << 11) + (fpart >> 3))


def blog16(s):
    return (blog32_q11(s) - (SHIFT << 11)).astype(np.int16)


def ds_new(num, den):
    """DistortionScale::new on Python ints"""
    raw = min(((num << SHIFT) & U64_MAX) + den // 2, U64_MAX) // den
    return min(raw, DS_MAX)


def ds_mul(a, b):
    a = np.asarray(a).astype(np.uint64)
    b = np.asarray(b).astype(np.uint64)
    return np.clip((a * b + np.uint64(1 << (SHIFT - 1))) >> np.uint64(SHIFT), 1, DS_MAX).astype(np.uint32)


def ds_from_f64(scale):
    """From<f64> for DistortionScale, vectorised (`as u64` saturates; NaN -> 0)"""
    v = np.asarray(scale, np.float64) * 32768.0
    zero = ~(v > 0.0)
    big = v >= 2.0 ** 64
    num = np.where(zero | big, 0.0, v).astype(np.uint64)
    num = np.where(big, np.uint64(U64_MAX), num)
    sh = num << np.uint64(SHIFT)                                    # wraps, like the reference's <<
    half = np.uint64(1 << 14)
    summed = np.where(sh > np.uint64(U64_MAX) - half, np.uint64(U64_MAX), sh + half)
    return np.minimum(summed // np.uint64(1 << 15), np.uint64(DS_MAX)).astype(np.uint32)


def _frac_pow(intra, importance):
    intra = np.asarray(intra).astype(np.float64)
    prop = np.asarray(importance, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.power((intra + prop) / intra, 1.0 / 3.0)


def distortion_scale_for(importance, intra):
    """per block: (f32 importance, u32 intra cost) -> DistortionScale"""
    d = ds_from_f64(_frac_pow(intra, importance))
    return np.where(np.asarray(intra) == 0, np.uint32(ONE), d).astype(np.uint32)


def pow_guard(importance, intra, ulps=16):
    """True where the block's DistortionScale does not depend on the last `ulps` ulp of pow's result: the
    inputs a fixture or a GPU test may keep.  Computed from the inputs alone."""
    s = _frac_pow(intra, importance)
    with np.errstate(invalid="ignore"):
        step = ulps * np.spacing(s)
        ok = (ds_from_f64(s - step) == ds_from_f64(s)) & (ds_from_f64(s + step) == ds_from_f64(s))
    return ok | (np.asarray(intra) == 0)


def inv_mean(scales):
    """-> (sum of blog32_q11, inv_mean.0)"""
    s = int(blog32_q11(scales).sum())
    log_inv_mean_q11 = (SHIFT << 11) - _tdiv(s, len(scales))
    return s, min(max(bexp64((log_inv_mean_q11 + (SHIFT << 11)) << (57 - 11)), 1), DS_MAX)


def frame_scales(intra, importance, activity=None):
    """-> (distortion_scales, spatiotemporal_scores, (sum, inv_mean, log_isqrt_mean_scale))"""
    d = distortion_scale_for(np.ravel(importance), np.ravel(intra))
    scores = d if activity is None else ds_mul(d, np.ravel(activity))
    s, im = inv_mean(scores)
    return ds_mul(d, im), ds_mul(scores, im), (s, im, (blog64(im) - q57(SHIFT)) >> 1)


# ---------------------------------------------------------------- k-means
def kmeans_sorted(data, k, bias=1):
    """src/util/kmeans.rs as written: `data` sorted; Python ints.  bias: the `+ 1` of the threshold (0: the
    mutation the fixture's tie cases are chosen to notice)"""
    data = [int(v) for v in data]
    n = len(data)
    low = [(i * (n - 1)) // (k - 1) for i in range(k)]
    means = [data[i] for i in low]
    high = list(low)
    total = [0] * k
    high[k - 1] = n
    total[k - 1] = means[k - 1]
    for _ in range(2 * n.bit_length()):
        for i in range(k - 1):
            t = (means[i + 1] + means[i] + bias) >> 1
            m, s = high[i], total[i]
            while m > 0 and data[m - 1] > t:
                s -= data[m - 1]
                m -= 1
            while m < n and data[m] <= t:
                s += data[m]
                m += 1
            high[i], total[i] = m, s
            m, s = low[i + 1], total[i + 1]
            while m < n and data[m] < t:
                s -= data[m]
                m += 1
            while m > 0 and data[m - 1] >= t:
                s += data[m - 1]
                m -= 1
            low[i + 1], total[i + 1] = m, s
        changed = False
        for i in range(k):
            count = high[i] - low[i]
            if count == 0:
                continue
            new = _tdiv(total[i] + (count >> 1), count)
            changed |= means[i] != new
            means[i] = new
        if not changed:
            break
    return means


KEY_MIN = -(SHIFT << 11)      # blog16(1); blog16(2^28 - 1) = KEY_MIN + KEY_BINS - 1 (the quartic's fraction reaches 0)
KEY_BINS = (28 << 11) + 1


def kmeans_hist(keys, k):
    """the same centroids from a histogram of the keys: inclusive prefix counts C and prefix sums S stand
    in for the sorted array (high = #{d <= t} = C[t], low = #{d < t} = C[t - 1], sums are differences of S)"""
    keys = np.asarray(keys).astype(np.int64)
    n = len(keys)
    hist = np.bincount(keys - KEY_MIN, minlength=KEY_BINS)
    assert len(hist) == KEY_BINS
    cnt = np.cumsum(hist)
    tot = np.cumsum(hist * (np.arange(KEY_BINS) + KEY_MIN))

    def upto(t):      # (#{d <= t}, their sum)
        b = min(t - KEY_MIN, KEY_BINS - 1)
        return (0, 0) if b < 0 else (int(cnt[b]), int(tot[b]))
    means = [int(np.searchsorted(cnt, (i * (n - 1)) // (k - 1), side="right")) + KEY_MIN for i in range(k)]
    for _ in range(2 * n.bit_length()):
        thr = [(means[i + 1] + means[i] + 1) >> 1 for i in range(k - 1)]
        changed = False
        new_means = list(means)
        for i in range(k):
            lo = upto(thr[i - 1] - 1) if i > 0 else (0, 0)
            hi = upto(thr[i]) if i < k - 1 else (n, int(tot[-1]))
            count = hi[0] - lo[0]
            if count == 0:
                continue
            new_means[i] = _tdiv(hi[1] - lo[1] + (count >> 1), count)
            changed |= new_means[i] != means[i]
        means = new_means
        if not changed:
            break
    return means


def scale_kmeans(scores, sorted_form=False):
    """-> (6, 8) int16: the centroids for k = 8, 7, ..., 3, unused entries 0"""
    keys = blog16(scores)
    out = np.zeros((6, 8), np.int16)
    data = np.sort(keys) if sorted_form else keys
    for row, k in enumerate(range(8, 2, -1)):
        out[row, :k] = kmeans_sorted(data, k) if sorted_form else kmeans_hist(data, k)
    return out


# ---------------------------------------------------------------- segmentation
def _bd_index(bit_depth):
    return min((bit_depth ^ 8) >> 1, 2)


def ac_q(tables, qindex, delta_q, bit_depth):
    return int(tables[_bd_index(bit_depth)][min(max(qindex + delta_q, 0), 255)])


def select_ac_qi(tables, quantizer, bit_depth):
    t = [int(v) for v in tables[_bd_index(bit_depth)]]
    if quantizer < t[0]:
        return 0
    if quantizer >= t[255]:
        return 255
    import bisect
    qi = bisect.bisect_left(t, quantizer)
    if t[qi] == quantizer:
        return qi
    return qi - 1 if quantizer * quantizer < t[qi - 1] * t[qi] else qi


def _i8(v):
    v &= 0xFF
    return v - 256 if v >= 128 else v


def segmentation_from_centroids(tables, centroids, base_q_idx, bit_depth):
    """tables: (3, 256) ac_qlookup (8 / 10 / 12-bit).  -> dict(position, max_segment, min_segment, data[8],
    threshold[7]) as segmentation_optimize_inner + update_threshold leave them"""
    c = [[int(v) for v in centroids[r][:8 - r]] for r in range(6)]

    def var(row):
        delta = [row[i] - row[i + 1] for i in range(len(row) - 1)]
        mean = _tdiv(sum(delta), len(delta))
        return sum((d - mean) ** 2 for d in delta)
    variance = [var(r) for r in c]
    position = max(i for i, v in enumerate(variance) if v == min(variance))
    log2_base = blog64(ac_q(tables, base_q_idx, 0, bit_depth))
    lower = 1 - base_q_idx
    data = [0] * 8
    sel = c[position]
    for i, key in enumerate(reversed(sel)):
        q = bexp64(log2_base - (key << (57 - 11 - 1)))
        data[i] = max(max(select_ac_qi(tables, q, bit_depth), 1) - base_q_idx, lower)
    max_segment = len(sel) - 1
    base = ac_q(tables, base_q_idx, 0, bit_depth)
    real = [ac_q(tables, base_q_idx, _i8(data[i]), bit_depth) for i in range(max_segment + 1)]
    thr = [0] * 7
    for i in range(max_segment):
        thr[i] = ds_new(base * base, real[i + 1] * real[i])
    return {"position": position, "max_segment": max_segment, "min_segment": 0, "data": data, "threshold": thr}


# ---------------------------------------------------------------- per coded block
def spatiotemporal_scale_batch(distortion, activity, w_in_imp_b, h_in_imp_b, blocks, thresholds=None, min_segment=0):
    """blocks: BLOCK records.  -> (scale u32[n], sidx u8[n]); sidx is 0 without thresholds"""
    d = np.asarray(distortion).astype(np.uint64).reshape(h_in_imp_b, w_in_imp_b)
    a = (np.full_like(d, ONE) if activity is None else
         np.asarray(activity).astype(np.uint64).reshape(h_in_imp_b, w_in_imp_b))
    prod = d * a
    scale = np.zeros(len(blocks), np.uint32)
    sidx = np.zeros(len(blocks), np.uint8)
    for i, b in enumerate(blocks):
        bw, bh = BLOCK_DIMS[int(b["bsize"])]
        x0, y0 = int(b["bo_x"]) >> 1, int(b["bo_y"]) >> 1
        x1, y1 = min(x0 + max(bw >> 3, 1), w_in_imp_b), min(y0 + max(bh >> 3, 1), h_in_imp_b)
        den = ((x1 - x0) * (y1 - y0)) << SHIFT
        s = (int(prod[y0:y1, x0:x1].sum()) + (den >> 1)) // den
        scale[i] = s & 0xFFFFFFFF
        if thresholds is not None:
            # partition_point of `s < t` over all seven entries, the zero ones included.  update_threshold's
            # entries never increase, so the predicate is partitioned and the point is the length of the
            # leading run of true
            lo = 0
            while lo < 7 and int(scale[i]) < int(thresholds[lo]):
                lo += 1
            sidx[i] = max(lo, min_segment)
    return scale, sidx
