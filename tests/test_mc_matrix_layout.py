"""The horizontal 8-tap pass of the 8-bit fused candidate kernels on the matrix pipe (mc8_column_t<.., MXNC>,
rav1e_amd/csrc/cand_common.hpp; geometry and band builder r1mc::mx_*, mc_window.hpp; rdo_mc_matrix, rdo_cand_plan.hpp),
on the host.  A host program (tests/c/mc_matrix_list.cpp, the host compiler alone) prints the fragment geometry, the
band of every row of the packed tap table for every lane, and the plan's choices; here a NumPy restatement of
v_mfma_i32_16x16x32_i8 -- lane l supplies A[l % 16][8 (l / 16) .. + 7] and B[8 (l / 16) .. + 7][l % 16], receives
D[4 (l / 16) + {0 .. 3}][l % 16], int32 accumulation -- runs the kernel's quads over a model of its LDS and must hand
every lane the accumulators hacc of its own column:

    hacc(row) = 8192 + 2 + 32 + sum_t h[t] * q[row][column + t],      h = taps / 2, q = pixel - 128 as staged.

Both layouts that ship are modelled: one candidate per wave (64x64) and two (32x32: two chained MFMAs, the other
candidate's row groups read the zeroed shadow)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rav1e_amd", "csrc")
BIAS = 8192 + 2 + 32
LAYOUTS = (1, 2)                # candidates per wave of the layouts that ship


def _table():
    src = open(os.path.join(CSRC, "mc_common.hpp")).read()
    m = re.search(r"kSubpel\[6\]\[16\]\[8\] = \{(.*?)\};", src, re.S)
    t = np.array([int(v) for v in re.findall(r"-?\d+", m.group(1))], np.int64).reshape(6, 16, 8)
    assert (t.sum(axis=2) == 128).all() and (t % 2 == 0).all()
    return t


HALF = _table() // 2            # the half-taps h, all within int8


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mc_matrix") / "mc_matrix_list")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-variable", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "c", "mc_matrix_list.cpp")])
    out = {"P": {}, "Q": {}, "G": {}, "T": {}, "B": {}}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        v = [int(x) for x in v]
        if k == "P":
            out["P"][v[0], v[1]] = dict(zip(("nc", "ws", "win", "src_off", "src", "zero_off", "zero", "lds"), v[2:]))
        elif k == "Q":
            out["Q"][v[0]] = dict(zip(("h", "ws", "quads", "a_end", "zero"), v[1:]))
        elif k == "G":
            out["G"][v[0], v[1]] = (v[2], v[3])
        elif k == "T":
            out["T"][v[0], v[1]] = (v[2], v[3])
        else:
            out["B"][v[0], v[1], v[2]] = v[3]
    assert len(out["B"]) == 6 * 16 * 64 and len(out["G"]) == 2 * 64
    return out


def le_bytes(x, n):
    return np.frombuffer(int(x).to_bytes(n, "little"), np.int8).astype(np.int32)


def mfma(a, b, c):
    """v_mfma_i32_16x16x32_i8 on per-lane operands: a, b (64, 8) int8 values, c (64, 4) int32 -> d (64, 4)"""
    lane = np.arange(64)
    A = np.zeros((16, 32), np.int64)
    B = np.zeros((32, 16), np.int64)
    Cm = np.zeros((16, 16), np.int64)
    for i in range(8):
        A[lane % 16, 8 * (lane // 16) + i] = a[:, i]
        B[8 * (lane // 16) + i, lane % 16] = b[:, i]
    for k in range(4):
        Cm[4 * (lane // 16) + k, lane % 16] = c[:, k]
    D = A @ B + Cm
    assert np.abs(D).max() < (1 << 31)
    return np.stack([D[4 * (lane // 16) + k, lane % 16] for k in range(4)], axis=1)


def test_plan_turns_the_pass_on_at_the_two_sizes_built(listed):
    on = {k: p["nc"] for k, p in listed["P"].items() if p["nc"]}
    assert on == {(8, 6): 1, (8, 5): 2}
    for (bd, wl), p in listed["P"].items():
        if not p["nc"]:
            continue
        q = listed["Q"][p["nc"]]
        assert (q["h"], q["ws"]) == (1 << wl, p["ws"]) and p["ws"] % 8 == 0
        assert q["a_end"] <= p["lds"]                                # the furthest A byte lies in the allocation
        assert p["src_off"] >= p["win"]
        if p["nc"] == 2:                                              # the shadow: behind the source, inside the LDS
            assert p["zero"] == q["zero"] and p["zero_off"] % 16 == 0
            assert p["zero_off"] >= p["src_off"] + p["src"] and p["zero_off"] + p["zero"] <= p["lds"]
        else:
            assert p["zero"] == 0


def test_band_is_the_half_taps_on_the_diagonal(listed):
    """byte b of lane l's B fragment is B[K = 8 (l / 16) + b][N = l % 16] = h[K - N] for 0 <= K - N < 8, else 0: every
    filter set, every fraction, every lane"""
    for f in range(6):
        for q in range(16):
            h = HALF[f, q]
            fx0, fx1 = listed["T"][f, q]
            assert np.array_equal(np.concatenate([le_bytes(fx0, 4), le_bytes(fx1, 4)]), h)   # what the kernels load
            for l in range(64):
                got = le_bytes(listed["B"][f, q, l], 8)
                for b in range(8):
                    d = 8 * (l // 16) + b - l % 16
                    assert got[b] == (h[d] if 0 <= d < 8 else 0), (f, q, l, b)


class Wave:
    """the LDS of one wave of the layout with nc candidates, and the kernel's quads over it"""

    def __init__(self, listed, nc, rng):
        self.nc, self.q = nc, listed["Q"][nc]
        self.h = self.w = self.q["h"]
        self.ws = self.q["ws"]
        self.p = listed["P"][8, {1: 6, 2: 5}[nc]]
        self.lds = rng.integers(-128, 128, self.p["lds"]).astype(np.int8)      # whatever lies there
        if nc == 2:
            self.lds[self.p["zero_off"]: self.p["zero_off"] + self.p["zero"]] = 0
        self.geom = [listed["G"][nc, l] for l in range(64)]
        self.listed = listed

    def window(self, cand):
        """view of candidate cand's staged window, (h + 7) x ws"""
        o = cand * (self.h + 7) * self.ws
        return self.lds[o: o + (self.h + 7) * self.ws].reshape(self.h + 7, self.ws)

    def valid_mask(self):
        """bytes the result may depend on: the windows' (h + 7) x (w + 7) pixels and the shadow"""
        m = np.zeros(len(self.lds), bool)
        for cand in range(self.nc):
            o = cand * (self.h + 7) * self.ws
            v = m[o: o + (self.h + 7) * self.ws].reshape(self.h + 7, self.ws)
            v[:, : self.w + 7] = True
        if self.nc == 2:
            m[self.p["zero_off"]: self.p["zero_off"] + self.p["zero"]] = True
        return m

    def run(self, rows):
        """rows: (filter set, fraction) per candidate -> hacc as the lanes receive it, (64, 4 * quads), and the set of
        LDS bytes read"""
        read = np.zeros(len(self.lds), bool)
        cbias = np.full((64, 4), BIAS, np.int64)
        out = []
        for quad in range(self.q["quads"]):
            d = cbias
            for m in range(self.nc):                    # one MFMA per candidate, chained through D
                a = np.zeros((64, 8), np.int64)
                for l, (off, cand) in enumerate(self.geom):
                    base = off if cand == m else self.p["zero_off"]
                    lo = base + quad * 4 * self.ws
                    assert lo % 8 == 0 and lo + 8 <= len(self.lds)
                    assert cand == m or lo + 8 <= self.p["zero_off"] + self.p["zero"]
                    a[l] = self.lds[lo: lo + 8]
                    read[lo: lo + 8] = True
                b = np.array([le_bytes(self.listed["B"][rows[m][0], rows[m][1], l], 8) for l in range(64)])
                d = mfma(a, b, d)
            out.append(d)
        return np.concatenate(out, axis=1), read

    def hacc(self, rows):
        """the accumulators of every lane's own column, rows 0 .. h + 6: (64, h + 7)"""
        want = np.zeros((64, self.h + 7), np.int64)
        for l in range(64):
            cand, c = l // self.w, l % self.w
            win = self.window(cand).astype(np.int64)
            h = HALF[rows[cand]]
            want[l] = BIAS + sum(h[t] * win[:, c + t] for t in range(8))
        return want


@pytest.mark.parametrize("nc", LAYOUTS)
def test_every_lane_receives_hacc_of_its_own_column(listed, nc):
    rng = np.random.default_rng(50 + nc)
    wave = Wave(listed, nc, rng)
    for rows in ([(0, 0)] * nc, [(2, 8), (1, 3)][:nc], [(3, 15), (2, 1)][:nc], [(5, 7), (4, 9)][:nc]):
        got, read = wave.run(rows)
        assert np.array_equal(got[:, : wave.h + 7], wave.hacc(rows)), rows
        ends = [wave.q["a_end"]] + ([wave.p["zero_off"] + (wave.q["quads"] - 1) * 4 * wave.ws + 8] if nc == 2 else [])
        assert read.nonzero()[0].max() + 1 == max(ends) <= len(wave.lds)
    # the lanes of the two candidates of a wave have different taps: a row group never sees the partner's
    if nc == 2:
        a, _ = wave.run([(2, 8), (1, 3)])
        b, _ = wave.run([(2, 8), (0, 12)])
        assert np.array_equal(a[:32], b[:32]) and not np.array_equal(a[32:], b[32:])


@pytest.mark.parametrize("nc", LAYOUTS)
def test_bytes_past_the_window_reach_no_consumed_value(listed, nc):
    """bytes beyond W + 7 of a row, rows beyond H + 6 and whatever lies behind the windows (source block, the rest of
    the work area) are read -- and change nothing the filter consumes"""
    rng = np.random.default_rng(60 + nc)
    wave = Wave(listed, nc, rng)
    rows = [(2, 8), (1, 5)][:nc]
    got, read = wave.run(rows)
    keep = wave.valid_mask()
    assert (read & ~keep).any()                          # such bytes ARE read
    other = Wave(listed, nc, np.random.default_rng(70 + nc))
    other.lds[keep] = wave.lds[keep]
    assert (other.lds[~keep] != wave.lds[~keep]).any()
    got2, _ = other.run(rows)
    n = wave.h + 7
    assert np.array_equal(got[:, :n], got2[:, :n])
    assert not np.array_equal(got[:, n:], got2[:, n:])   # the rows past H + 6 of the last quad do differ: never consumed
    assert 4 * wave.q["quads"] - n in (1, 2, 3)


@pytest.mark.parametrize("nc", LAYOUTS)
def test_accumulator_range_is_the_one_the_pack_relies_on(listed, nc):
    """windows of -128 / 127 chosen by tap sign drive the MFMA's accumulators to [-7106, 23494] over the tap table:
    what PACK4 (tests/test_mc8_pack4.py) states for the v_dot4 form"""
    lo, hi = 1 << 30, -(1 << 30)
    wave = Wave(listed, nc, np.random.default_rng(80 + nc))
    for f in range(6):
        for q in range(16):
            h = HALF[f, q]
            pat = np.resize(np.where(h > 0, 127, -128), wave.ws).astype(np.int8)
            for cand in range(nc):
                win = wave.window(cand)
                win[0::2] = pat                          # even rows to the top of the range, odd rows to the bottom
                win[1::2] = np.where(pat == 127, -128, 127)
            got, _ = wave.run([(f, q)] * nc)
            got = got[:, : wave.h + 7]
            assert np.array_equal(got, wave.hacc([(f, q)] * nc))
            lo, hi = min(lo, int(got.min())), max(hi, int(got.max()))
    assert (lo, hi) == (-7106, 23494)


def test_kernel_text_states_the_form_modelled_here():
    txt = open(os.path.join(CSRC, "cand_common.hpp")).read()
    assert "quad = __builtin_amdgcn_mfma_i32_16x16x32_i8(*(const long *)(ap0 + quad_at * 4 * WS), bb0, cbias, 0, 0, 0);" in txt
    assert "quad = __builtin_amdgcn_mfma_i32_16x16x32_i8(*(const long *)(ap1 + quad_at * 4 * WS), bb1, quad, 0, 0, 0);" in txt
    assert "ap0 = second ? zero : ad;" in txt and "ap1 = second ? ad : zero;" in txt
    assert "return quad[r & 3];" in txt
