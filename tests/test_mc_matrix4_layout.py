"""The horizontal 8-tap pass of the 8-bit fused candidate kernels on sixteen 4x4x4 matrix blocks (mc8_column_t<.., MX4>,
rav1e_amd/csrc/cand_common.hpp; geometry r1mc::mx4_*, mc_window.hpp; rdo_mc_matrix4, rdo_cand_plan.hpp), on the host.
A host program (tests/c/mc_matrix4_list.cpp, the host compiler alone) prints the fragment geometry, the three tap dwords
of every row of the packed tap table at every byte phase, and the plan's choices; here a NumPy restatement of
v_mfma_i32_4x4x4_16b_i8 -- block b is lanes 4 b .. 4 b + 3, lane 4 b + i supplies A[i][0 .. 3], lane 4 b + j supplies
B[0 .. 3][j] and receives D[0 .. 3][j] in registers 0 .. 3, int32 accumulation -- runs the kernel's quads (three chained
products each) over a model of a wave's LDS and must hand every lane the accumulators hacc of its own column:

    hacc(row) = 8192 + 2 + 32 + sum_t h[t] * q[row][column + t],      h = taps / 2, q = pixel - 128 as staged.

Both layouts are modelled, whether their size ships or not: four candidates per wave (16x16) and eight (8x8), every
candidate with taps of its own."""
import os
import subprocess

import numpy as np
import pytest

from test_mc_matrix_layout import BIAS, HALF, le_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rav1e_amd", "csrc")
WIDTHS = (16, 8)
SHIPPED = {(8, 4), (8, 3)}      # (bit depth, log2 size) at which rdo_mc_matrix4 is on


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mc_matrix4") / "mc_matrix4_list")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-variable", "-I" + CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "c", "mc_matrix4_list.cpp")])
    out = {"P": {}, "Q": {}, "A": {}, "T": {}, "B": {}}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        v = [int(x) for x in v]
        if k == "P":
            out["P"][v[0], v[1]] = dict(zip(("mx4", "mx_nc", "nc", "ws", "win", "src_off", "src", "a_end", "lds"), v[2:]))
        elif k == "Q":
            out["Q"][v[0]] = dict(zip(("nc", "ws", "quads", "a_end"), v[1:]))
        elif k == "A":
            out["A"][v[0], v[1], v[2], v[3]] = (v[4], v[5])
        elif k == "T":
            out["T"][v[0], v[1]] = (v[2], v[3])
        else:
            out["B"][v[0], v[1], v[2]] = tuple(v[3:])
    assert len(out["B"]) == 6 * 16 * 4 and len(out["P"]) == 12
    return out


def mfma4(a, b, c):
    """v_mfma_i32_4x4x4_16b_i8 on per-lane operands: a, b (64, 4) int8 values, c (64, 4) int32 -> d (64, 4)"""
    A = np.asarray(a, np.int64).reshape(16, 4, 4)                  # [block, i, K]
    B = np.asarray(b, np.int64).reshape(16, 4, 4)                  # [block, j, K]
    Cm = np.asarray(c, np.int64).reshape(16, 4, 4).transpose(0, 2, 1)   # lane j, register i -> [block, i, j]
    D = np.einsum("bik,bjk->bij", A, B) + Cm
    assert np.abs(D).max() < (1 << 31)
    return D.transpose(0, 2, 1).reshape(64, 4)


def test_mfma4_restatement_is_sixteen_independent_blocks():
    rng = np.random.default_rng(1)
    a, b = rng.integers(-128, 128, (64, 4)), rng.integers(-128, 128, (64, 4))
    c = rng.integers(-9999, 9999, (64, 4))
    d = mfma4(a, b, c)
    for blk in range(16):
        for i in range(4):
            for j in range(4):
                assert d[4 * blk + j, i] == c[4 * blk + j, i] + sum(a[4 * blk + i, k] * b[4 * blk + j, k] for k in range(4))


def test_plan_turns_the_pass_on_exactly_where_it_ships(listed):
    assert {k for k, p in listed["P"].items() if p["mx4"]} == SHIPPED
    assert {k: p["mx_nc"] for k, p in listed["P"].items() if p["mx_nc"]} == {(8, 6): 1, (8, 5): 2}     # r22's, unchanged
    for w in WIDTHS:                                       # the layout's bound is stated whether the size ships or not
        p, q = listed["P"][8, {16: 4, 8: 3}[w]], listed["Q"][w]
        assert (p["nc"], p["ws"]) == (q["nc"], q["ws"]) == (64 // w, w + 8)
        assert p["a_end"] == q["a_end"] <= p["lds"]
        assert p["win"] == q["nc"] * (w + 7) * q["ws"] and p["src_off"] >= p["win"]
        # the last candidate's row past H + 6 lies in the staged source block
        assert p["win"] < q["a_end"] <= p["src_off"] + p["src"]
    assert (listed["Q"][8]["a_end"], listed["Q"][16]["a_end"]) == (1936, 2232)
    for k, p in listed["P"].items():                       # no other size states a bound
        assert (p["a_end"] != 0) == (k in ((8, 4), (8, 3)))


def test_tap_dwords_are_the_half_taps_moved_up_by_the_byte_phase(listed):
    """byte K of dword s at phase j is B_s[K][j] = h[4 s + K - j] for 0 <= 4 s + K - j < 8, else 0: every filter set,
    every fraction, every phase"""
    for f in range(6):
        for q in range(16):
            h = HALF[f, q]
            fx0, fx1 = listed["T"][f, q]
            assert np.array_equal(np.concatenate([le_bytes(fx0, 4), le_bytes(fx1, 4)]), h)   # what the kernels load
            for j in range(4):
                got = np.concatenate([le_bytes(t, 4) for t in listed["B"][f, q, j]])
                for m in range(12):
                    assert got[m] == (h[m - j] if 0 <= m - j < 8 else 0), (f, q, j, m)


def test_fragment_addresses(listed):
    for w in WIDTHS:
        q = listed["Q"][w]
        for c in range(w):
            for quad in range(q["quads"]):
                for s in range(3):
                    row, off = listed["A"][w, c, quad, s]
                    assert row == 4 * quad + c % 4 and off == row * q["ws"] + (c & ~3) + 4 * s
                    assert off % 4 == 0 and off % q["ws"] + 4 <= q["ws"]         # an aligned dword inside its row


class Wave:
    """the LDS of one wave of 64 / w candidates w wide, and the kernel's quads over it"""

    def __init__(self, listed, w, rng):
        self.w = self.h = w
        self.q = listed["Q"][w]
        self.nc, self.ws = self.q["nc"], self.q["ws"]
        self.p = listed["P"][8, {16: 4, 8: 3}[w]]
        self.lds = rng.integers(-128, 128, self.p["lds"]).astype(np.int8)      # whatever lies there
        self.listed = listed

    def window(self, cand):
        """view of candidate cand's staged window, (h + 7) x ws"""
        o = cand * (self.h + 7) * self.ws
        return self.lds[o: o + (self.h + 7) * self.ws].reshape(self.h + 7, self.ws)

    def valid_mask(self):
        """bytes the result may depend on: the windows' (h + 7) x (w + 7) pixels"""
        m = np.zeros(len(self.lds), bool)
        for cand in range(self.nc):
            o = cand * (self.h + 7) * self.ws
            m[o: o + (self.h + 7) * self.ws].reshape(self.h + 7, self.ws)[:, : self.w + 7] = True
        return m

    def run(self, rows):
        """rows: (filter set, fraction) per candidate -> hacc as the lanes receive it, (64, 4 * quads), and the set of
        LDS bytes read"""
        read = np.zeros(len(self.lds), bool)
        cand, c = np.arange(64) // self.w, np.arange(64) % self.w
        out = []
        for quad in range(self.q["quads"]):
            d = np.full((64, 4), BIAS, np.int64)
            for s in range(3):                            # three chained MFMAs: C = the bias, then D
                a = np.zeros((64, 4), np.int64)
                b = np.zeros((64, 4), np.int64)
                for l in range(64):
                    lo = cand[l] * (self.h + 7) * self.ws + self.listed["A"][self.w, c[l], quad, s][1]
                    assert lo % 4 == 0 and lo + 4 <= len(self.lds)
                    a[l] = self.lds[lo: lo + 4]
                    read[lo: lo + 4] = True
                    b[l] = le_bytes(self.listed["B"][rows[cand[l]][0], rows[cand[l]][1], c[l] % 4][s], 4)
                d = mfma4(a, b, d)
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


def tap_rows(nc, f, q):
    """(filter set, fraction) per candidate: candidate 0 has (f, q), all nc differ in the fraction, neighbours in both"""
    return [((f + k) % 6, (q + 5 * k) % 16) for k in range(nc)]


@pytest.mark.parametrize("w", WIDTHS)
def test_every_lane_receives_hacc_of_its_own_column(listed, w):
    wave = Wave(listed, w, np.random.default_rng(50 + w))
    for f in range(6):
        for q in range(16):
            rows = tap_rows(wave.nc, f, q)
            assert len({r[1] for r in rows}) == wave.nc and all(a[0] != b[0] for a, b in zip(rows, rows[1:]))
            got, read = wave.run(rows)
            assert np.array_equal(got[:, : wave.h + 7], wave.hacc(rows)), rows
            assert read.nonzero()[0].max() + 1 == wave.q["a_end"] <= len(wave.lds)
    # a block never sees another candidate's taps: change one candidate's, only its lanes change
    a, _ = wave.run(tap_rows(wave.nc, 2, 8))
    other = tap_rows(wave.nc, 2, 8)
    other[1] = (5, 1)
    b, _ = wave.run(other)
    mine = np.arange(64) // w == 1
    assert np.array_equal(a[~mine], b[~mine]) and not np.array_equal(a[mine], b[mine])


@pytest.mark.parametrize("w", WIDTHS)
def test_bytes_past_the_window_reach_no_consumed_value(listed, w):
    """the byte beyond W + 7 of a row, the row beyond H + 6 (the next candidate's window; the staged source block for the
    last one) are read -- and change nothing the filter consumes"""
    wave = Wave(listed, w, np.random.default_rng(60 + w))
    rows = tap_rows(wave.nc, 2, 8)
    got, read = wave.run(rows)
    keep = wave.valid_mask()
    assert (read & ~keep).any()                          # such bytes ARE read
    assert read[wave.p["win"]:].any()                    # behind the last window too
    other = Wave(listed, w, np.random.default_rng(70 + w))
    other.lds[keep] = wave.lds[keep]
    assert (other.lds[~keep] != wave.lds[~keep]).any()
    got2, _ = other.run(rows)
    n = wave.h + 7
    assert np.array_equal(got[:, :n], got2[:, :n])
    assert not np.array_equal(got[:, n:], got2[:, n:])   # the row past H + 6 of the last quad does differ: never consumed
    assert 4 * wave.q["quads"] - n == 1


@pytest.mark.parametrize("w", WIDTHS)
def test_accumulator_range_is_the_one_the_pack_relies_on(listed, w):
    """windows of -128 / 127 chosen by tap sign drive the accumulators to [-7106, 23494] over the tap table: what PACK4
    (tests/test_mc8_pack4.py) states for the v_dot4 form"""
    lo, hi = 1 << 30, -(1 << 30)
    wave = Wave(listed, w, np.random.default_rng(80 + w))
    for f in range(6):
        for q in range(16):
            h = HALF[f, q]
            pat = np.resize(np.where(h > 0, 127, -128), wave.ws).astype(np.int8)
            for cand in range(wave.nc):
                win = wave.window(cand)
                win[0::2] = pat                          # even rows to the top of the range, odd rows to the bottom
                win[1::2] = np.where(pat == 127, -128, 127)
            got, _ = wave.run([(f, q)] * wave.nc)
            got = got[:, : wave.h + 7]
            assert np.array_equal(got, wave.hacc([(f, q)] * wave.nc))
            lo, hi = min(lo, int(got.min())), max(hi, int(got.max()))
    assert (lo, hi) == (-7106, 23494)


def test_kernel_text_states_the_form_modelled_here():
    txt = open(os.path.join(CSRC, "cand_common.hpp")).read()
    assert "const uint32_t *wrow = (const uint32_t *)win + (c >> 2);" in txt
    assert "const uint32_t *arow = wrow + (c & 3) * WSD;" in txt
    assert "const uint32_t *ar = arow + quad_at * 4 * WSD;" in txt
    assert "quad = __builtin_amdgcn_mfma_i32_4x4x4i8((int)ar[0], (int)t0, cbias, 0, 0, 0);" in txt
    assert "quad = __builtin_amdgcn_mfma_i32_4x4x4i8((int)ar[1], (int)t1, quad, 0, 0, 0);" in txt
    assert "quad = __builtin_amdgcn_mfma_i32_4x4x4i8((int)ar[2], (int)t2, quad, 0, 0, 0);" in txt
    # t0 .. t2 are r1mc::mx4_band's expressions
    assert "const uint64_t t64 = (((uint64_t)fx1 << 32) | fx0) << sh8;" in txt
    assert "const uint32_t t0 = (uint32_t)t64, t1 = (uint32_t)(t64 >> 32);" in txt
    assert "const uint32_t t2 = (uint32_t)(((uint64_t)fx1 << sh8) >> 32);" in txt
