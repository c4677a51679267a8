"""The partition decision on the GPU: every trial of tests/golden/part_pick_ref.npz (the reference's own text executed)
through r1_rd_partition_pick_batch with the nodes' states carried on the device, best_rd compared as bits; what the
entry points answer to a bad argument; r1_part_select_batch and r1_part_select_rect_batch against NumPy with guard
bytes around every destination; and one closed loop -- a 16x16 node coded whole and as four 8x8 through the device
chain, the pick, the three selects, nothing read until the end -- against tile_chain_util.host_chain composed with
rdo_glue.partition_pick_bottomup.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import layout_util as LU
import oracle_lib as O
import part_pick_util as U
from rav1e_amd import _lib, rdo_glue
from rav1e_amd.types import COEFF_CDF_CONTEXT, COEFF_NBR_CONTEXT, PART_BOTTOMUP, PART_PICK, PART_TOPDOWN, RD_PICK

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 0x5A


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _records(a):
    """a structured array -> its (n, itemsize) uint8 device tensor"""
    return _t(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize))


def _children(costs, kind):
    """up to four costs per node (None = absent) -> (the children array as R1RdPick (kind 0) or R1PartPick (kind 1)
    records with poisoned other fields, child_idx).  Row 0 is a decoy no index names."""
    dt = RD_PICK if kind == 0 else PART_PICK
    rows, idx = [1.0], []
    for node in costs:
        idx.append([-1] * 4)
        for k, c in enumerate(node):
            if c is not None:
                idx[-1][k] = len(rows)
                rows.append(c)
    a = np.zeros(len(rows), dt)
    a.view(np.uint8)[:] = GUARD
    a["best_rd"] = rows
    return _records(a), _t(np.array(idx, np.int32))


# ---------------------------------------------------------------- the fixture
def test_every_fixture_trial_with_states_carried_on_the_device(ctx):
    import torch
    ref = U.load()
    n_trials, n_nodes = len(ref["t_case"]), len(ref["n_case"])
    # the nodes' states: bottom-up nothing kept; top-down what the caller put there (cached_block.rd_cost)
    st0 = np.zeros(n_nodes, PART_PICK)
    st0["best_rd"], st0["best_partition"], st0["best_call"] = U.F64_MAX, -1, -1
    first = np.nonzero(ref["t_first"])[0]
    st0["best_rd"][ref["t_node"][first]] = ref["t_best_in"][first]
    st0["best_partition"] = ref["n_part_in"]
    st0["reserved"] = GUARD
    state = _records(st0)
    # round r = the r-th trial of every node; inside a round, one call per (rule, partition, lambda, exit, rate arm)
    seen, rounds = {}, {}
    for i in range(n_trials):
        node = int(ref["t_node"][i])
        r = seen.get(node, 0)
        seen[node] = r + 1
        key = (r, int(ref["t_rule"][i]), int(ref["t_partition"][i]), float(ref["t_lam"][i]), int(ref["t_ee"][i]), int(ref["t_rate"][i]) < 0)
        rounds.setdefault(key, []).append(i)
    assert max(seen.values()) == 4
    sizes, launched, kept_behind, n_calls = [1, 63, 65], [], [], 0
    for key in sorted(rounds):
        r, rule, partition, lam, ee, no_rate = key
        todo = rounds[key]
        while todo:
            chunk, todo = todo[:sizes[n_calls % 3]], todo[sizes[n_calls % 3]:]
            idx = _t(ref["t_node"][chunk].astype(np.int64))
            sub = state[idx].contiguous()                              # the carried states of this call's nodes
            kids, child_idx = _children([U.children(ref, i) for i in chunk], n_calls & 1)
            par = np.zeros(len(chunk), PART_PICK)
            par["best_rd"] = ref["t_ref"][chunk]
            ctx.rd_partition_pick_batch(
                sub, partition, r, rule, lam, kids, child_idx, enable_early_exit=bool(ee),
                part_rate=None if no_rate else _t(ref["t_rate"][chunk].astype(np.uint32).view(np.int32)),
                must_split=_t(ref["t_must"][chunk].astype(np.uint8)) if n_calls % 4 != 3 or ref["t_must"][chunk].any() else None,
                parent=_records(par) if rule == PART_BOTTOMUP else None,
                parent_idx=_t(np.arange(len(chunk), dtype=np.int32)) if rule == PART_BOTTOMUP else None)
            state[idx] = sub
            launched.append(chunk)
            kept_behind.append(sub)
            n_calls += 1
    torch.cuda.synchronize()                                            # the first host read
    assert {len(c) for c in launched} >= {1, 63, 65}
    assert any(len({int(ref["t_case"][i]) for i in c}) > 1 for c in launched)
    held = {}
    for chunk, sub in zip(launched, kept_behind):
        got = sub.cpu().numpy().reshape(-1).view(PART_PICK)
        for i, g in zip(chunk, got):
            node = int(ref["t_node"][i])
            r = sum(1 for j in held.get(node, ()))                      # this trial's call_id
            name = (str(ref["c_names"][ref["t_case"][i]]), i)
            assert U.bits(g["best_rd"]) == U.bits(ref["t_best_rd"][i]), name
            assert int(g["best_partition"]) == int(ref["t_best_part"][i]), name
            assert int(g["early_exit"]) == int(ref["t_early"][i]), name
            calls = held.setdefault(node, [])
            want_call = r if ref["t_kept"][i] else (calls[-1] if calls else -1)
            assert int(g["best_call"]) == want_call, name
            calls.append(want_call)
            assert (g["reserved"] == GUARD).all(), name
    assert sum(len(c) for c in launched) == n_trials
    final = state.cpu().numpy().reshape(-1).view(PART_PICK)
    assert np.array_equal(U.bits(final["best_rd"]), U.bits(ref["n_rd"]))
    assert np.array_equal(final["best_partition"].astype(np.int32), ref["n_part"])


# ---------------------------------------------------------------- refusals
def _pick_args(ctx, n=2):
    """a valid argument list of r1_rd_partition_pick_batch by name, with the tensors it points into"""
    st = ctx.part_pick_state(n)
    kids, child_idx = _children([[10.0, 20.0, 30.0, 40.0]] * n, 1)
    rate = _t(np.full(n, 16, np.int32))
    par = ctx.part_pick_state(n)
    pidx = _t(np.arange(n, dtype=np.int32))
    keep = (st, kids, child_idx, rate, par, pidx)
    args = dict(ctx=ctx.h, state=st.data_ptr(), n=n, partition=3, call_id=1, rule=0, lam=8.0, ee=1, part_rate=rate.data_ptr(),
                children=kids.data_ptr(), child_stride=16, n_children_states=kids.shape[0], child_idx=child_idx.data_ptr(),
                must_split=None, parent=par.data_ptr(), n_parent_states=n, parent_idx=pidx.data_ptr(), stream=None)
    return args, keep


PICK_REFUSALS = [("ctx", None), ("state", None), ("child_idx", None), ("n", -1), ("partition", -1), ("partition", 4),
                 ("partition", 10), ("rule", -1), ("rule", 2), ("call_id", -1), ("call_id", 128), ("child_stride", 0),
                 ("child_stride", 4), ("child_stride", 20), ("child_stride", -8), ("lam", -1.0), ("lam", float("inf")),
                 ("lam", float("nan")), ("children", None), ("n_children_states", -1), ("n_parent_states", -1)]


@pytest.mark.parametrize("name,value", PICK_REFUSALS)
def test_pick_refuses(ctx, name, value):
    import torch
    args, keep = _pick_args(ctx)
    before = keep[0].clone()
    assert ctx.lib.r1_rd_partition_pick_batch(*args.values()) == 0
    torch.cuda.synchronize()
    after_good = keep[0].clone()
    assert not torch.equal(before, after_good)
    args[name] = value
    assert ctx.lib.r1_rd_partition_pick_batch(*args.values()) == EINVAL, (name, value)
    assert name.encode() in ctx.lib.r1_last_error() or b"requirement failed" in ctx.lib.r1_last_error()
    torch.cuda.synchronize()
    assert torch.equal(keep[0], after_good)                              # a refused call launches nothing


def test_pick_with_no_nodes_touches_nothing(ctx):
    import torch
    args, keep = _pick_args(ctx)
    before = keep[0].clone()
    args["n"] = 0
    assert ctx.lib.r1_rd_partition_pick_batch(*args.values()) == 0
    torch.cuda.synchronize()
    assert torch.equal(keep[0], before)


def test_out_of_range_indices_are_absent(ctx):
    """a child index at or beyond n_children_states, or negative, loads nothing and counts as absent; a parent index
    outside the parent array means f64::MAX"""
    n = 6
    kids, _ = _children([[10.0, 20.0, 30.0, 40.0]], 0)                    # rows 1..4 behind the decoy
    rows = kids.shape[0]
    idx = np.array([[1, 2, 3, 4], [1, rows, 3, 4], [1, -7, 3, 4], [1, 2 ** 31 - 1, 3, 4], [1, -2 ** 31, 3, 4], [1, 2, 3, 4]], np.int32)
    par = np.zeros(2, PART_PICK)
    par["best_rd"] = 5.0                                                  # a ref_rd_cost every sum exceeds
    pidx = np.array([-1, 2, 2 ** 31 - 1, -2 ** 31, -3, 0], np.int32)
    want = []
    for s in range(n):
        ch = [float(10 * (k + 1)) if 0 <= idx[s, k] < rows else None for k in range(4)]
        ref_rd = 5.0 if 0 <= pidx[s] < 2 else U.F64_MAX
        want.append((rdo_glue.partition_pick_bottomup(U.F64_MAX, 3, 8.0, 16, ch, ref_rd=ref_rd),
                     rdo_glue.partition_pick_topdown(U.F64_MAX, 3, 8.0, 16, ch)))
    for rule in (PART_BOTTOMUP, PART_TOPDOWN):
        st = ctx.part_pick_state(n)
        ctx.rd_partition_pick_batch(st, 3, 5, rule, 8.0, kids, _t(idx), part_rate=_t(np.full(n, 16, np.int32)),
                                    parent=_records(par), parent_idx=_t(pidx))
        got = st.cpu().numpy().reshape(-1).view(PART_PICK)
        for s in range(n):
            kept, rd, early = want[s][rule]
            assert (int(got["best_call"][s]) == 5) == kept and int(got["early_exit"][s]) == int(early), (rule, s)
            assert float(got["best_rd"][s]) == (rd if kept else U.F64_MAX), (rule, s)
    assert [w[0][0] for w in want] == [True, True, True, True, True, False]    # the last one exits on its parent's cost
    assert [w[1][0] for w in want] == [True, False, False, False, False, True]  # top-down refuses an absent child


# ---------------------------------------------------------------- r1_part_select_batch
def _states(calls):
    st = np.zeros(len(calls), PART_PICK)
    st["best_rd"], st["best_partition"], st["best_call"] = 1.0, 3, calls
    return _records(st)


def _guarded_rows(n, row, shift, rng):
    """(the whole buffer, its (n, row) view at 256 + shift bytes, the host copy of the rows)"""
    import torch
    raw = torch.full((512 + shift + n * row,), GUARD, dtype=torch.uint8, device="cuda")
    view = raw[256 + shift:256 + shift + n * row].view(n, row)
    host = rng.integers(0, 256, (n, row), dtype=np.uint8)
    view.copy_(_t(host))
    return raw, view, host


@pytest.mark.parametrize("row,shift", [(COEFF_CDF_CONTEXT.itemsize, 0), (COEFF_NBR_CONTEXT.itemsize, 0), (20, 4), (20, 0),
                                       (COEFF_NBR_CONTEXT.itemsize, 8)])
@pytest.mark.parametrize("n_src", [1, 2, 4])
def test_select_moves_the_winning_trials_rows(ctx, row, shift, n_src):
    assert (row, shift) != (7872, 0) or row % 16 == 0
    rng = np.random.default_rng(row + shift + n_src)
    calls = np.array([-1, 0, 1, 2, 3, 4, 127, -128, 0, 1, 1, 0, 3], np.int8)     # every gate: none, each source, beyond n_src
    n = len(calls)
    raw_d, dst, hdst = _guarded_rows(n, row, shift, rng)
    srcs = [_guarded_rows(n, row, shift, rng) for _ in range(n_src)]
    missing = 1 if n_src == 4 else None                                          # one source of four is absent (NULL)
    ctx.part_select_batch(_states(calls), [None if k == missing else s[1] for k, s in enumerate(srcs)], dst)
    want = hdst.copy()
    for s, c in enumerate(calls):
        if 0 <= c < n_src and c != missing:
            want[s] = srcs[c][2][s]
    got = raw_d.cpu().numpy()
    assert np.array_equal(got[256 + shift:256 + shift + n * row].reshape(n, row), want)
    assert (got[:256 + shift] == GUARD).all() and (got[256 + shift + n * row:] == GUARD).all()
    for raw, _v, host in srcs:                                                    # the sources are only read
        assert np.array_equal(raw.cpu().numpy()[256 + shift:256 + shift + n * row].reshape(n, row), host)


def test_select_with_the_live_state_as_a_source(ctx):
    """srcs[c] == dst: the trial that ran last left the live state standing -- nothing is copied for its nodes, the
    others' rows come from the snapshot"""
    rng = np.random.default_rng(3)
    calls = np.array([1, 0, 1, -1, 0, 2], np.int8)
    n, row = len(calls), COEFF_NBR_CONTEXT.itemsize
    raw_d, dst, hdst = _guarded_rows(n, row, 0, rng)
    _raw_s, snap, hsnap = _guarded_rows(n, row, 0, rng)
    ctx.part_select_batch(_states(calls), [snap, dst], dst)
    want = hdst.copy()
    want[calls == 0] = hsnap[calls == 0]
    got = raw_d.cpu().numpy()
    assert np.array_equal(got[256:256 + n * row].reshape(n, row), want)
    assert (got[:256] == GUARD).all() and (got[256 + n * row:] == GUARD).all()


def test_select_strided_rows_leave_the_gaps(ctx):
    """rows inside wider records (the winner arrays of the commit with a larger stride): the bytes between rows stay"""
    import torch
    rng = np.random.default_rng(4)
    calls = np.array([0, 1, 0, 1, -1], np.int8)
    n = len(calls)
    big_d = torch.full((n, 48), GUARD, dtype=torch.uint8, device="cuda")
    big_s = [_t(rng.integers(0, 256, (n, 64), dtype=np.uint8)) for _ in range(2)]
    ctx.part_select_batch(_states(calls), [b[:, :32] for b in big_s], big_d[:, :32])
    got = big_d.cpu().numpy()
    for s, c in enumerate(calls):
        assert np.array_equal(got[s, :32], big_s[c].cpu().numpy()[s, :32] if c >= 0 else np.full(32, GUARD, np.uint8))
    assert (got[:, 32:] == GUARD).all()


def _select_args(ctx):
    import torch
    st = _states(np.array([0, 1], np.int8))
    a, b, d = (torch.zeros((2, 32), dtype=torch.uint8, device="cuda") for _ in range(3))
    ptrs = (C.c_void_p * 4)(a.data_ptr(), b.data_ptr(), None, None)
    return dict(ctx=ctx.h, state=st.data_ptr(), n=2, n_src=2, srcs=ptrs, src_stride=32, dst=d.data_ptr(), dst_stride=32,
                bytes=32, stream=None), (st, a, b, d, ptrs)


@pytest.mark.parametrize("name,value", [("ctx", None), ("state", None), ("srcs", None), ("dst", None), ("n", -1), ("n_src", 0),
                                        ("n_src", 5), ("bytes", -4), ("bytes", 30), ("src_stride", 30), ("dst_stride", 34),
                                        ("src_stride", -32), ("dst_stride", 28), ("dst", "+2"), ("srcs", "+2"), ("srcs", "=dst")])
def test_select_refuses(ctx, name, value):
    args, keep = _select_args(ctx)
    assert ctx.lib.r1_part_select_batch(*args.values()) == 0
    if value == "+2":
        if name == "dst":
            args["dst"] += 2
        else:
            args["srcs"] = (C.c_void_p * 4)(keep[1].data_ptr(), keep[2].data_ptr() + 2, None, None)
    elif value == "=dst":                                                         # the live state with another stride
        args["srcs"] = (C.c_void_p * 4)(keep[1].data_ptr(), keep[3].data_ptr(), None, None)
        args["src_stride"] = 64
    else:
        args[name] = value
    assert ctx.lib.r1_part_select_batch(*args.values()) == EINVAL, (name, value)


# ---------------------------------------------------------------- r1_part_select_rect_batch
def _planes(bd, w, h, kind, n, base_off=None):
    """n + 1 guarded device planes of one geometry with different noise everywhere (padding included): the destination
    first.  base_off: the element offset of the SOURCES' data in their buffers (another one than the destination's
    makes them incongruent with it modulo 16)"""
    out = []
    for k in range(n + 1):
        hp = O.HostPlane(w, h, bd, 16, 16, rng=np.random.default_rng(bd * 100 + w + 7 * k))
        if kind is None:
            p = hp
            off = 0
        else:
            p = LU.host_relayout(hp, kind, 8, 8)
            off = 1 if kind == "odd" else 0
        if k and base_off is not None:
            off = base_off
        out.append((p, LU.DevicePlane(p, off)))
    return out


RECTS = [
    # bw, bh, positions (x = 4 mod 16 among them; crossing store_w / store_h; negative)
    (4, 4, [(4, 0), (20, 4), (36, 8), (60, 44), (0, 12), (8, 12)]),
    (8, 8, [(4, 8), (20, 40), (56, 16), (60, 44), (-4, 0), (32, -4)]),
    (16, 8, [(4, 0), (20, 8), (52, 16), (36, 44), (0, 24), (16, 24)]),
    (64, 64, [(4, 0)]),
    (64, 64, [(0, 0)]),
    (32, 16, [(36, 4), (0, 40), (-16, 20)]),
]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind,base_off", [(None, None), ("odd", None), ("tight", None), ("tight", 3)])
@pytest.mark.parametrize("case", range(len(RECTS)))
def test_select_rect_moves_the_winning_trials_rectangle(ctx, bd, kind, base_off, case):
    bw, bh, pos = RECTS[case]
    w, h = 62, 46                       # the visible plane: rectangles cross its right and bottom edges
    planes = _planes(bd, w, h, kind, 3, base_off)
    (hdst, ddst), srcs = planes[0], planes[1:]
    n = len(pos)
    calls = np.array([(s % 3) for s in range(n)], np.int8)
    if n > 3:
        calls[3] = -1
        calls[-1] = 3                   # beyond n_src
    store = (w, h) if case % 2 == 0 else (w + 6, h + 5)          # the padding to the right and below, as the commit admits
    ctx.part_select_rect_batch(_states(calls), [d for _h, d in srcs], ddst, _t(np.array(pos, np.int16)), bw, bh, *store)
    want = hdst.data.copy()
    for s, (x, y) in enumerate(pos):
        c = int(calls[s])
        if not 0 <= c < 3:
            continue
        x0, x1, y0, y1 = max(x, 0), min(x + bw, store[0]), max(y, 0), min(y + bh, store[1])
        if x0 < x1 and y0 < y1:
            src = srcs[c][0]
            want[hdst.yorigin + y0:hdst.yorigin + y1, hdst.xorigin + x0:hdst.xorigin + x1] = \
                src.data[src.yorigin + y0:src.yorigin + y1, src.xorigin + x0:src.xorigin + x1]
    assert np.array_equal(ddst.host(), want)                      # the rectangles, and everything else byte-identical
    assert LU.guards_intact(ddst, *[d for _h, d in srcs])
    for hs, ds in srcs:
        assert np.array_equal(ds.host(), hs.data)


def test_select_rect_gates_and_the_live_plane_as_a_source(ctx):
    planes = _planes(8, 32, 32, "tight", 1)
    (hdst, ddst), (hsrc, dsrc) = planes
    pos = _t(np.array([[0, 0], [16, 0], [0, 16], [16, 16]], np.int16))
    ctx.part_select_rect_batch(_states(np.array([0, 1, 2, 0], np.int8)), [dsrc, ddst, None], ddst, pos, 16, 16)
    want = hdst.data.copy()
    for x, y in ((0, 0), (16, 16)):
        want[hdst.yorigin + y:hdst.yorigin + y + 16, hdst.xorigin + x:hdst.xorigin + x + 16] = \
            hsrc.data[hsrc.yorigin + y:hsrc.yorigin + y + 16, hsrc.xorigin + x:hsrc.xorigin + x + 16]
    assert np.array_equal(ddst.host(), want) and LU.guards_intact(ddst, dsrc)


def _rect_args(ctx):
    planes = _planes(8, 32, 32, "tight", 2)
    st = _states(np.array([0, 1], np.int8))
    pos = _t(np.array([[0, 0], [16, 0]], np.int16))
    sp = (_lib.R1Plane * 4)(planes[1][1].cstruct(), planes[2][1].cstruct(), _lib.R1Plane(), _lib.R1Plane())
    dp = planes[0][1].cstruct()
    return dict(ctx=ctx.h, state=st.data_ptr(), n=2, n_src=2, src_planes=sp, dst_plane=C.pointer(dp), pos_xy=pos.data_ptr(),
                bw=16, bh=16, store_w=32, store_h=32, stream=None), (planes, st, pos, sp, dp)


def _plane_with(p, **kw):
    q = _lib.R1Plane.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


@pytest.mark.parametrize("name,value", [("ctx", None), ("state", None), ("src_planes", None), ("dst_plane", None), ("pos_xy", None),
                                        ("n", -1), ("n_src", 0), ("n_src", 5), ("bw", 12), ("bw", 128), ("bh", 2),
                                        ("store_w", -1), ("store_h", -1), ("store_w", 41), ("store_h", 41),
                                        ("dst", dict(bit_depth=9)), ("dst", dict(bytes_per_px=2)), ("dst", dict(bytes_per_px=4)),
                                        ("dst", dict(data=None)), ("dst", dict(stride=0)),
                                        ("src", dict(stride=64)), ("src", dict(xorigin=4)), ("src", dict(yorigin=4)),
                                        ("src", dict(alloc_height=50)), ("src", dict(bit_depth=10, bytes_per_px=2))])
def test_select_rect_refuses(ctx, name, value):
    args, keep = _rect_args(ctx)
    assert ctx.lib.r1_part_select_rect_batch(*args.values()) == 0
    if name == "dst":
        q = _plane_with(keep[4], **value)
        args["dst_plane"] = C.pointer(q)
    elif name == "src":
        q = _plane_with(keep[3][1], **value)
        args["src_planes"] = (_lib.R1Plane * 4)(keep[3][0], q, _lib.R1Plane(), _lib.R1Plane())
    else:
        args[name] = value
    assert ctx.lib.r1_part_select_rect_batch(*args.values()) == EINVAL, (name, value)


# ---------------------------------------------------------------- the closed loop
@pytest.fixture(scope="module")
def node_host(oracle):
    import tile_chain_util as TC
    whole, split = U.node_cases()
    return whole, split, TC.host_chain(whole, oracle), TC.host_chain(split, oracle)


# (rate of PARTITION_NONE, rate of PARTITION_SPLIT) in 1/8 bit: the second pays the whole block 4096 / 8 bits more
NODE_RATES = [(8, 8), (4096, 8)]


def test_the_two_rates_let_each_side_win_once(node_host):
    whole, split, hw, hs = node_host
    winners = []
    for r_none, r_split in NODE_RATES:
        _k, best, _e = rdo_glue.partition_pick_bottomup(U.F64_MAX, 0, whole.lam, r_none, [float(hw["best_rd"].view(np.float64)[0])])
        kept, _rd, _e = rdo_glue.partition_pick_bottomup(best, 3, whole.lam, r_split, [float(v) for v in hs["best_rd"].view(np.float64)])
        winners.append(3 if kept else 0)
    assert winners == [0, 3]


@pytest.mark.parametrize("rates", NODE_RATES)
def test_node_coded_whole_and_split_then_picked_and_selected(ctx, node_host, rates):
    """PARTITION_NONE's chain on a clone of the tile state, PARTITION_SPLIT's four blocks on the live state (it runs
    last), the two picks, the three selects with srcs = [the clone, the live state]: one stream, nothing read until the
    end.  The live plane rectangle, CDF context and neighbour context are those of the side the host composition picks."""
    import torch
    import coeff_cdf_model as DM
    import tile_chain_util as TC
    from test_gpu_coeff_cdf import _dev_contexts
    from test_gpu_coeff_nbr import NBR_BYTES, _dev_nbr, _shifted_intact
    from coeff_rate_gpu_util import _guards_intact
    whole, split, hw, hs = node_host
    r_none, r_split = rates
    lam = whole.lam

    def tile_state(c):
        org, rec = c.planes()
        _ho, dorg = LU.relayout(org, "tight", 8, 8)
        hrec, drec = LU.relayout(rec, "tight", 8, 8)
        raw_c, dcdf, _ = _dev_contexts([DM.context_from_packed(c.cdf0)])
        raw_n, dnbr, _ = _dev_nbr(np.zeros(1, COEFF_NBR_CONTEXT))
        return dorg, hrec, drec, raw_c, dcdf, raw_n, dnbr
    clone, live = tile_state(whole), tile_state(split)
    ch_w = TC.DeviceChain(ctx, [whole], clone[0], clone[2], clone[4], clone[6])
    ch_s = TC.DeviceChain(ctx, [split], live[0], live[2], live[4], live[6])
    ch_w.step(0)
    for bi in range(4):
        ch_s.step(bi)
    # the children: the blocks' R1RdPick states as the chains left them, gathered on the device
    kids = torch.cat([ch_w.steps[0]["blk"]] + [t["blk"] for t in ch_s.steps]).contiguous()
    node = ctx.part_pick_state(1)
    ctx.rd_partition_pick_batch(node, 0, 0, PART_BOTTOMUP, lam, kids, _t(np.array([[0, -1, -1, -1]], np.int32)),
                                part_rate=_t(np.array([r_none], np.int32)))
    ctx.rd_partition_pick_batch(node, 3, 1, PART_BOTTOMUP, lam, kids, _t(np.array([[1, 2, 3, 4]], np.int32)),
                                part_rate=_t(np.array([r_split], np.int32)))
    ctx.part_select_batch(node, [clone[4], live[4]], live[4])
    ctx.part_select_batch(node, [clone[6], live[6]], live[6])
    ctx.part_select_rect_batch(node, [clone[2], live[2]], live[2], _t(np.array([[0, 0]], np.int16)), 16, 16)
    torch.cuda.synchronize()                                            # the first host read
    # the host composition
    c_whole = float(hw["best_rd"].view(np.float64)[0])
    c_split = [float(v) for v in hs["best_rd"].view(np.float64)]
    _k, best, _e = rdo_glue.partition_pick_bottomup(U.F64_MAX, 0, lam, r_none, [c_whole])
    kept, rd, early = rdo_glue.partition_pick_bottomup(best, 3, lam, r_split, c_split)
    got = node.cpu().numpy().reshape(-1).view(PART_PICK)[0]
    assert U.bits(got["best_rd"]) == U.bits(rd if kept else best)
    assert (int(got["best_partition"]), int(got["best_call"]), int(got["early_exit"])) == ((3, 1, 0) if kept else (0, 0, int(early)))
    # the children the device chains produced are the host chain's
    assert np.array_equal(U.bits(np.array(kids.cpu().numpy().reshape(-1).view(RD_PICK)["best_rd"])),
                          np.r_[hw["best_rd"], hs["best_rd"]].astype(np.uint64))
    win = hs if kept else hw
    hrec, drec = live[1], live[2]
    want = hrec.data.copy()
    want[hrec.yorigin:hrec.yorigin + 16, hrec.xorigin:hrec.xorigin + 16] = win["final"]
    assert np.array_equal(drec.host(), want)
    assert not np.array_equal(hw["final"], hs["final"])
    cdf = live[4].cpu().numpy().reshape(-1).view(COEFF_CDF_CONTEXT)[0]
    assert np.array_equal(DM.packed_of(cdf), win["cdf"][-1])
    nbr = live[6].cpu().numpy().reshape(-1).view(COEFF_NBR_CONTEXT)[0]
    assert np.array_equal(nbr["above"], win["above"][-1]) and np.array_equal(nbr["left"], win["left"][-1])
    assert not np.array_equal(hw["cdf"][-1], hs["cdf"][-1])
    # the clone is only read; nothing outside planes and contexts is touched
    assert np.array_equal(DM.packed_of(clone[4].cpu().numpy().reshape(-1).view(COEFF_CDF_CONTEXT)[0]), hw["cdf"][-1])
    assert LU.guards_intact(clone[2], live[2]) and _guards_intact(live[3]) and _guards_intact(clone[3])
    assert _shifted_intact(live[5], (1, NBR_BYTES)) and _shifted_intact(clone[5], (1, NBR_BYTES))
