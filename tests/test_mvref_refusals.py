"""What the four entry points of the MV-stack unit answer to a bad argument (the harness of tests/test_entry_refusals.py:
a zeroed stand-in context, host memory, nothing touches a device): every R1_EINVAL the header lists, and the empty batch,
which passes every check, returns 0 and touches nothing.  The device-resident refusals are in tests/test_gpu_mvref.py."""
import ctypes as C

import numpy as np
import pytest

from rav1e_amd.types import MV_STACK, TILE_BLOCKS
from test_entry_refusals import Harness


@pytest.fixture(scope="module")
def harness():
    return Harness()


def descs(harness, n=1, **over):
    d = np.zeros(n, TILE_BLOCKS)
    for k in range(n):
        d[k] = (C.addressof(harness.mem[0]), 32, 22, 10, 0, 0, 22, 10, 0)
        for f, v in over.items():
            d[k][f] = v
    return d


BAD_DESCS = [dict(cells=0), dict(cells=8), dict(cols=0), dict(rows=0), dict(stride=21), dict(cols=1025, stride=1025, frame_cols=1025),
             dict(stride=1025), dict(rows=65536, frame_rows=65536), dict(tile_x=-1), dict(tile_y=-1), dict(frame_cols=21),
             dict(frame_rows=9), dict(tile_x=4), dict(tile_y=1)]
GOOD_DESCS = [dict(), dict(stride=22), dict(cols=1024, stride=1024, frame_cols=1024), dict(tile_x=4, frame_cols=26),
              dict(tile_y=6, frame_rows=16), dict(rows=65535, frame_rows=65535)]


def calls(harness, d, n_tiles=None):
    """the four calls on an empty batch with descriptors d -> their statuses (pmv takes no descriptors)"""
    L, ctx, buf = harness.L, C.addressof(harness.fake_ctx), C.addressof(harness.mem[2])
    p = d.ctypes.data if d is not None else None
    n_tiles = len(d) if n_tiles is None else n_tiles
    return (L.r1_tile_blocks_reset_batch(ctx, p, n_tiles, buf, 0, None),
            L.r1_tile_blocks_store_batch(ctx, p, n_tiles, buf, 1, buf, 1, None, 0, 0, 1, 1, None),
            L.r1_mvref_stack_batch(ctx, p, n_tiles, buf, 0, buf, 1, 4, buf, buf, None))


@pytest.mark.parametrize("over", BAD_DESCS, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_bad_descriptor(harness, over):
    before = [bytes(m) for m in harness.mem]
    assert calls(harness, descs(harness, **over)) == (-1, -1, -1)
    assert calls(harness, np.concatenate([descs(harness), descs(harness, **over)])) == (-1, -1, -1)       # any of them
    assert [bytes(m) for m in harness.mem] == before


@pytest.mark.parametrize("over", GOOD_DESCS, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()) or "base")
def test_good_descriptor_and_empty_batch(harness, over):
    before = [bytes(m) for m in harness.mem]
    assert calls(harness, descs(harness, **over)) == (0, 0, 0)
    assert [bytes(m) for m in harness.mem] == before


def test_descriptor_count(harness):
    assert calls(harness, None, 1) == (-1, -1, -1)
    assert calls(harness, descs(harness), 0) == (-1, -1, -1)
    assert calls(harness, descs(harness, 64)) == (0, 0, 0)
    assert calls(harness, descs(harness, 65)) == (-1, -1, -1)


def test_arguments(harness):
    L, ctx, buf = harness.L, C.addressof(harness.fake_ctx), C.addressof(harness.mem[2])
    d = descs(harness, 2)
    p = d.ctypes.data
    before = [bytes(m) for m in harness.mem]
    sel = (C.c_int32 * 2)(0, 1)
    reset = lambda **o: L.r1_tile_blocks_reset_batch(*[{**dict(ctx=ctx, tiles=p, n_tiles=2, sel=C.addressof(sel), n=0, stream=None), **o}[k]
                                                        for k in ("ctx", "tiles", "n_tiles", "sel", "n", "stream")])
    assert reset() == 0 and reset(ctx=None) == -1 and reset(n=-1) == -1 and reset(n=65) == -1
    assert reset(sel=None, n=1) == -1                      # without sel every descriptor: n == n_tiles
    bad = (C.c_int32 * 2)(0, 2)
    assert reset(sel=C.addressof(bad), n=2) == -1 and reset(sel=C.addressof((C.c_int32 * 1)(-1)), n=1) == -1
    store = lambda **o: L.r1_tile_blocks_store_batch(*[{**dict(ctx=ctx, tiles=p, n_tiles=2, blocks=buf, n_blocks=1, trials=buf, n_trials=1,
                                                               state=buf, n=0, call_id=0, group=1, nt=1, stream=None), **o}[k]
                                                        for k in ("ctx", "tiles", "n_tiles", "blocks", "n_blocks", "trials", "n_trials",
                                                                  "state", "n", "call_id", "group", "nt", "stream")])
    assert store() == 0 and store(state=None) == 0 and store(call_id=127, group=4096, nt=16) == 0
    for o in (dict(ctx=None), dict(blocks=None), dict(trials=None), dict(n=-1), dict(n_blocks=0), dict(n_trials=0), dict(call_id=-1),
              dict(call_id=128), dict(group=0), dict(group=4097), dict(nt=0), dict(nt=17), dict(state=None, n=2)):
        assert store(**o) == -1, o
    stack = lambda **o: L.r1_mvref_stack_batch(*[{**dict(ctx=ctx, tiles=p, n_tiles=2, blocks=buf, n_blocks=0, queries=buf, n_queries=1,
                                                         max_queries=8, sign_bias=buf, out=buf, stream=None), **o}[k]
                                                  for k in ("ctx", "tiles", "n_tiles", "blocks", "n_blocks", "queries", "n_queries",
                                                            "max_queries", "sign_bias", "out", "stream")])
    assert stack() == 0 and stack(max_queries=1) == 0 and stack(max_queries=64) == 0
    for o in (dict(ctx=None), dict(blocks=None), dict(queries=None), dict(sign_bias=None), dict(out=None), dict(out=buf + 2),
              dict(n_blocks=-1), dict(n_queries=0), dict(max_queries=0), dict(max_queries=65)):      # more than 64 queries a block
        assert stack(**o) == -1, o
    pmv = lambda **o: L.r1_mvref_pmv_batch(*[{**dict(ctx=ctx, stacks=buf, n=0, pmv_out=buf + 8, stride=16, stream=None), **o}[k]
                                             for k in ("ctx", "stacks", "n", "pmv_out", "stride", "stream")])
    assert pmv() == 0 and pmv(stride=8) == 0 and pmv(stride=MV_STACK.itemsize) == 0
    for o in (dict(ctx=None), dict(stacks=None), dict(pmv_out=None), dict(n=-1), dict(stride=6), dict(stride=17), dict(stride=0),
              dict(pmv_out=buf + 1)):
        assert pmv(**o) == -1, o
    assert [bytes(m) for m in harness.mem] == before


def test_abi_and_symbols():
    from rav1e_amd import _lib
    assert _lib.load().r1_abi_version() == 7
    assert {"r1_tile_blocks_reset_batch", "r1_tile_blocks_store_batch", "r1_mvref_stack_batch", "r1_mvref_pmv_batch"} <= set(_lib.SYMBOLS)


def test_api_refuses_a_block_with_more_than_64_queries():
    """the wrapper sees the host arrays: the refusal comes before anything is enqueued (no device is touched)"""
    from rav1e_amd import api
    from rav1e_amd.types import MV_BLOCK, MV_QUERY
    blocks = np.zeros(1, MV_BLOCK)
    blocks["n_queries"] = 65

    class NoDevice:
        _tile_descs = staticmethod(lambda tiles: np.zeros(1, TILE_BLOCKS))
    with pytest.raises(ValueError):
        api.Context.mvref_stack_batch(NoDevice(), [None], blocks, np.zeros(65, MV_QUERY), [0] * 8)
