"""What the four head-symbol entry points answer to a bad argument, as a table in the manner of
tests/test_coeff_nbr_refusals.py (the harness of tests/test_entry_refusals.py: a zeroed stand-in context, host memory,
nothing touches a device): every R1_EINVAL the header lists, and n == 0, which passes every check, returns 0 and touches
nothing.  The device-resident refusals are in tests/test_gpu_head.py."""
import ctypes as C

import pytest

from test_entry_refusals import BUF, Harness

RATE = dict(nbrs=BUF, n_nbrs=1, cdfs=BUF, n_cdfs=1, blocks=BUF, n_blocks=1, trials=BUF, n=0, depth_state=None, tx_sizes=None,
            cfl_alpha=None, rate_add_out=BUF, rng_out=BUF, rng_stride=24)
PART = dict(nbrs=BUF, n_nbrs=1, cdfs=BUF, n_cdfs=1, nodes=BUF, partitions=BUF, n=0, rng_in=None, part_rate_out=BUF, rng_out=None)
COMMIT = dict(nbrs=BUF, n_nbrs=1, cdfs=BUF, n_cdfs=1, blocks=BUF, n_blocks=1, trials=BUF, n_trials=1, commits=BUF, state=BUF,
              n_states=0, call_id=0, group=1, nt=1, depth_state=None, tx_sizes=None, cfl_alpha=None)
RESET = dict(nbrs=BUF, n_nbrs=1, sel=BUF, n=0)
# BUF is zeroed memory: as tx_sizes it reads (TX_4X4, TX_4X4, TX_4X4)
DECIDED = [(dict(depth_state=BUF), -1), (dict(tx_sizes=BUF), -1), (dict(depth_state=BUF, tx_sizes=BUF), 0), (dict(cfl_alpha=BUF), 0)]
TABLE = [
    ("r1_intra_head_rate_batch", RATE, [
        (dict(), 0), (dict(ctx=None), -1), (dict(nbrs=None), -1), (dict(cdfs=None), -1), (dict(blocks=None), -1),
        (dict(trials=None), -1), (dict(rate_add_out=None), -1), (dict(rng_out=None), 0), (dict(n=-1), -1),
        (dict(n_nbrs=0), -1), (dict(n_cdfs=0), -1), (dict(n_blocks=0), -1), (dict(n_blocks=-2), -1),
        (dict(rng_stride=1), -1), (dict(rng_stride=0), -1), (dict(rng_stride=3), -1), (dict(rng_stride=2), 0),
        (dict(rng_out=None, rng_stride=0), 0),           # no rng wanted: the stride is not looked at
    ] + DECIDED),
    ("r1_partition_rate_batch", PART, [
        (dict(), 0), (dict(ctx=None), -1), (dict(nbrs=None), -1), (dict(cdfs=None), -1), (dict(nodes=None), -1),
        (dict(partitions=None), -1), (dict(part_rate_out=None), -1), (dict(rng_in=BUF), 0), (dict(rng_out=BUF), 0),
        (dict(n=-1), -1), (dict(n_nbrs=0), -1), (dict(n_cdfs=-1), -1),
    ]),
    ("r1_intra_head_commit_batch", COMMIT, [
        (dict(), 0), (dict(ctx=None), -1), (dict(nbrs=None), -1), (dict(cdfs=None), -1), (dict(blocks=None), -1),
        (dict(trials=None), -1), (dict(commits=None), -1), (dict(state=None), -1), (dict(n_states=-1), -1),
        (dict(n_nbrs=0), -1), (dict(n_cdfs=0), -1), (dict(n_blocks=0), -1), (dict(n_trials=0), -1),
        (dict(call_id=-1), -1), (dict(call_id=128), -1), (dict(call_id=127), 0),
        (dict(group=0), -1), (dict(group=4097), -1), (dict(group=4096), 0), (dict(nt=0), -1), (dict(nt=17), -1), (dict(nt=16), 0),
    ] + DECIDED),
    ("r1_head_nbr_reset_left_batch", RESET, [
        (dict(), 0), (dict(ctx=None), -1), (dict(nbrs=None), -1), (dict(sel=None), -1), (dict(n=-1), -1), (dict(n_nbrs=0), -1),
    ]),
]
ROWS = [(name, base, over, status) for name, base, cases in TABLE for over, status in cases]


@pytest.fixture(scope="module")
def harness():
    return Harness()


@pytest.mark.parametrize("name,base,over,status", ROWS, ids=["%s-%d" % (r[0][3:], i) for i, r in enumerate(ROWS)])
def test_status(harness, name, base, over, status):
    before = [bytes(m) for m in harness.mem]
    assert harness.call(name, base, over) == status
    assert [bytes(m) for m in harness.mem] == before          # n == 0 (and every refusal) touches nothing


def test_a_table_entry_that_is_no_tx_size(harness):
    """tx_sizes is a HOST table: an entry past the enum is R1_EINVAL before anything is enqueued"""
    L = harness.L
    fake = C.addressof(harness.fake_ctx)
    buf = C.addressof(harness.mem[2])
    for table, status in (((0, 1, 2), 0), ((0, 19, 2), -1), ((255, 0, 0), -1), ((18, 18, 18), 0)):
        t = (C.c_uint8 * 3)(*table)
        assert L.r1_intra_head_rate_batch(fake, buf, 1, buf, 1, buf, 1, buf, 0, buf, t, None, buf, None, 0, None) == status
        assert L.r1_intra_head_commit_batch(fake, buf, 1, buf, 1, buf, 1, buf, 1, buf, buf, 0, 0, 1, 1, buf, t, None, None) == status


def test_abi_and_symbols():
    from rav1e_amd import _lib
    assert _lib.load().r1_abi_version() == 7
    assert {t[0] for t in TABLE} <= set(_lib.SYMBOLS)
    assert all(cases[0] == (dict(), 0) for _, _, cases in TABLE) and len(ROWS) >= 60
