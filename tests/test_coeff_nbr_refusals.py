"""What the four neighbour-context entry points answer to a bad argument, as a table in the manner of
tests/test_entry_refusals.py (its harness: a zeroed stand-in context, host memory, nothing touches a device): every
R1_EINVAL the header lists, and n == 0, which passes every check, returns 0 and touches nothing."""
import pytest

from test_entry_refusals import BUF, Harness

GATHER = dict(contexts=BUF, n_contexts=1, descs=BUF, n=0, bw=16, bh=16, xdec=1, ydec=1, blocks_out=BUF, chains_out=BUF)
STORE = dict(descs=BUF, n=0, bw=16, bh=16, tx_size=2, xdec=1, ydec=1, ctx_in=BUF, state=None, call_id=0, contexts=BUF, n_contexts=1)
RESET = dict(contexts=BUF, n_contexts=1, sel=BUF, n=0, planes=3)
WINNER = dict(state=BUF, n_states=0, call_id=0, tx_type_mask=0x0E0F, is_inter=0, uv_tx_size=1, eob_win=None, ntx=4, trials=BUF)
# what the gather and the store share: sizes and subsampling
GEOMETRY = [
    (dict(bw=12), -1), (dict(bw=128, bh=128), -1), (dict(bw=2, bh=8), -1), (dict(bw=64, bh=8), -1), (dict(bw=4, bh=32), -1),
    (dict(bw=64, bh=64), 0), (dict(bw=4, bh=16, tx_size=13), 0), (dict(bw=64, bh=16, tx_size=18), 0),
    (dict(xdec=0, ydec=1), -1), (dict(xdec=2, ydec=0), -1), (dict(xdec=1, ydec=-1), -1), (dict(xdec=0, ydec=0), 0),
    (dict(xdec=1, ydec=0), 0), (dict(xdec=1, ydec=0, bw=8, bh=16, tx_size=1), -1),      # 4:2:2 admits no tall block
    (dict(xdec=1, ydec=0, bw=4, bh=16, tx_size=0), -1), (dict(xdec=1, ydec=0, bw=16, bh=4, tx_size=0), 0),
]
TABLE = [
    ("r1_coeff_nbr_gather_batch", GATHER, [
        (dict(), 0), (dict(ctx=None), -1), (dict(contexts=None), -1), (dict(descs=None), -1),
        (dict(blocks_out=None), 0), (dict(chains_out=None), 0), (dict(blocks_out=None, chains_out=None), -1),
        (dict(n=-1), -1), (dict(n_contexts=0), -1), (dict(n_contexts=-3), -1),
    ] + [(dict((k, v) for k, v in o.items() if k != "tx_size"), s) for o, s in GEOMETRY]),
    ("r1_coeff_nbr_store_batch", STORE, [
        (dict(), 0), (dict(ctx=None), -1), (dict(contexts=None), -1), (dict(descs=None), -1), (dict(ctx_in=None), 0),
        (dict(n=-1), -1), (dict(n_contexts=0), -1),
        (dict(tx_size=19), -1), (dict(tx_size=-1), -1), (dict(tx_size=3), -1), (dict(tx_size=9), -1), (dict(tx_size=1), 0),
        (dict(tx_size=7), 0), (dict(bw=32, bh=8, tx_size=2), -1),
        (dict(state=BUF, call_id=128), -1), (dict(state=BUF, call_id=-1), -1), (dict(state=BUF, call_id=127), 0),
        (dict(call_id=500), 0),             # no state: the call_id is not looked at
    ] + GEOMETRY),
    ("r1_coeff_nbr_reset_left_batch", RESET, [
        (dict(), 0), (dict(ctx=None), -1), (dict(contexts=None), -1), (dict(sel=None), -1), (dict(n=-1), -1),
        (dict(n_contexts=0), -1), (dict(planes=0), -1), (dict(planes=4), -1), (dict(planes=1), 0), (dict(planes=2), 0),
    ]),
    ("r1_rd_winner_tx_type_batch", WINNER, [
        (dict(), 0), (dict(ctx=None), -1), (dict(state=None), -1), (dict(trials=None), -1), (dict(n_states=-1), -1),
        (dict(call_id=-1), -1), (dict(call_id=128), -1), (dict(call_id=127), 0),
        (dict(tx_type_mask=0), -1), (dict(tx_type_mask=0x1000), -1), (dict(tx_type_mask=0x10001), -1), (dict(tx_type_mask=0x0001), 0),
        (dict(tx_type_mask=0xFFFF, is_inter=1, eob_win=BUF), 0), (dict(tx_type_mask=0x1FFFF, is_inter=1, eob_win=BUF), -1),
        (dict(is_inter=1), -1),             # inter reads the winner's eobs
        (dict(is_inter=1, eob_win=BUF), 0),
        (dict(uv_tx_size=19), -1), (dict(uv_tx_size=-1), -1), (dict(uv_tx_size=18), 0),
        (dict(ntx=0), -1), (dict(ntx=17), -1), (dict(ntx=1), 0), (dict(ntx=16), 0),
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


def test_table_lists_every_refusal_of_the_header():
    assert {t[0] for t in TABLE} == {"r1_coeff_nbr_gather_batch", "r1_coeff_nbr_store_batch", "r1_coeff_nbr_reset_left_batch",
                                    "r1_rd_winner_tx_type_batch"}
    assert all(cases[0] == (dict(), 0) for _, _, cases in TABLE) and len(ROWS) >= 80
