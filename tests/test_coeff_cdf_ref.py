"""The device-resident coefficient CDF context without a GPU: tests/golden/coeff_cdf_ref.npz (the reference's
write_coeffs_lv_map executed over sequences of blocks on ONE ContextWriter whose CDFs are never rolled back,
gen_coeff_cdf_ref.py) against the NumPy model the GPU tests use (tests/coeff_cdf_model.py): every stored context and
rate, what the owned-rows rule of the scatter is worth, the packing glue, the struct layout against the header compiled
as C, and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coeff_rate_model as M
import coeff_cdf_model as DM
from rav1e_amd import rdo_glue as RG
from rav1e_amd.types import COEFF_CDF_CONTEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return DM.load_fixture()


def test_fixture_holds_the_sequences_the_issue_names(fixture):
    G, seqs = fixture
    assert len(seqs) >= 40 and all(3 <= len(s.blocks) <= 6 for s in seqs)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "coeff_cdf_ref.npz")) < 1 << 20
    blocks = [c for s in seqs for c in s.blocks]
    assert {c.cb for c in blocks} == {2, 4}
    assert {(c.xdec, c.ydec) for c in blocks} == {(1, 1), (1, 0), (0, 0)}
    # all five tx-type tables are written somewhere
    tables = {DM.TX_TABLE[M.tx_set(c.ts, c.inter, c.red)] for c in blocks
              if M.NUM_TX_SET[M.tx_set(c.ts, c.inter, c.red)] > 1 and any(int(e) for e in c.eobs[0])}
    assert tables == set(DM.TX_TABLE.values())
    assert any(c.do_chroma and c.ntx[1] == 0 for c in blocks) and any(not c.do_chroma for c in blocks)
    assert any(c.do_chroma and c.ntx[1] and M.txs_ctx(c.ts) == M.txs_ctx(c.uv_ts) for c in blocks)
    assert any(not any(int(e) for p in range(3) for e in c.eobs[p]) for c in blocks)
    # the packed layout is R1CoeffCdfContext's: the reference's field names and shapes in the struct's order
    names = [n for n in COEFF_CDF_CONTEXT.names if n != "pad"]
    want = [("eob_flag_cdf" + n[8:]) if n.startswith("eob_flag") else n + "_cdf" for n in names]
    assert [str(f) for f in G["fields"]] == want
    for n, shape in zip(names, G["field_shapes"]):
        assert tuple(int(v) for v in shape if v) == COEFF_CDF_CONTEXT.fields[n][0].shape, n
    assert G["seq_ctx"].shape[2] == DM.CTX_U16 - 6 == 3930


def test_model_reproduces_every_stored_context_and_rate(fixture):
    """every sequence replayed block after block on one record: the whole context behind every block, the rate, the
    final rng and the 96 context bytes; the padding stays zero"""
    _, seqs = fixture
    for s in seqs:
        ctx = s.context(0)
        for c in s.blocks:
            r = c.adapt(ctx)
            key = (s.name, c.step, c.name)
            assert r["rate"] == c.rate and r["rng"] == c.rng_out, key
            assert r["ctx"] == c.ctx_out.tolist(), key
            got, want = DM.packed_of(ctx), s.packed[c.step + 1]
            assert np.array_equal(got, want), (key, np.nonzero(got != want)[0][:8].tolist())
            assert not ctx["pad"].any()
        assert not np.array_equal(s.packed[0], s.packed[len(s.blocks)]), s.name


def test_gather_equals_the_slices_the_block_fixture_stores():
    """the gather rule on a context built from a slice: scatter a stored R1CoeffCdfs of the block fixture into an empty
    context with every row owned, gather it back, and get the stored slice"""
    import coeff_rate_block_model as BM
    _, cases = BM.load_fixture()
    for c in cases[::3]:
        for pt, ts in ((0, c.ts), (1, c.uv_ts)):
            ctx = np.zeros(1, COEFF_CDF_CONTEXT)[0]
            DM.scatter(ctx, c.cdfs[pt], ts, pt, c.inter, c.red, whole_tables=True)
            assert DM.gather(ctx, ts, pt, c.inter, c.red).tobytes() == c.cdfs[pt].tobytes(), (c.name, pt)


def test_whole_table_scatter_moves_the_444_sequences(fixture):
    """the scatter switched to whole tables: the chroma slice's stale txb_skip rows 0-6 overwrite what luma adapted, in
    exactly the sequences that hold a block with do_chroma whose luma and chroma txs_ctx are equal (luma always moves
    its half of the table) -- the sequences named 444same among them"""
    _, seqs = fixture
    moved, expect = set(), set()
    for s in seqs:
        ctx = s.context(0)
        for c in s.blocks:
            if c.do_chroma and M.txs_ctx(c.ts) == M.txs_ctx(c.uv_ts):
                expect.add(s.name)          # luma codes at least one txb_skip symbol in every block; the chroma slice goes
                                            # back behind V even where the chroma grid is empty (4x16 in 4:2:0)
            c.adapt(ctx, whole_tables=True)
        if not np.array_equal(DM.packed_of(ctx), s.packed[len(s.blocks)]):
            moved.add(s.name)
    assert moved == expect, (sorted(moved ^ expect))
    assert {s.name for s in seqs if s.name.startswith("444same")} <= moved and len(moved) < len(seqs)


def test_coeff_cdf_context_packs_the_reference_fields(fixture):
    """rdo_glue.coeff_cdf_context: a dict of the reference's field arrays (either spelling) -> the record"""
    G, seqs = fixture
    rec = seqs[3].context(2)
    by_ref = {str(f): rec[n] for f, n in zip(G["fields"], [n for n in COEFF_CDF_CONTEXT.names if n != "pad"])}
    assert RG.coeff_cdf_context(by_ref).tobytes() == rec.tobytes()
    by_name = {n: rec[n].tolist() for n in COEFF_CDF_CONTEXT.names if n != "pad"}
    assert RG.coeff_cdf_context(by_name).tobytes() == rec.tobytes()
    del by_name["dc_sign"]
    with pytest.raises(KeyError):
        RG.coeff_cdf_context(by_name)
    by_ref["coeff_br_cdf"] = by_ref["coeff_br_cdf"][:4]
    with pytest.raises(AssertionError):
        RG.coeff_cdf_context(by_ref)


def test_struct_layout_equals_the_header_compiled_as_c(tmp_path):
    """R1CoeffCdfContext: 7872 bytes, a multiple of 16, and every field's offset and size, include/rav1e_amd.h compiled
    by gcc as C against the NumPy dtype"""
    name, dt = "R1CoeffCdfContext", COEFF_CDF_CONTEXT
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rav1e_amd.h"', 'int main(void) {',
             '  printf("%s.size %%zu 0\\n", sizeof(%s));' % (name, name)]
    for f in dt.names:
        lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in out if l}
    assert dt.itemsize == 7872 and dt.itemsize % 16 == 0 and got[name + ".size"] == [7872, 0]
    assert len(dt.names) == 19 and len(got) == 20
    for f in dt.names:
        assert got[name + "." + f] == [dt.fields[f][1], dt.fields[f][0].itemsize], (f, got[name + "." + f])


def test_library_exports_the_cdf_context_calls():
    from rav1e_amd import _lib
    L = _lib.load()
    for sym, nargs in (("r1_coeff_cdf_slice_batch", 9), ("r1_coeff_cdf_adapt_batch", 30)):
        assert hasattr(L, sym) and sym in _lib.SYMBOLS and len(getattr(L, sym).argtypes) == nargs
    assert L.r1_coeff_cdf_adapt_batch.argtypes[25] is C.c_int
    assert L.r1_abi_version() == 7
