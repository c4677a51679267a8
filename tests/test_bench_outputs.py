"""bench.py's plain run and --dump-outputs: the options parse, the dump plan stays under its byte limit, is the
same from run to run and writes exact values; on the GPU a plain run times exactly --steps steps, measures
nothing else, and dumps what the fused candidate path computed (checked against the CPU oracle)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_is_the_default_and_full_is_an_option():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def _ladder_outs(coeff_dtype):
    """the headline's output buffers at 4K, K = 16 (shapes and dtypes only: stride-0 views, no memory)"""
    import torch
    from rav1e_amd import workload as W
    outs = {}
    for s, c in W.speed6_ladder(3840, 2160, 16).items():
        n = len(c)
        outs[s] = {"sad": torch.zeros(1, dtype=torch.int32).expand(n),
                   "satd": torch.zeros(1, dtype=torch.int32).expand(n),
                   "coeffs": torch.zeros(1, s * s, dtype=coeff_dtype).expand(n, s * s)}
    return outs


@pytest.mark.parametrize("bd", [8, 10])
def test_dump_plan_of_the_headline_fits_and_is_fixed(bd):
    import torch
    outs = _ladder_outs(torch.int16 if bd == 8 else torch.int32)
    p = bench.dump_plan(outs)
    total = 0
    for name, t, idx, dt in p:
        rows = t.shape[0] if idx is None else len(idx)
        total += rows * (t.numel() // t.shape[0]) * np.dtype(dt).itemsize
        if idx is not None:
            assert len(idx) and (np.diff(idx) > 0).all() and idx[-1] < t.shape[0]
        # exact: 16-bit integers in float32, 32-bit ones in float64
        assert dt == (np.float32 if t.element_size() == 2 else np.float64), name
    assert total <= bench.DUMP_LIMIT
    assert {n for n, *_ in p} == {"%s_%dx%d" % (b, s, s) for s in (64, 32, 16, 8) for b in ("sad", "satd", "coeffs")}
    # the same sample in another process' plan; the coefficient rows are candidates the scalars keep
    q = {n: idx for n, _, idx, _ in bench.dump_plan(_ladder_outs(torch.int16 if bd == 8 else torch.int32))}
    for n, _, idx, _ in p:
        assert (idx is None and q[n] is None) or np.array_equal(idx, q[n]), n
    for s in (64, 32, 16, 8):
        c, sad = q["coeffs_%dx%d" % (s, s)], q["sad_%dx%d" % (s, s)]
        assert c is not None and (sad is None or np.isin(c, sad).all())


def test_dump_outputs_writes_the_buffers_exactly(tmp_path):
    import torch
    g = torch.Generator().manual_seed(0)
    outs = {8: {"sad": torch.randint(0, 1 << 30, (300,), generator=g, dtype=torch.int32),
                "coeffs": torch.randint(-32768, 32767, (300, 64), generator=g, dtype=torch.int16),
                "dist": torch.randint(0, 1 << 50, (300,), generator=g, dtype=torch.int64)}}
    bench.dump_outputs(str(tmp_path / "whole"), outs)
    for name, t in outs[8].items():
        a = np.load(tmp_path / "whole" / ("%s_8x8.npy" % name))
        assert a.dtype == (np.float32 if name == "coeffs" else np.float64)
        assert np.array_equal(a.astype(np.int64), t.numpy().astype(np.int64)), name
    # over the limit: a seeded sample of rows, the same twice
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, limit=20000)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) == ["coeffs_8x8.npy", "dist_8x8.npy", "sad_8x8.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in files) <= 20000      # 128: the .npy header
    plan = {n: idx for n, _, idx, _ in bench.dump_plan(outs, 20000)}
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b)
        name = f[:-len("_8x8.npy")]
        idx = plan[f[:-4]]
        if idx is None:
            idx = np.arange(300)
        assert len(a) == len(idx) and (name != "coeffs" or len(idx) < 300)
        assert np.array_equal(a.astype(np.int64), outs[8][name].numpy()[idx].astype(np.int64))


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_candidates(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    from rav1e_amd import workload as W
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--prewarm-ms", "0", "--dump-outputs", str(dump), "--detail-out", str(tmp_path / "detail.json")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    # a plain run measures nothing beside the headline
    assert d["extra_lines"] == [] and "cpu_baseline" not in d and "pipelined_value" not in d and "parity_ok" not in d
    assert sum(f.stat().st_size for f in dump.iterdir()) <= bench.DUMP_LIMIT + 128 * 12
    # the dump is what the path computed: sampled candidates of every size against the scalar oracle
    cands = W.speed6_ladder(3840, 2160, 16)
    a, b = O.HostPlane(3840, 2160, 8), O.HostPlane(3840, 2160, 8)
    a.data, b.data = W.random_plane_array(3840, 2160, 8, 1), W.random_plane_array(3840, 2160, 8, 2)
    pa, pb = a.cstruct(), b.cstruct()
    L = O.lib()
    plan = {n: idx for n, _, idx, _ in bench.dump_plan(_ladder_outs(torch.int16))}
    for s, ts in ((64, 4), (32, 3), (16, 2), (8, 1)):
        tag = "%dx%d" % (s, s)
        cidx = plan["coeffs_" + tag]
        sidx = plan["sad_" + tag] if plan["sad_" + tag] is not None else np.arange(len(cands[s]))
        pick = cidx[np.linspace(0, len(cidx) - 1, 6).astype(int)]
        sub = np.ascontiguousarray(cands[s][pick])
        sad, satd = np.zeros(len(sub), np.uint32), np.zeros(len(sub), np.uint32)
        co = np.zeros((len(sub), s * s), np.int16)
        assert L.r1o_rdo_cand_batch(C.byref(pa), C.byref(pb), s, s, ts, O.ptr(sub), len(sub),
                                    O.ptr(sad), O.ptr(satd), O.ptr(co), None) == 0
        rows = np.searchsorted(sidx, pick)
        assert np.array_equal(np.load(dump / ("sad_%s.npy" % tag))[rows], sad), tag
        assert np.array_equal(np.load(dump / ("satd_%s.npy" % tag))[rows], satd), tag
        assert np.array_equal(np.load(dump / ("coeffs_%s.npy" % tag))[np.searchsorted(cidx, pick)], co), tag
