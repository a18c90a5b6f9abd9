"""bench.py on the GPU: a plain run stops at the headline figure, --full adds the other legs, and
--dump-outputs writes what the last timed step returned -- the same bits from run to run, and the
bits a caller of the timed path (noc.lqt.kkt_solve_tiled on the bench's blocks) receives."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# odd sizes: 37 trajectories (no multiple of a wave's trajectories), horizon 20
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--horizon", "20", "--global-batch", "37"]


def _bench(monkeypatch, argv):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    (line,) = [json.loads(s) for s in buf.getvalue().splitlines() if s.startswith("{")]
    return bench, line


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def expected():
    """What a caller of the timed path receives for the bench's inputs (computed once)."""
    import torch
    from noc import lqt, problems
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    blocks = problems.make_bench_blocks("cartpole", N=20, batch=37, seed=bench.BENCH_SEED,
                                        shard=(37, 0))
    out = lqt.kkt_solve_tiled(blocks["tiled"], reg=blocks["reg"], want_gains=False)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out._asdict().items() if t is not None}


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, monkeypatch, expected):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _, line = _bench(monkeypatch, SMALL + ["--dump-outputs", a])
    _bench(monkeypatch, SMALL + ["--dump-outputs", b])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(37 / (line["ms_per_step"] * 1e-3))
    for k in ("ipm_solve", "cpu_baseline", "residual_vs_seq_ref"):
        assert k not in line, k
    da, db = _load(a), _load(b)
    assert set(da) == set(expected) and set(db) == set(expected)
    assert {"dx", "du", "pred", "feasible"} <= set(da)
    for k, want in expected.items():
        assert da[k].dtype in (np.float32, np.float64), (k, da[k].dtype)
        assert da[k].shape == want.shape, k
        assert np.array_equal(da[k], db[k]), k                      # run to run
        assert np.array_equal(da[k], want.astype(da[k].dtype)), k   # the caller's arrays
    assert da["dx"].dtype == np.float64 and da["dx"].shape == (37, 21, 4)


def test_dump_beyond_the_budget_is_a_fixed_sample(tmp_path, monkeypatch, expected):
    import bench
    total = sum(v.size * 8 for v in expected.values())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", total // 3)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _bench(monkeypatch, SMALL + ["--dump-outputs", a])
    _bench(monkeypatch, SMALL + ["--dump-outputs", b])
    da, db = _load(a), _load(b)
    keep = da["dx"].shape[0]
    assert 1 <= keep <= 37 // 3
    assert sum(v.nbytes for v in da.values()) <= total // 3
    idx = np.sort(np.random.default_rng(0).choice(37, keep, replace=False))
    assert set(da) == set(expected)
    for k, want in expected.items():
        assert np.array_equal(da[k], db[k]), k
        assert np.array_equal(da[k], want[idx].astype(da[k].dtype)), k


def test_full_adds_the_other_legs(monkeypatch):
    _, line = _bench(monkeypatch, SMALL + ["--full", "--cpu-seconds", "0.2", "--cpu-sample", "8"])
    assert line["ipm_solve"]["trajectories"] == 37 and line["ipm_solve"]["wall_ms"] > 0
    assert line["ipm_solve"]["bit_identical_to_recompute_all"] is True
    assert line["cpu_baseline"]["value"] > 0
    res = line["residual_vs_seq_ref"]
    assert res["max"] <= res["tolerance"] and res["feasible_equal"] is True
