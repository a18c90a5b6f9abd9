"""Every schedule of the persistent interior-point solver against the oracle.

Batch size against the device's SIMD count selects how noc/ipm.py and csrc/ipm_persistent.hip run
a batch: probe launch + cost-ordered resume, heavy-first split on two streams, tail ladder +
gather, two or four speculative candidates, the wide kernel, the one- or the two-wave instance
(and the launch-per-phase loop beside them).  tests/test_ipm_gpu.py shows those paths equal to
each other; here each one, as the DEFAULT selection reaches it, is held to whole solves of
oracle/noc_oracle.py (P:127-254, S:108-202) committed in tests/golden/golden_v3.npz
(tests/golden/make_golden.py: schedule_fixtures).  A batch of any size is drawn from a group's K
fixture rows, so every trajectory has an oracle answer whatever the device's SIMD count.

Tolerances (those of test_random_solves_match_oracle): outer iterations and KKT solves equal to
the oracle's exactly, controls within 1e-6, the oracle's final cost (bp = 0) of the GPU's controls
within 1e-8 max(1, |cost|); trajectories drawn from the same fixture row bit-identical among
themselves, whatever workgroup, launch position or instance solved them.  Every fixture row's
accept tests are at least 64 eps |cost| from a tie (make_golden.py: MIN_MARGIN), so rounding
cannot turn one; the one exempt row (cart200's heavy row) carries the retry-cap run.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v3.npz")
GROUPS = {"cart30": ("cartpole", 30), "cart200": ("cartpole", 200), "pend150": ("pendulum", 150)}
# compared bit for bit between trajectories of the same fixture row
TWIN_KEYS = ("u", "x", "total_it", "kkt_solves", "it", "inner", "bp", "rp", "rinc")


@functools.lru_cache(maxsize=None)
def _fixture(tag, mode="par"):
    """One group's rows (read-only): inputs, the oracle's controls, counts and final cost."""
    from oracle import noc_oracle as O, problems as PR
    gold = np.load(GOLDEN)
    name, N = GROUPS[tag]
    g = lambda k: gold[f"{tag}/{k}"]
    prob = O.NumpyProblem(PR.pendulum_ocp(1.0 / N) if name == "pendulum" else PR.cartpole_ocp(1.0 / N))
    fx = SimpleNamespace(tag=tag, name=name, N=N, prob=prob, x0=g("x0"), u0=g("u0"),
                         K=len(g("x0")), mode=mode)
    if mode == "par":
        fx.u, fx.iters, fx.kkt_solves, fx.cost = g("par_u"), g("par_iters"), g("par_kkt_solves"), g("par_cost")
    else:  # the oracle's seq solve (one KKT solve per iteration, S:108-177); its cost from its controls
        fx.u, fx.iters, fx.kkt_solves = g("seq_u"), g("seq_iters"), None
        fx.cost = np.array([_final_cost(fx, fx.u[k], k) for k in range(fx.K)])
    fx.heavy = int(gold["cart200/heavy_row"]) >= 0 if tag == "cart200" else False
    for v in vars(fx).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


def _final_cost(fx, U, k):
    from oracle import noc_oracle as O
    return fx.prob.total_cost(O.rollout(fx.prob.dynamics, U, fx.x0[k].copy()), U, 0.0)


def _simds():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _clean_env(monkeypatch, **env):
    """Only the variables a case names are set: the default selection is what runs."""
    for k in list(os.environ):
        if k.startswith("NOC_PERSIST_") or k == "NOC_WIDE_WAVES":
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(fx, Bt, seed, **kw):
    """An engine loaded with Bt trajectories drawn from the fixture rows: each row once, then a
    seeded draw.  Returns (engine, idx)."""
    from noc import problems
    from noc.ipm import BatchedIPM
    idx = np.empty(Bt, dtype=np.int64)
    k = min(fx.K, Bt)
    idx[:k] = np.arange(k)
    idx[k:] = np.random.default_rng(seed).integers(0, fx.K, Bt - k)
    kw.setdefault("lanes", 64)
    kw.setdefault("persistent", True)
    eng = BatchedIPM(problems.make_problem(fx.name, fx.N).family, fx.N, Bt, **kw)
    eng.load(fx.u0[idx], fx.x0[idx])
    return eng, idx


def _check(eng, fx, idx, case):
    from noc import _lib
    torch.cuda.synchronize()
    t = {k: eng.t[k].cpu().numpy() for k in TWIN_KEYS + ("phase", "repeats")}
    assert np.all(t["phase"] == _lib.PHASE_DONE), (case, np.flatnonzero(t["phase"] != _lib.PHASE_DONE))
    bad = np.flatnonzero(t["total_it"] != fx.iters[idx])
    assert bad.size == 0, (case, "total_it", bad[:8], idx[bad[:8]], t["total_it"][bad[:8]])
    if fx.kkt_solves is not None:
        bad = np.flatnonzero(t["kkt_solves"] != fx.kkt_solves[idx])
        assert bad.size == 0, (case, "kkt_solves", bad[:8], idx[bad[:8]], t["kkt_solves"][bad[:8]])
    uniq, first = np.unique(idx, return_index=True)
    du = float(np.max(np.abs(t["u"] - fx.u[idx])))
    dc = [abs(_final_cost(fx, t["u"][b], k) - fx.cost[k]) / max(1.0, abs(fx.cost[k]))
          for k, b in zip(uniq, first)]
    print(f"SCHEDULE {case}: Bt {len(idx)} max|u - u_oracle| {du:.3e} max cost error {max(dc):.3e} "
          f"repeats {int(t['repeats'].sum())}")
    assert du < 1e-6, (case, du)
    assert max(dc) <= 1e-8, (case, dc)
    twin = first[np.searchsorted(uniq, idx)]   # the first trajectory drawn from the same row
    for k in TWIN_KEYS:
        assert np.array_equal(t[k], t[k][twin]), (case, k)
    return t


def _mode(mode):
    from noc import _lib
    return _lib.MODE_PAR if mode == "par" else _lib.MODE_SEQ


@pytest.mark.parametrize("mode", ["par", "seq"])
def test_probe_ordered_resume_matches_oracle(mode, monkeypatch):
    """Beyond two waves per SIMD: probe launch, cost-ordered resume on the two-wave instance."""
    _clean_env(monkeypatch)
    fx = _fixture("cart30", mode)
    eng, idx = _engine(fx, 2 * _simds() + 77, seed=1)
    assert eng.Bt > eng._resident_slots() and not eng._tail_eligible()
    eng.solve_persistent(mode=_mode(mode))
    assert eng._order is not None
    order = eng._order.cpu().numpy()
    assert sorted(order.tolist()) == list(range(eng.Bt)) and order.tolist() != list(range(eng.Bt))
    _check(eng, fx, idx, f"probe-{mode}")


def test_default_heavy_split_matches_oracle(monkeypatch):
    """#SIMDs < B <= 2 #SIMDs: the probe order with the costliest #SIMDs / 8 trajectories on two
    speculative candidates each, beside the rest on the two-wave instance (solve_split)."""
    _clean_env(monkeypatch)
    fx = _fixture("cart30")
    eng, idx = _engine(fx, _simds() + 77, seed=2)
    assert eng._heavy_split_eligible() and not eng._tail_eligible()
    eng.solve_persistent()
    assert eng._order is not None
    _check(eng, fx, idx, "heavy")


@pytest.mark.parametrize("forced", [False, True])
def test_heavy_split_on_dense_blocks_matches_oracle(forced, monkeypatch):
    """NOC_PERSIST_STRUCT=0 at the split's batch size: both launches of a split share the workspace's
    block buffers, so they must share one layout -- no split by default (the candidates need the
    compact blocks), and a forced one (NOC_PERSIST_HEAVY) runs its heavy launch on the dense
    one-wave instance whatever NOC_PERSIST_HEAVY_SPEC asks."""
    env = dict(NOC_PERSIST_STRUCT="0")
    if forced:
        env.update(NOC_PERSIST_HEAVY="64", NOC_PERSIST_HEAVY_SPEC="2")
    _clean_env(monkeypatch, **env)
    fx = _fixture("cart30")
    eng, idx = _engine(fx, _simds() + 77, seed=2)
    assert not eng._heavy_split_eligible()
    if forced:
        eng.solve_persistent(schedule="probe")
        assert eng._order is not None
    else:
        eng.solve_persistent()
        assert eng._order is None  # one index-order launch of the dense two-wave instance
    _check(eng, fx, idx, f"heavy-dense-{'forced' if forced else 'default'}")


def test_heavy_split_without_candidates_matches_oracle(monkeypatch):
    """The split with its heavy launch on the plain one-wave instance."""
    _clean_env(monkeypatch, NOC_PERSIST_HEAVY="64", NOC_PERSIST_HEAVY_SPEC="0")
    fx = _fixture("cart30")
    eng, idx = _engine(fx, _simds() + 77, seed=2)
    eng.solve_persistent(schedule="probe")
    assert eng._order is not None
    _check(eng, fx, idx, "heavy-1wave")


def test_tail_ladder_and_gather_match_oracle(monkeypatch):
    """One wave per SIMD: capped launches, then the trajectories still running gathered into a
    small workspace and resumed with speculative candidates.  The caps sit inside cart30's solve
    counts (127-159), so the last one leaves only the two slowest rows' copies running."""
    _clean_env(monkeypatch, NOC_PERSIST_TAIL_CAPS="40,80,120,150")
    fx = _fixture("cart30")
    simds = _simds()
    eng, idx = _engine(fx, simds, seed=3)
    assert eng._tail_eligible() and not eng._heavy_split_eligible()
    eng.solve_persistent()
    log = eng.tail_log
    assert any(0 < 2 * r <= simds for _, r in log), log
    print(f"SCHEDULE tail: tail_log {log}")
    _check(eng, fx, idx, "tail")


@pytest.mark.parametrize("mode", ["par", "seq"])
@pytest.mark.parametrize("div", [2, 4])
def test_speculative_candidates_match_oracle(div, mode, monkeypatch):
    """B = #SIMDs / 2 and #SIMDs / 4: two and four candidate waves per trajectory (spec_auto)."""
    _clean_env(monkeypatch)
    fx = _fixture("cart30", mode)
    eng, idx = _engine(fx, _simds() // div, seed=4 + div)
    assert not eng._tail_eligible() and not eng._heavy_split_eligible()
    assert eng.Bt * div <= _simds() < eng.Bt * 2 * div  # spec_auto's branch for `div` candidates
    eng.solve_persistent(mode=_mode(mode))
    assert eng._order is None
    _check(eng, fx, idx, f"spec{div}-{mode}")


@pytest.mark.parametrize("size", ["half", "5"])
def test_candidates_across_the_rp_clip_match_oracle(size, monkeypatch):
    """N = 200 cart-poles with candidates (two at #SIMDs / 2, four at B = 5 -- the default
    selection there, ahead of the wide kernel); the heavy row's retry-cap run is accounted
    without recomputation (repeats)."""
    _clean_env(monkeypatch)
    fx = _fixture("cart200")
    eng, idx = _engine(fx, _simds() // 2 if size == "half" else 5, seed=8)
    eng.solve_persistent()
    t = _check(eng, fx, idx, f"spec-repeats-{size}")
    if fx.heavy:
        assert int(t["repeats"].sum()) > 0


def test_every_retry_recomputed_matches_oracle(monkeypatch):
    """NOC_WS_NO_REPEAT_SKIP: the identical retries at the rp clip computed one by one."""
    _clean_env(monkeypatch)
    from noc import _lib
    fx = _fixture("cart200")
    eng, idx = _engine(fx, 8, seed=9)
    eng.ws.flags = _lib.WS_NO_REPEAT_SKIP
    eng.solve_persistent()
    t = _check(eng, fx, idx, "no-skip")
    assert int(t["repeats"].sum()) == 0


def test_dense_one_wave_instance_matches_oracle(monkeypatch):
    _clean_env(monkeypatch, NOC_PERSIST_STRUCT="0")
    fx = _fixture("cart30")
    eng, idx = _engine(fx, 37, seed=10)
    eng.solve_persistent()
    _check(eng, fx, idx, "dense")


@pytest.mark.parametrize("waves", [None, "2"])
def test_wide_kernel_matches_oracle(waves, monkeypatch):
    """Pendulum, N = 150 > 128, B = 4 <= #CUs: the wide kernel by default, four or two waves."""
    _clean_env(monkeypatch, **({} if waves is None else {"NOC_WIDE_WAVES": waves}))
    fx = _fixture("pend150")
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 4
    eng, idx = _engine(fx, 4, seed=11)
    eng.solve_persistent()
    _check(eng, fx, idx, f"wide-{waves or 'default'}")


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("lanes", [8, 32])
def test_launch_per_phase_loop_matches_oracle(lanes, compact, monkeypatch):
    """The launch-per-phase loop on compact and dense blocks, at scan widths with several
    segments per trajectory (lanes 8) and with dead lanes (lanes 32, N = 30)."""
    _clean_env(monkeypatch)
    fx = _fixture("cart30")
    eng, idx = _engine(fx, 37, seed=12, lanes=lanes, persistent=False, compact=compact)
    assert eng.compact == compact
    eng.solve()
    _check(eng, fx, idx, f"loop-l{lanes}-{'compact' if compact else 'dense'}")
