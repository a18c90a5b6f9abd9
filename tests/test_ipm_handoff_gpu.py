"""Hand-offs of one interior-point solve between the drivers, in every direction: the
launch-per-phase loop (noc_ipm_step and its two-stream sub-steps, dense and compact blocks), the
one-wave persistent kernel and the wide persistent kernel (noc_ipm_solve, NOC_WS_RESUME).

The contract is the per-trajectory state of noc_ipm_ws (include/noc_hip.h).  Every case first
asserts a census -- the workspace at the hand-off holds the phases the case is about -- and then
compares with the uninterrupted solve by the driver that finishes:
  * counters (total_it, kkt_solves, final phase, bp): identical;
  * controls: 1e-12 relative where both sides run the one-wave / lanes-64 arithmetic (the bound of
    test_ipm_gpu.py::test_persistent_solve_equals_multilaunch_loop); 1e-8 where the wide kernel is
    on one side (test_wide_solve_matches_one_wave_kernel), on a start where the uninterrupted
    one-wave and wide solves have equal counts (asserted).
The hand-off point is the first one at which the census holds (a bounded, deterministic search:
the solves are deterministic, so it is the same point in every run)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COUNTERS = ("total_it", "kkt_solves", "phase", "bp")
WIDE_SEEDS = (33, 5, 4)


def _problem(name, N, Bt, seed):
    from noc import problems
    ocp = problems.make_problem(name, N)
    x0, u0 = problems.initial_conditions(name, N, Bt, seed=seed)
    return ocp, x0, u0


def _snapshot(eng, keys=COUNTERS + ("u",)):
    torch.cuda.synchronize()
    return {k: eng.t[k].cpu().numpy().copy() for k in keys}


def _uninterrupted(ocp, N, Bt, x0, u0, wide, monkeypatch, spec=None):
    """The whole solve by one persistent kernel (wide: NOC_PERSIST_WIDE)."""
    from noc import _lib
    from noc.ipm import BatchedIPM
    monkeypatch.setenv("NOC_PERSIST_WIDE", wide)
    if spec is not None:
        monkeypatch.setenv("NOC_PERSIST_SPEC", spec)
    eng = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=True)
    plan = _lib.ipm_plan(eng._lib, eng.fam_c, N, Bt)
    assert plan[_lib.PLAN_FAMILY] == (2 if wide == "1" else 1), plan     # the kernel it claims
    eng.load(u0, x0)
    eng.solve_persistent(schedule="index")
    return _snapshot(eng)


def _census(eng):
    torch.cuda.synchronize()
    return set(np.unique(eng.t["phase"].cpu().numpy()).tolist())


def _compare(got, ref, rtol):
    from noc import _lib
    assert np.all(ref["phase"] == _lib.PHASE_DONE)
    for k in COUNTERS:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    err = float(np.max(np.abs(got["u"] - ref["u"])))
    assert np.all(np.isfinite(got["u"])) and err <= rtol * max(1.0, float(np.max(np.abs(ref["u"])))), err


def _equal_counts(a, b):
    return all(np.array_equal(a[k], b[k]) for k in COUNTERS)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resumer", ["one_wave", "wide"])
@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
@pytest.mark.parametrize("name,N,Bt,seed", [("cartpole", 80, 32, 12), ("pendulum", 150, 4, 33)])
def test_launch_per_phase_to_persistent_from_between_step_main_and_promote(name, N, Bt, seed, compact,
                                                                           resumer, monkeypatch):
    """The two-stream driver's sub-steps called directly, stopped between noc_ipm_step_main and
    noc_ipm_promote at the first iteration whose workspace holds ROLLED and ROLLOUT_PENDING rows
    (ipm_schedule.h: resume_phase maps them) next to SOLVE or LINEARIZE ones, then resumed by each
    persistent kernel."""
    from noc import _lib
    from noc.ipm import BatchedIPM
    mode, term = _lib.MODE_PAR, _lib.TERMINAL_STAGE0
    if resumer == "wide":
        # the first of the seeds the wide kernel's own tests use (test_ipm_gpu.py: 33, 5, 4) on
        # which the uninterrupted one-wave and wide solves take the same decisions
        for seed in WIDE_SEEDS:
            ocp, x0, u0 = _problem(name, N, Bt, seed)
            ref1 = _uninterrupted(ocp, N, Bt, x0, u0, "0", monkeypatch, spec="1")
            ref = _uninterrupted(ocp, N, Bt, x0, u0, "1", monkeypatch)
            if _equal_counts(ref, ref1):
                break
        assert _equal_counts(ref, ref1), "every start holds a rounding-level decision"
        rtol = 1e-8
    else:
        ocp, x0, u0 = _problem(name, N, Bt, seed)
        ref, rtol = _uninterrupted(ocp, N, Bt, x0, u0, "0", monkeypatch, spec="1"), 1e-12
    eng = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=False, compact=compact, overlap=False)
    assert eng.compact == compact
    eng.load(u0, x0)
    eng.init(0.1)
    fam, ws, s = ctypes.byref(eng.fam_c), ctypes.byref(eng.ws), eng._stream()
    want = {_lib.PHASE_ROLLED, _lib.PHASE_ROLLOUT_PENDING}
    found = None
    for step in range(400):
        _lib.check(eng._lib.noc_ipm_rollout(fam, ws, s), "noc_ipm_rollout", eng._lib)
        eng._call("step_main", mode, term, s)
        census = _census(eng)
        if want <= census and census & {_lib.PHASE_SOLVE, _lib.PHASE_LINEARIZE}:
            found = step
            break
        _lib.check(eng._lib.noc_ipm_promote(ws, s), "noc_ipm_promote", eng._lib)
    assert found is not None, "no iteration with ROLLED and ROLLOUT_PENDING rows"
    monkeypatch.setenv("NOC_PERSIST_WIDE", "1" if resumer == "wide" else "0")
    monkeypatch.setenv("NOC_PERSIST_SPEC", "1")
    res = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=True)
    for k in BatchedIPM._SHARED_FIELDS:
        res.t[k].copy_(eng.t[k])
    res.solve_persistent(resume=True, schedule="index")
    _compare(_snapshot(res), ref, rtol)


@pytest.mark.parametrize("first,second", [("0", "1"), ("1", "0")], ids=["one_wave_to_wide",
                                                                        "wide_to_one_wave"])
def test_persistent_kernels_hand_over_across_a_cap(first, second, monkeypatch):
    """A solve capped on one persistent kernel and resumed on the other (NOC_PERSIST_WIDE toggled
    between the launches), at the first cap that leaves every trajectory unfinished with SOLVE
    (mid-retry) rows among them."""
    from noc import _lib
    from noc.ipm import BatchedIPM
    name, N, Bt, seed = "pendulum", 150, 4, 33
    ocp, x0, u0 = _problem(name, N, Bt, seed)
    refs = {w: _uninterrupted(ocp, N, Bt, x0, u0, w, monkeypatch) for w in ("0", "1")}
    assert _equal_counts(refs["0"], refs["1"]), "the start must not hold a rounding-level decision"
    for cap in range(4, 40):
        monkeypatch.setenv("NOC_PERSIST_WIDE", first)
        eng = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=True)
        eng.load(u0, x0)
        eng.solve_persistent(max_solves=cap, schedule="index")
        census = _census(eng)
        if _lib.PHASE_SOLVE in census and _lib.PHASE_DONE not in census and len(census) > 1:
            break
    else:
        pytest.fail("no cap leaves SOLVE rows next to other unfinished ones")
    assert np.all(eng.t["kkt_solves"].cpu().numpy() == cap)
    monkeypatch.setenv("NOC_PERSIST_WIDE", second)
    eng.solve_persistent(resume=True, schedule="index")
    _compare(_snapshot(eng), refs[second], 1e-8)


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
@pytest.mark.parametrize("spec", ["1", None], ids=["default_instance", "speculative_instance"])
def test_persistent_to_launch_per_phase(spec, compact, monkeypatch):
    """noc_ipm_step continues what a capped noc_ipm_solve left (BatchedIPM.solve_persistent(
    max_solves=...) followed by BatchedIPM.step): the cap is the first that leaves SOLVE,
    LINEARIZE, ROLLOUT and DONE rows.  The rows at SOLVE carry the hand-off marker (kkt_active =
    0): their blocks are not in the workspace -- it holds the persistent solver's compact records,
    and the speculative instance has written neither reg, pred nor feasible -- so prepare rebuilds
    them (csrc/ipm_schedule.h: blocks_missing).
    Before that rebuild this case failed: the KKT scan read the compact records as dense blocks,
    and every row left at SOLVE (8 of 32 at the cap this picks) finished with other total_it and
    kkt_solves and controls off by up to 0.46, finite; the other rows were right."""
    from noc import _lib
    from noc.ipm import BatchedIPM
    name, N, Bt, seed = "cartpole", 80, 32, 12
    ocp, x0, u0 = _problem(name, N, Bt, seed)
    mode, term = _lib.MODE_PAR, _lib.TERMINAL_STAGE0
    # the reference: the uninterrupted launch-per-phase solve at lanes 64 (the resuming driver)
    loop = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=False, compact=compact, overlap=False)
    loop.load(u0, x0)
    loop.solve(mode=mode)
    ref = _snapshot(loop)
    monkeypatch.setenv("NOC_PERSIST_WIDE", "0")
    if spec is None:
        monkeypatch.delenv("NOC_PERSIST_SPEC", raising=False)
    else:
        monkeypatch.setenv("NOC_PERSIST_SPEC", spec)
    eng = BatchedIPM(ocp.family, N, Bt, lanes=64, persistent=True)
    plan = _lib.ipm_plan(eng._lib, eng.fam_c, N, Bt)
    assert (plan[_lib.PLAN_MAIN + _lib.PLAN_SPEC] > 1) == (spec is None), plan
    want = {_lib.PHASE_SOLVE, _lib.PHASE_LINEARIZE, _lib.PHASE_ROLLOUT, _lib.PHASE_DONE}
    lo = int(ref["kkt_solves"].min())
    for cap in range(lo, lo + 400):
        eng.load(u0, x0)
        eng.t["reg"].fill_(float("nan"))      # what the capped launch does not write stays poison
        eng.t["pred"].fill_(float("nan"))
        eng.t["feasible"].fill_(0)
        eng.solve_persistent(max_solves=cap, schedule="index")
        if _census(eng) == want:
            break
    else:
        pytest.fail("no cap leaves rows at SOLVE, LINEARIZE, ROLLOUT and DONE")
    at_solve = eng.t["phase"] == _lib.PHASE_SOLVE
    assert bool((eng.t["kkt_active"][at_solve] == 0).all())            # the hand-off marker
    eng.compact = compact                      # the workspace's fields are dense-sized: either fits
    for _ in range(400):
        for _ in range(8):
            eng.step(mode, term)
        if eng.all_done():
            break
    _compare(_snapshot(eng), ref, 1e-12)
