"""CPU: the high-precision reference of the first DDP passes (tests/ddp_pass_cases.py) and its cases
are fit to hold the one-launch kernel to (tests/test_ddp_passes_gpu.py does that on the device).

  * the fp64 oracle (oracle.noc_oracle.ddp with its trace, stopped after K passes; its trials are
    those of ddp_nonlin_rollout) agrees with the reference to ORACLE_ERR[k], and the table equals
    the measurement to a factor of two, so neither can drift;
  * every decision of every case has a margin no fp64 implementation can cross;
  * the census of what the cases exercise is pinned;
  * deliberate defects of the size the GPU test is meant to catch move the reference far beyond
    the GPU bound.

Finite-gain rejections.  No further seeds had to be searched for a pass rejected at a finite gain
<= -0.05: the cases hold one (pendulum-twin-row2: gains -0.19 and -2.1 before its accept, so the
retry arithmetic is also run where new_cost is a number), and test_census pins it.  Two more
occurred at seeds that were replaced for their conditioning (ddp_pass_cases._BUMP).
"""
import math

import numpy as np
import pytest

import ddp_pass_cases as C
import family_cases as F

ALL = C.CASES + C.TWIN_CASES + (C.TRACED_CASE,)
BUILTIN = C.CASES + C.TWIN_CASES


# --------------------------------------------------------------------------------------------------
# the fp64 oracle, stopped after K passes
# --------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


class _Trace(list):
    def __init__(self, cap):
        super().__init__()
        self.cap = cap

    def append(self, d):
        super().append(d)
        if len(self) >= self.cap:
            raise _Stop


def torch_problem(case):
    """the torch restatement of the case's own problem (oracle/problems.py, torch.func autodiff)"""
    from oracle import problems as PR
    import traj_param_problems as TP
    if case.traced:
        import custom_families as CF
        return CF.cartpole_track_limit_torch(1.0 / case.N)
    base = {"pendulum": lambda: PR.pendulum_ocp(1.0 / case.N),
            "cartpole": lambda: PR.cartpole_ocp(1.0 / case.N),
            "linear2": lambda: PR.linear_ocp(1, F.LINEAR_STEP, constrained=True)}[case.name]()
    if case.row < 0:
        return base
    r = C.case_row(case)
    wrap = {"pendulum": 0, "cartpole": 1, "linear2": -1}[case.name]
    return TP._param_ocp(base, wrap, r["goal"], r["wx"], r["wu"], r["wf"], r["u_bound"])


_ORACLE = {}


def oracle_passes(case):
    """per-pass dicts of the fp64 oracle, in the reference's keys"""
    if case.id not in _ORACLE:
        from oracle import noc_oracle as O

        class Recorder(O.NumpyProblem):
            """keeps every trial ddp hands to the feasibility test (ddp_nonlin_rollout's output)"""
            def feasible(self, X, U):
                self.trials.append((X.copy(), U.copy()))
                return super().feasible(X, U)

        prob = Recorder(torch_problem(case))
        prob.trials = []
        trace = _Trace(C.K)
        x0, u0 = C.start(case)
        with pytest.raises(_Stop):
            O.ddp(prob, u0, x0, case.bp, trace=trace)
        _ORACLE[case.id] = [dict(t, TX=X, TU=U) for t, (X, U) in zip(trace, prob.trials)]
    return _ORACLE[case.id]


# --------------------------------------------------------------------------------------------------
def test_oracle_error_table():
    """ORACLE_ERR[k] is the fp64 oracle's largest own-maximum error after k passes over every case,
    every compared scalar and both trial arrays; the decisions agree exactly."""
    worst = {k: (0.0, None) for k in range(1, C.K + 1)}
    for case in ALL:
        ref, got = C.case_passes(case), oracle_passes(case)
        assert len(got) == C.K
        for k in range(1, C.K + 1):
            r, g = ref[k - 1], got[k - 1]
            assert (g["it"], g["inner"], bool(g["success"])) == (r["it"], r["inner"], r["success"]), \
                (case.id, k)
            for f, e in C.errors(g, r).items():
                assert math.isfinite(e), (case.id, k, f)
                if e > worst[k][0]:
                    worst[k] = (e, (case.id, f))
    print("measured oracle error:", worst)
    for k, (e, where) in worst.items():
        assert e <= C.ORACLE_ERR[k] <= 2.0 * e, (k, e, where, C.ORACLE_ERR[k])
        assert C.gpu_bound(k) <= 1e-9, (k, C.gpu_bound(k))   # else the cases are too ill-conditioned


def _kind(p):
    if p["success"]:
        return "accept"
    return "box" if p["new_cost"] == math.inf else "reject"


@pytest.mark.parametrize("case", ALL, ids=str)
def test_decision_margins(case):
    """Conditions, not measurements.  Every decision is an accept with gain >= 0.05 on a backward
    pass whose Quu pivots all exceed 1e-6 |Quu|, or a trial outside the box (new_cost = inf), or
    a rejection with finite gain <= -0.05; a trial control is never within 1e-9 u_bound of the box's
    faces (the feasibility comparison is then the same in fp64); nothing is clipped or capped.
    Conditioning: a finite trial cost differs from the nominal cost by at least 1e-3 of it (else
    gain = (new_cost - cost) / pred is a quotient of rounding errors and every later pass inherits
    it through rp), and |Hu| stays above 1e-2, two orders from the stopping test."""
    for k, p in enumerate(C.case_passes(case), 1):
        where = (case.id, k)
        assert not p["clipped"] and not p["retry_cap"], where
        assert p["box"] > 1e-9, (where, p["box"])
        assert abs(p["pivot"]) > 1e-6, (where, p["pivot"])
        if p["success"]:
            assert p["gain"] >= 0.05 and p["pivot"] > 1e-6 and p["feas"], (where, p["gain"])
        elif math.isfinite(p["new_cost"]):
            assert p["gain"] <= -0.05 and p["feas"], (where, p["gain"])
        else:
            assert p["new_cost"] == math.inf and p["gain"] in (math.inf, -math.inf), where
        assert not -0.05 < p["gain"] < 0.05, (where, p["gain"])
        if math.isfinite(p["new_cost"]):   # gain's numerator keeps at least 13 of its 16 digits
            assert abs(p["new_cost"] - p["cost"]) >= 1e-3 * abs(p["cost"]), where
        assert p["hu"] > 1e-2, where    # far from the |Hu| < 1e-4 stopping test


def test_census():
    """What the built-in cases exercise, pinned."""
    kinds = {c.id: [_kind(p) for p in C.case_passes(c)] for c in BUILTIN}
    print({k: "".join(x[0] for x in v) for k, v in kinds.items()})
    first_accept = [i for i, v in kinds.items() if v[0] == "accept"]
    first_box = [i for i, v in kinds.items() if v[0] == "box"]
    retry = [c.id for c in BUILTIN for a, b in zip(C.case_passes(c), C.case_passes(c)[1:])
             if not a["success"] and b["success"] and a["it"] == b["it"]]
    double = [c.id for c in BUILTIN for a, b in zip(C.case_passes(c), C.case_passes(c)[1:])
              if a["success"] and b["success"]]
    finite_reject = [i for i, v in kinds.items() if "reject" in v]
    assert len(first_accept) >= 3, first_accept
    assert len(first_box) >= 3, first_box
    assert len(set(retry)) >= 2, retry       # r_inc doubled, the multiplier stayed the outer reg_inc
    assert len(set(double)) >= 2, double     # pass 2 on re-evaluated derivatives, swapped buffers
    assert sorted(finite_reject) == sorted(C.FINITE_REJECT_CASES), finite_reject
    # every family appears among the accepted first passes or the retries
    assert {i.split("-")[0] for i in first_accept + retry} == set(F.NAMES)


# --------------------------------------------------------------------------------------------------
POWER = "cartpole-twin-row0"


def test_power_of_the_bound():
    """One cart-pole case, pass 1: dropping Vx . fxx from the backward pass, or changing the pole
    length by 1e-9, moves the trial controls by more than ten times the GPU bound; leaving the last
    stage of lane 0's chunk (stage 1 of N = 65: lane 0 holds stages 0, 1) out of the nominal cost
    moves `cost` by more than that too.  The case is the cart-pole twin's row 0 (N = 65, controls
    at 0.3 u_bound, so that the step is a visible share of the trial controls): 1.8e-3, 8.5e-10 and
    1.6e-2 against 2.5e-10.  On the four other cart-pole N = 65 cases the three figures are 2.1e-8
    to 2.2e-4, 3.3e-12 to 2.3e-10 and 5.4e-3 to 1.7e-2: where the start controls fill 0.9 or more
    of the box, a 2e-9 relative change of one constant moves the controls by up to nine bounds, not
    ten -- the dropped term and the short sum stay three orders or more beyond it everywhere."""
    case = C.BY_ID[POWER]
    ref = C.case_passes(case)[0]
    bound = 10.0 * C.gpu_bound(1)
    no_fxx = C.case_passes(case, zero=("fxx",))[0]
    longer = C.case_passes(case, constants={"pole_length": 0.5 + 1e-9})[0]
    short = C.case_passes(case, skip_stage=1)[0]
    moved = {"fxx": F.own_max_error(no_fxx["TU"], ref["TU"]),
             "pole_length": F.own_max_error(longer["TU"], ref["TU"]),
             "cost": F.own_max_error(short["cost"], ref["cost"])}
    print("power:", moved, "ten times the bound:", bound)
    for k, v in moved.items():
        assert v > bound, (k, v, bound)
