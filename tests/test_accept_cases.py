"""CPU checks of tests/accept_cases.py: the restated accept step reproduces the oracle's own
loops (oracle/noc_oracle.py, written as loops from the same reference lines) decision for
decision, its retry accounting equals the retries replayed one by one, and the planted table of
tests/test_ipm_trial_gpu.py meets its own preconditions."""
import math
from fractions import Fraction

import numpy as np
import pytest

import accept_cases as AC


def _problem(name, N):
    from oracle import problems as PR, noc_oracle as O
    from noc import problems
    make = PR.pendulum_ocp if name == "pendulum" else PR.cartpole_ocp
    x0, u0 = problems.initial_conditions(name, N, 1, seed=5)
    return O.NumpyProblem(make(1.0 / N)), x0[0], u0[0]


def _replay(trace, mode):
    """Feed the records of one oracle solve through accept_step; returns the final state."""
    s = AC.initial_state(0.1)
    stage_ends = 0
    for i, r in enumerate(trace):
        assert s["bp"] == r["bp"] and s["it"] == r["it"], (i, s, r)
        s = dict(s, cost=r["cost"], hu=r["hu"])
        s, o = AC.accept_step(s, mode, r["new_cost"], r["pred"], r["feas"])
        assert o["success"] == r["success"], (i, o, r)
        ends = i + 1 == len(trace) or trace[i + 1]["bp"] != r["bp"]
        assert (o["phase"] in (AC.ROLLOUT, AC.DONE)) == ends, (i, o, r)
        assert (o["phase"] == AC.DONE) == (i + 1 == len(trace)), (i, o)
        if ends:
            stage_ends += 1
            assert s["rp"] == 1.0 and s["rinc"] == 2.0 and s["it"] == 0
        else:
            # the regularisation and its increment, bit for bit (== on floats)
            assert s["rp"] == r["rp"] and s["rinc"] == r["rinc"], (i, s, r)
            assert o["rep"] == 0 or mode == AC.PAR
        if mode == AC.PAR:
            # the oracle's inner counts this iteration's passes so far; accounted repeats are
            # the oracle's following (identical) records
            assert s["inner"] - o["rep"] == r["inner"], (i, s, r)
            assert o["take"] == (o["phase"] != AC.SOLVE)
        else:
            assert o["take"] == r["success"]
        if o["phase"] != AC.SOLVE:
            s["inner"] = 0          # the next linearisation starts a new retry count
    return s, stage_ends


@pytest.mark.parametrize("name,N", [("pendulum", 12), ("cartpole", 10)])
def test_restatement_reproduces_the_par_oracle_trace(name, N):
    from oracle import noc_oracle as O
    prob, x0, u0 = _problem(name, N)
    trace = []
    _, total, solves = O.par_interior_point_optimal_control(prob, u0, x0, terminal="stage0",
                                                            trace=trace)
    assert len(trace) == solves and any(not r["success"] for r in trace)
    # no run of identical retries at the clip in these solves: one record per accept_step call
    assert all(r["rp"] < 1e16 for r in trace)
    s, ends = _replay(trace, AC.PAR)
    assert ends == len(AC.BP_CHAIN) - 1
    assert s["total_it"] == total and s["kkt_solves"] == solves
    assert s["bp"] == AC.BP_CHAIN[-1]


@pytest.mark.parametrize("name,N", [("pendulum", 12), ("cartpole", 10)])
def test_restatement_reproduces_the_seq_oracle_trace(name, N):
    from oracle import noc_oracle as O
    prob, x0, u0 = _problem(name, N)
    trace = []
    _, total = O.seq_interior_point_optimal_control(prob, u0, x0, trace=trace)
    assert len(trace) == total and any(not r["success"] for r in trace)
    s, ends = _replay(trace, AC.SEQ)
    assert ends == len(AC.BP_CHAIN) - 1
    assert s["total_it"] == total and s["kkt_solves"] == total
    assert s["bp"] == AC.BP_CHAIN[-1]


@pytest.mark.parametrize("inner0", [0, 1, 250, 499, 500])
@pytest.mark.parametrize("rinc0", [2.0, 2.0 ** 600])
def test_retry_accounting_equals_the_retries_one_by_one(inner0, rinc0):
    """A run of identical rejected retries at rp = 1e16 (P:151-188), one accept test per retry
    (NO_REPEAT_SKIP), against calls that account them, with `room` smaller than, equal to and
    larger than the retries that remain."""
    start = dict(AC.initial_state(0.004), rp=1e16, rinc=rinc0, cost=-1.0, hu=0.5, gnorm=2.0, it=4,
                 inner=inner0, total_it=9, kkt_solves=77)
    one = [start]
    while True:                                       # the reference's loop, pass by pass
        s, o = AC.accept_step(one[-1], AC.PAR, 0.0, -1.0, True, flags=AC.NO_REPEAT_SKIP)
        assert o["rep"] == 0 and not o["success"]
        one.append(s)
        if o["phase"] != AC.SOLVE:
            assert o["take"] and o["phase"] == AC.LINEARIZE and s["inner"] == 501
            break
    passes = len(one) - 1
    assert passes == 501 - inner0
    remaining = passes - 1                            # after the first, computed pass
    for room in sorted({0, 1, remaining - 1, remaining, remaining + 1, 501} - {-1}):
        s, o = AC.accept_step(start, AC.PAR, 0.0, -1.0, True, room=room)
        k = 1 + min(room, remaining)
        assert o["rep"] == k - 1
        assert s == one[k], (room, s, one[k])
        assert (o["phase"] == AC.LINEARIZE) == (k == passes) and o["take"] == (k == passes)
        # ... and a later call continues the run where the cap cut it
        while o["phase"] == AC.SOLVE:
            s, o = AC.accept_step(s, AC.PAR, 0.0, -1.0, True)
        assert s == one[-1]


def test_planted_rows_take_their_intended_branch():
    rows = AC.planted_rows()
    assert len(rows) % 4 != 0                        # the last block of the launch is partial
    assert len({r["name"] for r in rows}) == len(rows)
    seen = set()
    for r in rows:
        for m in r["modes"]:
            mode = AC.PAR if m == "par" else AC.SEQ
            _, o = AC.expected(r, mode)
            got = o["branch"] if o else "untouched"
            want = r["want"][m]
            if want == "cap_keep" and o["rep"] == 0:
                assert r["state"]["inner"] == 500
            assert got == want, (r["name"], m, got, want)
            seen.add((m, got))
            if r["name"].startswith("clip_hi_inner") and m == "par":
                _, o2 = AC.expected(r, mode, flags=AC.NO_REPEAT_SKIP)
                assert o2["rep"] == 0
                assert o2["branch"] == ("cap_keep" if r["state"]["inner"] == 500 else "reject")
                assert o["rep"] == 500 - r["state"]["inner"]
            if got == "stage_next":
                _, o1 = AC.expected(r, mode, flags=AC.ONE_STAGE)
                assert o1["phase"] == AC.DONE
    for m in ("par", "seq"):
        for b in ("accept", "reject", "stage_next", "stage_last", "untouched"):
            assert (m, b) in seen, (m, b)
    assert ("par", "cap_keep") in seen
    by = {r["name"]: r for r in rows}
    # named preconditions of single rows
    g = lambda n, m=AC.PAR: AC.expected(by[n], m)
    assert math.copysign(1.0, g("gain+0")[1]["gain"]) == 1.0 and g("gain+0")[1]["gain"] == 0.0
    assert math.copysign(1.0, g("gain-0")[1]["gain"]) == -1.0 and g("gain-0")[1]["gain"] == 0.0
    assert g("gain_subnormal")[1]["gain"] == AC.TINY
    assert g("gain+inf")[1]["gain"] == AC.INF and g("gain-inf")[1]["gain"] == -AC.INF
    assert g("gain-inf_infeasible")[1]["gain"] == -AC.INF
    for n in ("gain_nan_0/0", "gain_nan_inf-inf", "gain_nan_pred"):
        assert math.isnan(g(n)[1]["gain"])
    assert g("clip_lo")[0]["rp"] == 1e-16 and g("clip_lo", AC.SEQ)[0]["rp"] < 1e-16
    assert g("clip_hi_from_below")[0]["rp"] == 1e16 and g("clip_hi_from_below")[1]["rep"] == 0
    assert g("clip_hi_rinc_overflow")[0]["rinc"] == AC.INF
    assert g("cap_keeps_infeasible")[1]["take"] and g("clip_hi_infeasible_kept")[1]["take"]
    assert g("cap_inner_to_500")[0]["inner"] == 500 and g("cap_inner_to_501")[0]["inner"] == 501
    assert not g("bwd_infeasible_small_hu", AC.SEQ)[1]["take"]
    assert g("bwd_infeasible_small_hu", AC.SEQ)[1]["phase"] == AC.SOLVE
    assert AC.BP_EXACT / 5 == 1e-4 and g("stage_bp_exact")[1]["phase"] == AC.DONE
    assert {g(f"stage_bp_{n}")[1]["phase"] for n in ("below", "exact", "above")} == {AC.DONE,
                                                                                     AC.ROLLOUT}
    assert AC.HU_LO < 1e-4 < AC.HU_HI


def test_planted_gains_include_fused_would_differ_values():
    """The shrink factor of these rows differs in the last bit between 1 - c * (c * c) with two
    roundings (the reference) and with a fused multiply-subtract, above the 1/3 floor -- and the
    planted rp carries that bit into the stored rp."""
    by = {r["name"]: r for r in AC.planted_rows()}
    for i, gain in enumerate(AC.FUSED_GAINS):
        assert AC.fused_would_differ(gain) and AC.shrink_two_roundings(gain) > 1.0 / 3.0
        r = by[f"gain_fused{i}"]
        for mode in (AC.PAR, AC.SEQ):
            s, o = AC.expected(r, mode)
            assert o["gain"] == gain and o["success"]
            assert s["rp"] == r["state"]["rp"] * AC.shrink_two_roundings(gain)
            assert s["rp"] != r["state"]["rp"] * AC.shrink_fused(gain)


def test_planted_trial_costs_are_exact_in_any_order():
    """The recipes of tests/test_ipm_trial_gpu.py: stage costs 0.5 * (wx e e) with wx = 2 and e in
    {0, 1}, controls at 0 inside a bound of 1.  Every term is a dyadic rational with a one-bit
    mantissa, at most one of them non-zero, so every partial sum in every order -- and with or
    without fused multiply-adds -- is exact; checked here in exact rational arithmetic."""
    for e in (0.0, 1.0):
        term = Fraction(1, 2) * (Fraction(2) * Fraction(e) * Fraction(e))
        assert term == Fraction(0.5 * (2.0 * e * e)) and term in (0, 1)
    assert math.log(1.0 - 0.0) + math.log(0.0 + 1.0) == 0.0       # the barrier term at u = 0
    for trial, total in (("zero", 0), ("one", 1)):
        terms = [Fraction(0)] * 131 + ([Fraction(1)] if trial == "one" else [])
        assert sum(terms) == total == Fraction(AC.trial_cost(trial))
        # any partial sum of these terms is 0 or 1: representable, so no order rounds
        assert set(np.cumsum([float(t) for t in terms[::-1]])) <= {0.0, 1.0}
    assert AC.trial_cost("infeasible") == AC.INF
    # every planted cost and pred is a double by construction; the gain is then two IEEE operations
    for r in AC.planted_rows():
        assert isinstance(r["state"]["cost"], float) and isinstance(r["pred"], float)
