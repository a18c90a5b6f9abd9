"""The interior-point solvers' accept step, restated from the reference in float64, and the table
of planted states that tests/test_ipm_trial_gpu.py feeds to the trial kernel.

accept_step restates one pass of the reference's inner loop body and the loop conditions around
it -- par: noc/par_interior_point_newton.py P:159-202 with the stage finish P:238-245; seq:
noc/seq_interior_point_newton.py S:126-161 with S:186-193 -- on the per-trajectory scalars the
device keeps in its workspace (include/noc_hip.h: noc_ipm_ws), in the style of
oracle/noc_oracle.py (whose _cube it reuses).  It is written from those lines, not from
csrc/ipm_schedule.h.

Every operation in it is ONE correctly rounded IEEE-754 double operation (sub, div, mul, max, min,
ldexp; comparisons), in the order the reference evaluates them.  The device takes the same
operations on the same doubles, so its results must equal these bit for bit: that is the tolerance
of every comparison against this file, derived, not measured.

What the reference does not have and this file adds, with its derivation:
  * retry accounting (rep).  A rejected par trial whose rp was already at the upper clip leaves
    rp unchanged (rp * r_inc >= 2e16 clips back to 1e16, P:173), and the inner loop changes neither
    x, u nor the blocks (P:151-175 closes over them), so the next pass of P:153-175 has the inputs
    of this one and is rejected again -- until inner_it_counter > 500 ends the loop (P:177-182).
    Each such pass is one par_Newton call, inner += 1, r_inc *= 2 and nothing else.  accept_step
    accounts min(room, 501 - inner) of them in one call (room: what the caller's solve cap still
    allows); test_accept_cases.py replays them one by one against that.
  * inner in seq mode: the device counts the KKT solves since the last linearisation there too.
  * reg, the regularisation of the next KKT solve when that is a retry on the same blocks:
    rp * ||cu|| (P:116-118) or mu (S:51).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from oracle.noc_oracle import _cube

PAR, SEQ = 0, 1                                   # NOC_MODE_*
ROLLOUT, LINEARIZE, SOLVE, DONE, ROLLED, ROLLOUT_PENDING = range(6)   # NOC_PHASE_*
ONE_STAGE, RESUME, NO_REPEAT_SKIP = 1, 2, 4       # NOC_WS_*
STATE_FIELDS = ("bp", "rp", "rinc", "cost", "hu", "gnorm", "it", "inner", "total_it", "kkt_solves")
INF, NAN = float("inf"), float("nan")
TINY = 5e-324                                     # the smallest positive subnormal double


def initial_state(bp=0.1):
    """The start of a barrier schedule (P:134-135, P:233 / S:110-111, S:181)."""
    return dict(bp=bp, rp=1.0, rinc=2.0, cost=0.0, hu=1.0, gnorm=0.0, it=0, inner=0, total_it=0,
                kkt_solves=0)


def accept_step(state, mode, new_cost, pred, bwd_ok, flags=0, room=501):
    """One accept test on `state` (a dict of STATE_FIELDS; cost, hu, gnorm are those of the
    iteration's linearisation).  new_cost: the trial's total cost, inf when infeasible (P:159-163 /
    S:127-129); pred, bwd_ok: the KKT solve's predicted reduction and backward feasibility.
    Returns (new state, outcome): outcome["take"]: x <- x + dx, u <- u + du; ["phase"]: where the
    solve continues (ROLLOUT: the next barrier stage, LINEARIZE: a new Newton iteration, SOLVE: a
    retry on the same blocks, DONE); ["reg"]: the regularisation to store for a SOLVE retry, else
    None; ["rep"]: identical retries accounted without a solve; plus gain, success, branch."""
    s = dict(state)
    f = np.float64
    with np.errstate(all="ignore"):
        gain = float((f(new_cost) - f(s["cost"])) / f(pred))            # P:164-165 / S:133-134
    success = bool(gain > 0.0) and bool(bwd_ok)                         # P:166 / S:137
    rp_used = s["rp"]
    if success:
        shrink = max(1.0 / 3.0, 1.0 - _cube(2.0 * gain - 1.0))          # P:169 / S:141
        s["rp"] = s["rp"] * shrink
        s["rinc"] = 2.0                                                 # P:172 / S:144
    else:
        s["rp"] = s["rp"] * s["rinc"]                                   # P:170 / S:142
        s["rinc"] = 2 * s["rinc"]
    s["inner"] += 1                                                     # P:174
    s["kkt_solves"] += 1
    rep = 0
    if mode == PAR:
        s["rp"] = min(max(s["rp"], 1e-16), 1e16)                        # P:173
        if (not success and not (flags & NO_REPEAT_SKIP) and s["rp"] == rp_used
                and not s["inner"] > 500):
            rep = max(0, min(room, 501 - s["inner"]))                   # see the module docstring
            s["inner"] += rep
            s["kkt_solves"] += rep
            with np.errstate(all="ignore"):
                s["rinc"] = float(np.ldexp(f(s["rinc"]), rep))          # r_inc doubles per pass
        end_iter = success or s["inner"] > 500                          # P:177-182
        take = end_iter                                                 # P:184: the last trial
        if end_iter:
            s["it"] += 1                                                # P:194
        stage_done = end_iter and (s["hu"] < 1e-4 or s["it"] > 1000)    # P:199-202
        relinearize = end_iter
    else:
        take = success                                                  # S:145-146
        end_iter = True
        s["it"] += 1                                                    # S:152
        stage_done = s["hu"] < 1e-4 and bool(bwd_ok)                    # S:157-161
        relinearize = success      # a rejected step leaves x, u -- and so the blocks -- unchanged
    if stage_done:
        s["total_it"] += s["it"]                                        # P:239 / S:187
        s["bp"] = s["bp"] / 5                                           # P:238 / S:186
        s["it"] = 0
        s["rp"], s["rinc"] = 1.0, 2.0                                   # P:134-135 / S:110-111
        more = s["bp"] > 1e-4 and not (flags & ONE_STAGE)               # P:243-245 / S:191-193
        phase = ROLLOUT if more else DONE
    else:
        phase = LINEARIZE if relinearize else SOLVE
    reg = None
    if phase == SOLVE:
        reg = s["rp"] * s["gnorm"] if mode == PAR else s["rp"]          # P:116-118 / S:51
    if stage_done:
        branch = "stage_next" if phase == ROLLOUT else "stage_last"
    elif mode == PAR and end_iter and not success:
        branch = "cap_keep"
    else:
        branch = ("accept" if success else "reject") + ("" if rep == 0 else "_rep")
    return s, dict(take=take, phase=phase, reg=reg, rep=rep, gain=gain, success=success,
                   branch=branch)


# ------------------------------------------------------------------------------------------------
# the predicate of tools/rp_trace_check.py: a fused 1 - c * (c * c) rounds once
def shrink_two_roundings(g):
    c = 2.0 * g - 1.0
    return max(1.0 / 3.0, 1.0 - c * (c * c))


def shrink_fused(g):
    c = 2.0 * g - 1.0
    t = c * c
    return max(1.0 / 3.0, float(Fraction(1) - Fraction(t) * Fraction(c)))


def fused_would_differ(g):
    return shrink_fused(g) != shrink_two_roundings(g)


# Gains at which a fused multiply-subtract in the shrink factor would round differently
# (test_accept_cases.py checks the predicate on each, and that the factor is not the 1/3 floor,
# where the difference would not show): found by scanning k / 401
FUSED_GAINS = (3 / 401.0, 28 / 401.0, 73 / 401.0, 154 / 401.0, 282 / 401.0, 314 / 401.0)

# ------------------------------------------------------------------------------------------------
# The planted table.  One row = one batch row of a trial-kernel launch: the workspace scalars, the
# KKT outputs pred / feasible, and the trial point as a recipe whose total cost is EXACT in any
# summation order:
#   trial "zero": every stage cost and the final cost 0      -> new_cost 0
#         "one":  one stage cost 1.0, the rest 0             -> new_cost 1
#         "infeasible": one control at u + du = 2 > u_bound  -> new_cost inf
# (tests/test_ipm_trial_gpu.py: wx_0 = 2 and one e_0 = 1 give 0.5 * (2 * 1 * 1) = 1; u + du = 0
# with u_bound = 1 gives -bp * (log 1 + log 1) = 0.)  So gain = (new_cost - cost) / pred is two
# exact-input IEEE operations on the planted cost and pred.
# modes: which of "par", "seq" the row runs in; want: {mode: branch accept_step must take}.
HU_LO, HU_HI = float(np.nextafter(1e-4, 0.0)), float(np.nextafter(1e-4, 1.0))
BP_CHAIN = [0.1]
while BP_CHAIN[-1] > 1e-4:
    BP_CHAIN.append(BP_CHAIN[-1] / 5)          # 0.1, 0.02, ..., the last one <= 1e-4


def _bp_hitting_1e4():
    """A double whose correctly rounded quotient by 5 is exactly the double 1e-4, with its two
    neighbours (their quotients fall on either side or on it; the restatement says which)."""
    b = 1e-4 * 5
    for cand in (b, float(np.nextafter(b, 0.0)), float(np.nextafter(b, 1.0))):
        if cand / 5 == 1e-4:
            return cand
    raise AssertionError("no double with bp / 5 == 1e-4 next to 5e-4")


BP_EXACT = _bp_hitting_1e4()


def _row(name, want, modes=("par", "seq"), trial="zero", pred=-1.0, feasible=1, phase=SOLVE, **st):
    state = dict(bp=0.1, rp=1.0, rinc=2.0, cost=0.5, hu=1.0, gnorm=3.0, it=7, inner=2,
                 total_it=40, kkt_solves=90)
    state.update(st)
    if isinstance(want, str):
        want = {m: want for m in modes}
    return dict(name=name, state=state, pred=pred, feasible=feasible, trial=trial, phase=phase,
                modes=tuple(modes), want=want)


def planted_rows():
    R = []
    both = lambda a, b: dict(par=a, seq=b)
    # ---- gain values: gain = (0 - cost) / -1 = cost unless said otherwise
    R.append(_row("gain+0", "reject", cost=0.0, pred=1.0))             # (0 - 0) / 1 = +0
    R.append(_row("gain-0", "reject", cost=0.0, pred=-1.0))            # (0 - 0) / -1 = -0
    R.append(_row("gain_subnormal", "accept", cost=TINY))
    R.append(_row("gain_negative", "reject", cost=-0.75))
    R.append(_row("gain_half", "accept", cost=0.5))                    # shrink 1
    R.append(_row("gain_one", "accept", cost=1.0))                     # shrink 1/3
    R.append(_row("gain_two", "accept", cost=2.0))                     # 1 - 27 < 1/3
    for i, g in enumerate(FUSED_GAINS):
        R.append(_row(f"gain_fused{i}", "accept", cost=g, rp=2.0 ** (i - 2)))  # keeps the last bit
    R.append(_row("gain_one_from_trial_one", "accept", trial="one", cost=2.0))  # (1 - 2) / -1
    R.append(_row("gain+inf", "accept", cost=-1.0, pred=0.0))          # 1 / +0
    R.append(_row("gain-inf", "reject", cost=-1.0, pred=-0.0))         # 1 / -0
    R.append(_row("gain_nan_0/0", "reject", cost=0.0, pred=0.0))
    R.append(_row("gain_nan_inf-inf", "reject", cost=INF, trial="infeasible"))
    R.append(_row("gain-inf_infeasible", "reject", cost=1.0, trial="infeasible"))
    R.append(_row("gain_nan_pred", "reject", pred=NAN))
    # ---- backward feasibility
    R.append(_row("bwd_infeasible", "reject", feasible=0))
    R.append(_row("bwd_infeasible_small_hu", both("reject", "reject"), feasible=0, hu=HU_LO))
    # ---- rp clips (par clips, seq does not)
    for inner in (0, 250, 499, 500):
        R.append(_row(f"clip_hi_inner{inner}", both("cap_keep", "reject"), cost=-1.0, rp=1e16,
                      inner=inner))
    R.append(_row("clip_hi_rinc_overflow", both("cap_keep", "reject"), cost=-1.0, rp=1e16,
                  rinc=2.0 ** 1000, inner=3))
    R.append(_row("clip_hi_rinc_inf", both("cap_keep", "reject"), cost=-1.0, rp=1e16, rinc=INF,
                  inner=3))
    R.append(_row("clip_hi_from_below", "reject", cost=-1.0,
                  rp=float(np.nextafter(1e16, 0.0)), rinc=4.0))        # clips to 1e16 != rp_used
    R.append(_row("clip_hi_infeasible_kept", both("cap_keep", "reject"), cost=1.0,
                  trial="infeasible", rp=1e16, inner=10))
    R.append(_row("clip_lo", "accept", cost=1.0, rp=1e-16))            # 1e-16 / 3 clips back (par)
    R.append(_row("clip_lo_rejected", "reject", cost=-1.0, rp=1e-16))
    # ---- the retry cap (par): inner becomes 500 (another retry) and 501 (the trial is kept)
    R.append(_row("cap_inner_to_500", "reject", modes=("par",), cost=-1.0, rp=8.0, inner=499))
    R.append(_row("cap_inner_to_501", "cap_keep", modes=("par",), cost=-1.0, rp=8.0, inner=500))
    R.append(_row("cap_keeps_infeasible", "cap_keep", modes=("par",), cost=1.0,
                  trial="infeasible", rp=8.0, inner=500))
    R.append(_row("cap_keep_ends_stage", "stage_next", modes=("par",), cost=-1.0, rp=8.0,
                  inner=500, hu=HU_LO))
    # ---- the stop test
    R.append(_row("stop_hu_below", "stage_next", hu=HU_LO))
    R.append(_row("stop_hu_at", "accept", hu=1e-4))
    R.append(_row("stop_hu_above", "accept", hu=HU_HI))
    R.append(_row("stop_hu_nan", "accept", hu=NAN))
    R.append(_row("stop_hu_below_rejected", both("reject", "stage_next"), hu=HU_LO, cost=-1.0))
    R.append(_row("stop_it_999", "accept", it=999))
    R.append(_row("stop_it_1000", both("stage_next", "accept"), it=1000))
    R.append(_row("stop_it_1000_rejected", "reject", it=1000, cost=-1.0))
    # ---- the stage finish along the barrier chain, and around bp / 5 == 1e-4
    for i, bp in enumerate(BP_CHAIN[:-1]):
        last = not (BP_CHAIN[i + 1] > 1e-4)
        R.append(_row(f"stage_bp{i}", "stage_last" if last else "stage_next", bp=bp, hu=HU_LO,
                      it=3 + i, rp=0.125, rinc=16.0))
    for nm, bp in (("exact", BP_EXACT), ("below", float(np.nextafter(BP_EXACT, 0.0))),
                   ("above", float(np.nextafter(BP_EXACT, 1.0)))):
        R.append(_row(f"stage_bp_{nm}", "stage_next" if bp / 5 > 1e-4 else "stage_last", bp=bp,
                      hu=HU_LO))
    # ---- rows that are not at SOLVE: nothing may change
    for nm, ph in (("rollout", ROLLOUT), ("linearize", LINEARIZE), ("done", DONE),
                   ("rolled", ROLLED), ("rollout_pending", ROLLOUT_PENDING)):
        R.append(_row(f"phase_{nm}", "untouched", phase=ph, hu=HU_LO))
    return R


def trial_cost(trial):
    """The exact total cost of a planted trial point (inf: infeasible)."""
    return {"zero": 0.0, "one": 1.0, "infeasible": INF}[trial]


def expected(row, mode, flags=0, room=501):
    """(new state, outcome) of a planted row, or (state, None) for a row that is not at SOLVE."""
    if row["phase"] != SOLVE:
        return dict(row["state"]), None
    return accept_step(row["state"], mode, trial_cost(row["trial"]), row["pred"],
                       row["feasible"] != 0, flags, room)
