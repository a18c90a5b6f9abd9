"""Per-trajectory cost parameters in interior-point DDP and the building blocks on the GPU: a
heterogeneous batch (every trajectory its own goal, wx, wu, wf, u_bound) gives, row for row, bit
for bit what the shared-parameter call gives for that trajectory alone with a Family carrying its
parameters -- on the one-launch kernel (noc_ddp_solve_params), on the nx = 8 building-block loop
and on the blocks themselves; the record follows the trajectory; uniform rows equal the shared
path; and the rows agree with the numpy oracle on their own problems, independently of the
project's kernels."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rows(fam, Bt):
    """all five parameters differ between rows: goal (position component shifted), wx and wf
    (scaled), wu, u_bound -- the rows of tests/test_traj_params_gpu.py::_case"""
    import noc
    b = np.arange(Bt, dtype=np.float64)
    n = fam.nx
    goal = np.tile(np.asarray(list(fam.goal)[:n], dtype=np.float64), (Bt, 1))
    goal[:, 0] += 0.15 * (b - 1.0)
    wx = np.asarray(list(fam.wx)[:n], dtype=np.float64)[None, :] * (0.8 + 0.25 * b)[:, None]
    wf = np.asarray(list(fam.wf)[:n], dtype=np.float64)[None, :] * (1.3 - 0.2 * b)[:, None]
    wu = np.asarray(list(fam.wu)[:fam.nu], dtype=np.float64)[None, :] * (1.0 + 0.5 * b)[:, None]
    ub = fam.u_bound * (0.6 + 0.15 * b)
    params = noc.TrajectoryParams(goal=goal, wx=wx, wu=wu, wf=wf, u_bound=ub)
    solo = [dataclasses.replace(fam, goal=list(goal[i]), wx=list(wx[i]), wu=list(wu[i]),
                                wf=list(wf[i]), u_bound=float(ub[i])) for i in range(Bt)]
    return params, solo


def _case(name, N, Bt):
    """(ocp, x0, u0, TrajectoryParams, per-row solo OCPs)"""
    from noc import problems
    if name == "linear2":   # linear (2, 1) with the control box, so that u_bound is a parameter
        ocp = problems.double_integrators(1, 0.1, constrained=True)
        rng = np.random.default_rng(3)
        x0, u0 = rng.normal(size=(Bt, 2)), 0.1 * rng.normal(size=(Bt, N, 1))
    elif name == "linear8":
        ocp = problems.double_integrators(4, 0.1, constrained=True)
        rng = np.random.default_rng(3)
        x0, u0 = 0.5 * rng.normal(size=(Bt, 8)), 0.1 * rng.normal(size=(Bt, N, 4))
    else:
        ocp = problems.make_problem(name, N)
        x0, u0 = problems.initial_conditions(name, N, Bt, seed=3)
    params, solo = _rows(ocp.family, Bt)
    return ocp, x0, u0, params, [ocp._replace(family=f) for f in solo]


def _solve(ocp, u0, x0, **kw):
    from noc.differential_dynamic_programming import interior_point_ddp
    U, its, info = interior_point_ddp(ocp, u0, x0, return_info=True, **kw)
    return dict(U=U, X=info["states"], its=np.asarray(its), passes=np.asarray(info["passes"]),
                done=np.asarray(info["done"]))


def _assert_rows_equal(batch, solos):
    for i, s in enumerate(solos):
        for k in ("U", "X", "its", "passes", "done"):
            assert np.array_equal(batch[k][i], s[k][0]), (i, k)


def _solos(solo, u0, x0, **kw):
    return [_solve(solo[i], u0[i:i + 1], x0[i:i + 1], **kw) for i in range(len(solo))]


# N = 1: one stage, 63 idle lanes; N = 130: uneven lane chunks (3 / 2 stages)
@pytest.mark.parametrize("name,N,Bt", [("pendulum", 30, 4), ("cartpole", 25, 3), ("linear2", 20, 2),
                                       ("pendulum", 1, 2), ("pendulum", 130, 2)])
def test_heterogeneous_batch_equals_solo_solves_one_launch(name, N, Bt):
    ocp, x0, u0, params, solo = _case(name, N, Bt)
    batch = _solve(ocp, u0, x0, params=params)
    assert batch["done"].all()
    _assert_rows_equal(batch, _solos(solo, u0, x0))
    if N > 1:  # the rows really are different problems
        assert len({batch["U"][i].tobytes() for i in range(Bt)}) == Bt


def test_one_stage_equals_solo_one_stage_calls():
    from noc.differential_dynamic_programming import ddp
    ocp, x0, u0, params, solo = _case("pendulum", 30, 4)
    X, U, its = ddp(ocp, u0, x0, 0.1, params=params)
    for i in range(4):
        Xs, Us, its_s = ddp(solo[i], u0[i:i + 1], x0[i:i + 1], 0.1)
        assert np.array_equal(X[i], Xs[0]) and np.array_equal(U[i], Us[0])
        assert int(its[i]) == int(its_s[0])


def test_uniform_rows_equal_the_shared_path():
    import noc
    ocp, x0, u0, _, _ = _case("cartpole", 25, 3)
    fam = ocp.family
    uniform = noc.TrajectoryParams(goal=np.tile(fam.goal, (3, 1)), wx=fam.wx, wu=fam.wu, wf=fam.wf,
                                   u_bound=np.full(3, fam.u_bound))
    shared, with_params = _solve(ocp, u0, x0), _solve(ocp, u0, x0, params=uniform)
    for k in shared:
        assert np.array_equal(shared[k], with_params[k]), k


def test_record_follows_the_trajectory():
    ocp, x0, u0, params, _ = _case("pendulum", 30, 4)
    fwd = _solve(ocp, u0, x0, params=params)
    reversed_rows = type(params)(**{f.name: np.asarray(getattr(params, f.name))[::-1].copy()
                                    for f in dataclasses.fields(params)})
    rev = _solve(ocp, u0[::-1].copy(), x0[::-1].copy(), params=reversed_rows)
    for k in fwd:
        assert np.array_equal(fwd[k][::-1], rev[k]), k
    assert not np.array_equal(fwd["U"], rev["U"])


def test_max_passes_cap_equals_the_solo_capped_solves():
    ocp, x0, u0, params, solo = _case("pendulum", 30, 4)
    batch = _solve(ocp, u0, x0, params=params, max_passes=7)
    solos = _solos(solo, u0, x0, max_passes=7)
    _assert_rows_equal(batch, solos)
    assert (batch["passes"] == 7).all() and not batch["done"].any()
    assert all(int(s["passes"][0]) == 7 and not s["done"][0] for s in solos)


# ----------------------------------------------------------------------------------- oracle
_ORACLE_BATCH = {}


def _pendulum_oracle_rows():
    """pendulum N = 30, Bt = 4: the rows of tests/test_traj_params_gpu.py::_pendulum_oracle_case"""
    import noc
    from noc import problems
    N, Bt = 30, 4
    ocp = problems.make_problem("pendulum", N)
    fam = ocp.family
    x0, u0 = problems.initial_conditions("pendulum", N, Bt, seed=9)
    b = np.arange(Bt, dtype=np.float64)
    goal = np.tile(np.asarray(fam.goal, dtype=np.float64), (Bt, 1))
    goal[:, 0] += 0.1 * (b - 1.0)
    wx = np.asarray(fam.wx, dtype=np.float64)[None, :] * (0.9 + 0.1 * b)[:, None]
    wf = np.asarray(fam.wf, dtype=np.float64)[None, :] * (1.2 - 0.1 * b)[:, None]
    wu = np.asarray(fam.wu, dtype=np.float64)[None, :] * (1.0 + 0.5 * b)[:, None]
    ub = np.array([4.0, 4.5, 5.5, 6.5])
    params = noc.TrajectoryParams(goal=goal, wx=wx, wu=wu, wf=wf, u_bound=ub)
    return ocp, x0, u0, params, (goal, wx, wu, wf, ub)


def _pendulum_batch_once():
    if "pend" not in _ORACLE_BATCH:
        ocp, x0, u0, params, rows = _pendulum_oracle_rows()
        _ORACLE_BATCH["pend"] = dict(_solve(ocp, u0, x0, params=params), x0=x0, u0=u0, rows=rows)
    return _ORACLE_BATCH["pend"]


@pytest.mark.parametrize("row", [0, 1, 2, 3])
def test_pendulum_rows_match_the_oracle_on_their_own_problem(row):
    """Independent of the project's kernels: row b of the heterogeneous batch against
    oracle.noc_oracle.interior_point_ddp on a TorchOCP built with that row's goal, weights and
    bound (tests/traj_param_problems.py), with the tolerances of
    tests/test_ddp.py::test_ddp_matches_oracle (its docstring gives their reasons): iterations and
    backward passes within one, controls within 1e-5, cost at bp = 0.8e-4 within 1e-9 relative.
    The rows were checked on the CPU oracle before they were fixed: 63 / 63 / 65 / 63 DDP
    iterations and 92 / 93 / 96 / 93 backward passes; per barrier stage at most 15 iterations
    (12-13, 11, 12, 13-14, 15), so no stage is anywhere near its 500-iteration cap; every row's
    control reaches its own bound (max |u| / u_bound > 0.9999; bounds 4, 4.5, 5.5, 6.5); goals
    moved by -0.1 / 0 / +0.1 / +0.2."""
    from oracle import noc_oracle as O
    from traj_param_problems import pendulum_problem
    r = _pendulum_batch_once()
    goal, wx, wu, wf, ub = r["rows"]
    prob = pendulum_problem(1.0 / 30, goal[row], wx[row], wu[row], wf[row], ub[row])
    u0, x0 = r["u0"][row], r["x0"][row]
    Ur, itr, pr = O.interior_point_ddp(prob, u0, x0)
    assert r["done"][row]
    assert abs(int(r["its"][row]) - itr) <= 1, (int(r["its"][row]), itr)
    assert abs(int(r["passes"][row]) - pr) <= 1, (int(r["passes"][row]), pr)
    U = r["U"][row]
    assert np.max(np.abs(U - Ur)) < 1e-5
    c = prob.total_cost(O.rollout(prob.dynamics, U, x0), U, 0.8e-4)
    cr = prob.total_cost(O.rollout(prob.dynamics, Ur, x0), Ur, 0.8e-4)
    assert abs(c - cr) <= 1e-9 * max(1.0, abs(cr))
    assert np.max(np.abs(U)) > 0.999 * ub[row]   # the bound is active at the optimum


# ------------------------------------------------------------------------- nx = 8 host loop
LIN_STEP, LIN_N, LIN_UB = 0.1, 24, (0.8, 2.0, 3.0)


def _linear8_rows():
    """four stacked constrained double integrators (8, 4), N = 24, Bt = 3: per-row u_bound and a
    per-row goal in the position components (the velocity goals stay 0)"""
    import noc
    from noc import problems
    Bt = len(LIN_UB)
    ocp = problems.double_integrators(4, LIN_STEP, constrained=True)
    rng = np.random.default_rng(11)
    x0 = 0.5 * rng.normal(size=(Bt, 8))
    u0 = 0.1 * rng.normal(size=(Bt, LIN_N, 4))
    goal = np.zeros((Bt, 8))
    goal[:, 0::2] = 0.2 * (np.arange(Bt)[:, None] - 1.0) * np.array([1.0, -1.0, 0.5, 2.0])[None, :]
    ub = np.asarray(LIN_UB)
    solo = [ocp._replace(family=dataclasses.replace(ocp.family, goal=list(goal[i]),
                                                    u_bound=float(ub[i]))) for i in range(Bt)]
    return ocp, x0, u0, noc.TrajectoryParams(goal=goal, u_bound=ub), solo, goal


def test_linear8_building_block_loop_equals_solo_and_matches_the_oracle():
    """nx = 8 runs _solve_blocks (no one-launch instance): the batch with per-row u_bound and goal
    equals the solo building-block solves bit for bit, and every row is within the nx = 8 DDP
    tolerance of tests/test_ddp.py::test_ddp_nx8_building_block_loop_matches_oracle (iterations
    within one, controls 1e-5) of the oracle on the row's own oracle.problems.linear_ocp(4, 0.1,
    constrained=True, u_bound=ub_b).  That problem has its goal at the origin; the row's goal g_b
    (positions only, zero velocities) is a fixed point of the double integrators' A (A g = g), so
    tracking g_b from x0 is the origin problem from x0 - g_b with the same controls, which is what
    the oracle solves.  On the CPU oracle: 137 / 88 / 97 DDP iterations (264 / 156 / 174
    backward passes), at most 55 iterations in a barrier stage (row 0 at bp = 0.1), and every
    row's control reaches its bound (max |u| / u_bound > 0.9999)."""
    from oracle import noc_oracle as O, problems as PR
    ocp, x0, u0, params, solo, goal = _linear8_rows()
    batch = _solve(ocp, u0, x0, params=params)
    assert batch["done"].all() and (batch["passes"] >= batch["its"]).all()
    _assert_rows_equal(batch, _solos(solo, u0, x0))
    for b in range(len(LIN_UB)):
        prob = O.NumpyProblem(PR.linear_ocp(4, LIN_STEP, constrained=True, u_bound=LIN_UB[b]))
        Ur, itr, _ = O.interior_point_ddp(prob, u0[b], x0[b] - goal[b])
        assert abs(int(batch["its"][b]) - itr) <= 1, (b, int(batch["its"][b]), itr)
        assert np.max(np.abs(batch["U"][b] - Ur)) < 1e-5, b


# --------------------------------------------------------------------------- building blocks
@pytest.mark.parametrize("name,N,Bt", [("cartpole", 12, 3), ("linear8", 6, 2)])
def test_building_blocks_with_params_equal_the_solo_calls(name, N, Bt):
    import torch
    from noc import differential_dynamic_programming as D
    from noc.costates import final_cost_grad
    from noc.par_interior_point_newton import (check_traj_feasibility, compute_derivatives,
                                               total_cost)
    ocp, x0, u0, params, solo = _case(name, N, Bt)
    X = np.zeros((Bt, N + 1, x0.shape[1]))
    for b in range(Bt):
        X[b, 0] = x0[b]
        for k in range(N):
            X[b, k + 1] = ocp.dynamics(X[b, k], u0[b, k])
    bp = np.array([0.1, 0.02, 1e-3])[:Bt]
    d = compute_derivatives(ocp, X, u0, bp, params=params)
    cost = total_cost(ocp, X, u0, bp, params=params)
    ok = check_traj_feasibility(ocp, X, u0, params=params)
    g, H = final_cost_grad(ocp, X[:, -1], hessian=True, params=params)
    k1, K1, _, _, _ = D.bwd_pass(ocp, X[:, -1], d, 1.0, params=params)
    assert ok.all() and torch.isfinite(cost).all()
    for i in range(Bt):
        sl = slice(i, i + 1)
        ds = compute_derivatives(solo[i], X[sl], u0[sl], bp[sl])
        for f in d._fields:
            assert torch.equal(getattr(d, f)[i], getattr(ds, f)[0]), (i, f)
        assert torch.equal(cost[i], total_cost(solo[i], X[sl], u0[sl], bp[sl])[0]), i
        gs, Hs = final_cost_grad(solo[i], X[sl, -1], hessian=True)
        assert torch.equal(g[i], gs[0]) and torch.equal(H[i], Hs[0]), i
        ks, Ks, _, _, _ = D.bwd_pass(solo[i], X[sl, -1], ds, 1.0)
        assert torch.equal(k1[i], ks[0]) and torch.equal(K1[i], Ks[0]), i
    # the rows are different problems, and differ from the shared-parameter result
    shared = compute_derivatives(ocp, X, u0, bp)
    assert not torch.equal(shared.cx, d.cx) and not torch.equal(shared.cuu, d.cuu)
    # one feasibility row: |u| between row 0's own bound (0.6 of the family's) and the family's
    fam_ub = ocp.family.u_bound
    bad = u0.copy()
    bad[0, N // 2, 0] = -0.8 * fam_ub
    with_rec = check_traj_feasibility(ocp, X, bad, params=params).cpu().numpy()
    without = check_traj_feasibility(ocp, X, bad).cpu().numpy()
    assert not with_rec[0] and with_rec[1:].all() and without.all()
    assert np.array_equal(D.check_feasibility(ocp, X, bad, params=params).cpu().numpy(), with_rec)
    assert np.array_equal(
        check_traj_feasibility(solo[0], X[:1], bad[:1]).cpu().numpy(), with_rec[:1])


def test_building_blocks_refuse_params_on_unbatched_inputs():
    from noc import _lib
    from noc.par_interior_point_newton import total_cost
    ocp, x0, u0, params, _ = _case("cartpole", 12, 3)
    X = np.zeros((13, 4))
    with pytest.raises(_lib.NocError, match="batched"):
        total_cost(ocp, X, u0[0], 0.1, params=params)


# --------------------------------------------------------------------------------- refusal
def test_traced_cost_family_refuses_params():
    import noc
    from noc import _lib
    from noc.differential_dynamic_programming import interior_point_ddp
    import custom_families as CF
    N, B = 30, 2
    ocp = CF.cartpole_track_limit(1.0 / N)
    rng = np.random.default_rng(5)
    x0 = np.array([0.01, -0.01, 0.01, -0.01]) + 0.01 * rng.normal(size=(B, 4))
    u0 = 0.1 * rng.normal(size=(B, N, 1))
    with pytest.raises(_lib.NocError, match="traced"):
        interior_point_ddp(ocp, u0, x0, params=noc.TrajectoryParams(u_bound=np.array([30.0, 40.0])))
