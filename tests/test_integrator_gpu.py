"""Families registered with integrator="rk4" (tests/integrator_families.py: cart-pole (4, 1),
actuated pendulum (3, 1), vectored cart-pole (4, 2), dt = 0.05) through every consumer of the
family device code: noc_derivatives, noc_nonlin_rollout, the fused linearise, whole interior-point
solves (launch-per-phase, persistent one-wave and wide) and interior-point DDP.

The reference is the torch restatement with oracle.problems.discretize_dynamics(ode, dt, 1) under
torch.func and the numpy loops of oracle/noc_oracle.py.  tests/test_integrator_cases.py holds the
preconditions on the CPU: the RK4 and the Euler reference differ at every point by far more than
any tolerance below, and every whole-solve start keeps a 1e-6 margin at every oracle decision.

Tolerances are the project's own: 1e-10 for derivatives and blocks (tests/test_ipm_gpu.py), 1e-12
for states (tests/test_golden_gpu.py), controls of a whole solve within 1e-6 of the oracle's with
identical counts (tests/test_multi_control_gpu.py), the wide kernel within 1e-8 of the one-wave
kernel (tests/test_ipm_gpu.py), DDP as tests/test_ddp.py; the persistent solve against the
launch-per-phase loop and NOC_PERSIST_STRUCT=0 against the default bit for bit (include/noc_hip.h:
noc_ipm_solve).

An RK4 family's library compiles the KKT scan at the library's -ffp-contract=on
(NOC_SCAN_CONTRACT_ON, csrc/kkt_scan_impl.h), so the stand-alone scan of the launch-per-phase loop
and the copy inlined into the persistent kernel round alike at every nu.  Every comparison prints
its figure before it asserts (pytest -s).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import integrator_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

DERIV_TOL = 1e-10
STATE_TOL = 1e-12


def _np(t):
    return t.detach().cpu().numpy()


def _report(what, field, err):
    print(f"observed {what} {field} {err:.3e}")
    return err


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _lib_of(name):
    from noc import _lib
    return _lib.load_for(C.ocp(name).family)


# --------------------------------------------------------------------------------------------------
# 1. noc_derivatives and noc_nonlin_rollout at the case points
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_compute_derivatives_at_the_points(name):
    from noc.par_interior_point_newton import compute_derivatives
    X, U, _ = C.points(name)
    d = compute_derivatives(C.ocp(name), np.array(X), np.array(U), np.full(C.POINTS_B, C.POINTS_BP))
    torch.cuda.synchronize()
    ref = C.reference(name)
    for k in C.FIELDS:
        got = _np(getattr(d, k))
        assert got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        # the barrier's cu / cuu near the bound are of order 1e4 .. 1e11: relative to the field
        assert _report(f"derivatives[{name}]", k, relerr(got, ref[k])) < DERIV_TOL, k
    for k in ("fxx", "fuu"):
        got = _np(getattr(d, k))
        assert relerr(got, np.swapaxes(got, -1, -2)) < DERIV_TOL, k


@pytest.mark.parametrize("name", C.NAMES)
def test_zero_gain_rollout_stage_by_stage(name):
    from noc.par_interior_point_newton import nonlin_rollout
    X, U, _ = C.points(name)
    X, U = np.array(X), np.array(U)
    nx, nu = C.SHAPE[name]
    K = np.zeros((C.POINTS_B, C.POINTS_N, nu, nx))
    k = np.zeros((C.POINTS_B, C.POINTS_N, nu))
    xn, un = nonlin_rollout(C.ocp(name), K, k, X, U)
    xn, un = _np(xn), _np(un)
    assert np.array_equal(un, U) and np.array_equal(xn[:, 0], X[:, 0])
    prob = C.problem(name)
    for b in range(C.POINTS_B):
        steps = np.stack([prob.dynamics(x, u) for x, u in zip(xn[b, :-1], U[b])])
        assert _report(f"rollout[{name}]", "x", relerr(xn[b, 1:], steps)) < STATE_TOL


# --------------------------------------------------------------------------------------------------
# 2. the fused linearise
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["par", "seq"])
@pytest.mark.parametrize("lanes", [64, 8])
@pytest.mark.parametrize("name", C.NAMES)
def test_fused_linearisation_matches_autodiff(name, lanes, mode):
    from noc import _lib
    from noc.ipm import BatchedIPM
    from oracle import noc_oracle as O
    fam = C.ocp(name).family
    x0, U = C.linearise_start(name)
    N, B = C.LINEARISE_N, C.POINTS_B
    assert N % lanes != 0 and N % 8 != 0
    eng = BatchedIPM(fam, N, B, lanes=lanes)
    assert eng.lanes == lanes
    eng.load(U, x0)
    eng.init(bp0=0.1)
    eng.prepare(mode=_lib.MODE_PAR if mode == "par" else _lib.MODE_SEQ,
                terminal=_lib.TERMINAL_FINAL_COST)
    nat = eng.natural_blocks()
    torch.cuda.synchronize()
    prob = C.problem(name)
    X = _np(eng.t["x"])
    what = f"fused[{name},lanes={lanes},{mode}]"
    for b in range(B):
        assert relerr(X[b], O.rollout(prob.dynamics, U[b], x0[b])) < STATE_TOL
        assert prob.feasible(X[b], U[b])
        L = O.linearize(prob, X[b], U[b], 0.1)
        for k in ("A", "B", "Q", "R", "M", "r", "P"):
            got = _np(nat[k][b])
            assert got.shape == L[k].shape, (k, got.shape, L[k].shape)
            assert _report(what, k, relerr(got, L[k])) < DERIV_TOL, (k, b)


# --------------------------------------------------------------------------------------------------
# 3. whole solves against the oracle loops
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["par", "seq"])
@pytest.mark.parametrize("name", C.NAMES)
def test_solve_matches_the_oracle_loop(name, mode):
    from noc.par_interior_point_newton import par_interior_point_optimal_control
    from noc.seq_interior_point_newton import seq_interior_point_optimal_control
    from oracle import noc_oracle as O
    seed, iters, solves = C.STARTS[(name, mode)]
    N, B = C.shape_of(mode)
    x0, u0 = C.solve_start(name, N, B, seed)
    ocp = C.ocp(name)
    assert _lib_of(name).noc_ipm_solve_supported(ctypes.byref(ocp.family.to_c()), N, 64) == 1
    prob = C.problem(name)
    if mode == "par":
        U, its, info = par_interior_point_optimal_control(ocp, u0, x0, return_info=True)
        assert list(info["kkt_solves"]) == list(solves), (list(info["kkt_solves"]), solves)
    else:
        U, its = seq_interior_point_optimal_control(ocp, u0, x0)
    assert [int(v) for v in its] == list(iters), (its, iters)
    for b in range(B):
        if mode == "par":
            Ur = O.par_interior_point_optimal_control(prob, u0[b], x0[b], terminal="stage0")[0]
        else:
            Ur = O.seq_interior_point_optimal_control(prob, u0[b], x0[b])[0]
        assert _report(f"solve[{name},{mode}]", "U", float(np.max(np.abs(U[b] - Ur)))) < 1e-6


# --------------------------------------------------------------------------------------------------
# 4. the persistent solve: against the launch-per-phase loop, and dense against compact blocks
# --------------------------------------------------------------------------------------------------
def _engine_solve(name, mode, persistent):
    from noc import _lib
    from noc.ipm import BatchedIPM
    N, B = C.shape_of(mode)
    assert B == 3                         # a wave has neighbours
    x0, u0 = C.solve_start(name, N, B, C.STARTS[(name, mode)][0])
    eng = BatchedIPM(C.ocp(name).family, N, B, lanes=64, persistent=persistent)
    eng.load(u0, x0)
    eng.solve(mode=_lib.MODE_PAR if mode == "par" else _lib.MODE_SEQ)
    torch.cuda.synchronize()
    assert bool(torch.all(eng.t["phase"] == _lib.PHASE_DONE))
    U, it, s = eng.result()
    return U.clone(), _np(it).copy(), _np(s).copy()


@pytest.mark.parametrize("mode", ["par", "seq"])
@pytest.mark.parametrize("name", C.NAMES)
def test_persistent_equals_launch_per_phase(name, mode, monkeypatch):
    monkeypatch.setenv("NOC_PERSIST_WIDE", "0")
    Up, itp, sp = _engine_solve(name, mode, True)
    Um, itm, sm = _engine_solve(name, mode, False)
    assert np.array_equal(itp, itm) and np.array_equal(sp, sm), (itp, itm, sp, sm)
    _report(f"persistent[{name},{mode}]", "U", relerr(_np(Up), _np(Um)))
    assert torch.equal(Up, Um)
    iters = C.STARTS[(name, mode)][1]
    assert list(itp) == list(iters)


@pytest.mark.parametrize("name", C.NAMES)
def test_structured_blocks_equal_dense_instance(name, monkeypatch):
    monkeypatch.setenv("NOC_PERSIST_WIDE", "0")
    res = []
    for struct in ("1", "0"):
        monkeypatch.setenv("NOC_PERSIST_STRUCT", struct)
        res.append(_engine_solve(name, "par", True))
    (Us, its, ss), (Ud, itd, sd) = res
    assert np.array_equal(its, itd) and np.array_equal(ss, sd)
    assert torch.equal(Us, Ud)


# --------------------------------------------------------------------------------------------------
# 5. the wide kernel
# --------------------------------------------------------------------------------------------------
def test_wide_kernel_matches_the_oracle_and_the_one_wave_kernel(monkeypatch):
    from noc import _lib
    from noc.ipm import BatchedIPM
    name = C.CART
    fam = C.ocp(name).family
    lib = _lib_of(name)
    smallest = next(n for n in range(129, 4096)
                    if lib.noc_ipm_solve_supported(ctypes.byref(fam.to_c()), n, 64) == 1)
    assert smallest == C.WIDE_N
    seed, iters, solves = C.STARTS[(name, "wide")]
    x0, u0 = C.solve_start(name, C.WIDE_N, C.WIDE_B, seed)
    res = {}
    for wide in ("1", "0"):      # NOC_PERSIST_WIDE is read per launch (tests/test_ipm_gpu.py)
        monkeypatch.setenv("NOC_PERSIST_WIDE", wide)
        eng = BatchedIPM(fam, C.WIDE_N, C.WIDE_B, lanes=64, persistent=True)
        eng.load(u0, x0)
        eng.solve()
        torch.cuda.synchronize()
        assert np.all(_np(eng.t["phase"]) == _lib.PHASE_DONE)
        res[wide] = [_np(t).copy() for t in eng.result()]
    (Uw, itw, sw), (Un, itn, sn) = res["1"], res["0"]
    assert list(itw) == list(iters) and list(sw) == list(solves), (itw, sw)
    assert np.array_equal(itn, itw) and np.array_equal(sn, sw), (itn, sn)
    assert _report("wide", "U vs oracle", float(np.max(np.abs(Uw - C.wide_oracle_controls())))) < 1e-6
    assert _report("wide", "U vs one-wave", relerr(Uw, Un)) <= 1e-8
    assert not np.array_equal(Uw, Un), "the wide kernel did not run: bit-identical to the one-wave kernel"


# --------------------------------------------------------------------------------------------------
# 6. interior-point DDP
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [C.CART, C.PEND])
def test_ddp_matches_the_oracle(name):
    from noc.differential_dynamic_programming import interior_point_ddp
    from oracle import noc_oracle as O
    seed, iters, passes = C.STARTS[(name, "ddp")]
    N, B = C.shape_of("ddp")
    x0, u0 = C.solve_start(name, N, B, seed)
    ocp = C.ocp(name)
    assert _lib_of(name).noc_ddp_supported(ctypes.byref(ocp.family.to_c())) == 1
    U, its, info = interior_point_ddp(ocp, u0, x0, return_info=True)
    assert info["done"].all()
    assert [int(v) for v in its] == list(iters), (its, iters)
    assert [int(v) for v in info["passes"]] == list(passes), (info["passes"], passes)
    prob = C.problem(name)
    for b in range(B):
        Ur, itr, pr = O.interior_point_ddp(prob, u0[b], x0[b])
        assert (itr, pr) == (iters[b], passes[b])
        assert _report(f"ddp[{name}]", "U", float(np.max(np.abs(U[b] - Ur)))) < 1e-5, b
        X = O.rollout(prob.dynamics, U[b], x0[b])
        c = prob.total_cost(X, U[b], 0.8e-4)
        cr = prob.total_cost(O.rollout(prob.dynamics, Ur, x0[b]), Ur, 0.8e-4)
        assert _report(f"ddp[{name}]", "cost", abs(c - cr) / max(1.0, abs(cr))) <= 1e-9, b
        assert prob.feasible(X, U[b])
