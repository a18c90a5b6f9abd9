"""CPU tests of the oracle (parity unpinned: the reference has no tests/fixtures and cannot run
here) -- it is pinned instead by independent cross-checks:
  * the faithful restatement of seq bwd/fwd (S:42-90) == dense KKT solve == associative-scan
    restatement of paroc (tree and sequential order) on well-conditioned problems;
  * the C restatement (oracle/kkt_ref.c) == the numpy restatement;
  * the numpy model of the HIP kernel's chunked wave scan == oracle for every lane count;
  * iteration counts of the full IPM loops == those the survey measured independently;
  * committed golden fixtures (tests/golden/golden_v1.npz) are reproduced.
"""
import os

import numpy as np
import pytest

from lq_cases import rand_lq, oracle_batch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "golden_v1.npz")


def _maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("nx,nu,N", [(2, 1, 30), (4, 1, 60), (8, 4, 30)])
@pytest.mark.parametrize("affine", [False, True])
def test_riccati_equals_dense_kkt_and_scan(nx, nu, N, affine):
    from oracle import noc_oracle as O
    case = rand_lq(nx * 10 + N + int(affine), 2, N, nx, nu, affine=affine)
    for b in range(2):
        g = lambda k: None if k not in case else case[k][b]
        args = (g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), g("reg"))
        dx, du, pred, feas, K, d, S, v = O.kkt_solve(*args, g("x0"), g("q"), g("c"), g("p"),
                                                     symmetrize=True)
        fdx = O.kkt_solve(*args, g("x0"), g("q"), g("c"), g("p"))[0]   # faithful S:42-90
        ddx, ddu, obj = O.dense_kkt(*args, g("x0"), g("q"), g("c"), g("p"))
        assert _maxrel(dx, ddx) < 1e-10 and _maxrel(du, ddu) < 1e-10
        assert _maxrel(fdx, ddx) < 1e-8
        # paper-form element scan (R^-1 form, paroc's formulation): its error grows with the
        # open-loop expansion of A - B R^-1 M' (exponential in N), hence the looser nx=8 bound
        stol = 1e-10 if nx <= 4 else 1e-7
        for tree in (False, True):
            S2, v2 = O.scan_bwd(*args, g("q"), g("c"), g("p"), tree=tree)
            assert _maxrel(S2, S) < stol and _maxrel(v2, v) < stol
        K2, d2, pred2, feas2 = O.gains_from_values(g("A"), g("B"), g("R"), g("M"), g("r"), S, v,
                                                   g("reg"), g("c"))
        du2, dx2 = O.scan_fwd(g("A"), g("B"), K2, d2, g("x0"), g("c"))
        assert _maxrel(dx2, dx) < stol and abs(pred2 - pred) < stol * 10 * max(1, abs(pred))
        assert feas and feas2
        if not affine:  # with x0 = 0, sum dV equals the QP optimum (survey §8c)
            assert abs(pred - obj) < 1e-9 * max(1.0, abs(obj))


def test_faithful_seq_riccati_drifts_on_long_nx8_horizons():
    """Finding recorded in DESIGN.md: S:61-62 propagate Vxx unsymmetrised; at nx=8, nu=4, N=200
    the faithful restatement drifts ~1e-4..1e-2 from the exact KKT solution, while the
    symmetrised Riccati and the chunked scan (the HIP kernel's algorithm) stay at ~1e-15."""
    import kernel_model as KM
    from oracle import noc_oracle as O
    case = rand_lq(8264, 1, 200, 8, 4)
    g = lambda k: case[k][0]
    args = (g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), g("reg"))
    exact = O.dense_kkt(*args)[0]
    faithful = O.kkt_solve(*args)[0]
    stable = O.kkt_solve(*args, symmetrize=True)[0]
    model = KM.model_kkt(*args, L=64)[0]
    assert _maxrel(faithful, exact) > 1e-7
    assert _maxrel(stable, exact) < 1e-12
    assert _maxrel(model, exact) < 1e-12


@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 1), (8, 4)])
@pytest.mark.parametrize("L", [64, 32, 16, 8])
@pytest.mark.parametrize("N", [1, 7, 75])
def test_kernel_model_matches_oracle(nx, nu, L, N):
    import kernel_model as KM
    case = rand_lq(N * 7 + L + nx, 2, N, nx, nu, affine=True)
    ref = oracle_batch(case)
    for b in range(2):
        g = lambda k: case[k][b]
        m = KM.model_kkt(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), g("reg"),
                         g("x0"), g("q"), g("c"), g("p"), L=L)
        for i, k in enumerate(["dx", "du", "pred", "feasible", "K", "d", "S", "v"]):
            if k == "feasible":
                assert bool(m[i]) == bool(ref[k][b])
            else:
                assert _maxrel(m[i], ref[k][b]) < 1e-11, k


def test_c_restatement_matches_numpy():
    from oracle import kkt_ref
    for nx, nu, N in [(2, 1, 40), (4, 1, 120), (8, 4, 30)]:
        case = rand_lq(nx + N, 4, N, nx, nu)
        ref = oracle_batch(case, symmetrize=False)
        out = kkt_ref.solve(*(case[k] for k in ("A", "B", "Q", "R", "M", "r", "P", "reg")), threads=2)
        for k in ("dx", "du", "pred", "K", "d"):
            assert _maxrel(out[k], ref[k]) < 1e-11, k
        assert np.array_equal(out["feasible"].astype(bool), ref["feasible"].astype(bool))


def test_feasibility_flag_matches_eigh_test():
    from oracle import kkt_ref
    case = rand_lq(3, 3, 20, 4, 1)
    case["R"][1, 5] = -30.0
    ref = oracle_batch(case, symmetrize=False)
    out = kkt_ref.solve(*(case[k] for k in ("A", "B", "Q", "R", "M", "r", "P", "reg")))
    assert list(ref["feasible"].astype(int)) == [1, 0, 1] == list(out["feasible"])


def test_derivative_oracle_against_finite_differences():
    """torch.func derivatives (the compute_derivatives restatement, P:13-28) vs central
    differences of the callables themselves."""
    from oracle import problems as PR
    ocp = PR.cartpole_ocp(0.01)
    rng = np.random.default_rng(0)
    X = rng.normal(size=(4, 4)) * 0.3
    U = rng.normal(size=(3, 1))
    cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu = PR.compute_derivatives(ocp, X, U, 0.1)
    h = 1e-6
    for k in range(3):
        for j in range(4):
            e = np.zeros(4); e[j] = h
            fd = (PR.dynamics_np(ocp, X[k] + e, U[k]) - PR.dynamics_np(ocp, X[k] - e, U[k])) / (2 * h)
            assert np.allclose(fd, fx[k][:, j], atol=1e-7)
        e = np.array([h])
        fd = (PR.dynamics_np(ocp, X[k], U[k] + e) - PR.dynamics_np(ocp, X[k], U[k] - e)) / (2 * h)
        assert np.allclose(fd, fu[k][:, 0], atol=1e-7)


def test_wrap_angle_matches_jnp_remainder_semantics():
    import torch
    from oracle import problems as PR
    x = np.array([-7.0, -1e-17, -0.0, 0.0, 3.0, 6.283185307179586, 7.5, -6.283185307179586, 1e3])
    got = PR.wrap_angle(torch.as_tensor(x)).numpy()
    ref = np.remainder(x, 2 * np.pi)   # numpy == jnp.remainder semantics
    assert np.array_equal(np.where(got == 0, 0.0, got), np.where(ref == 0, 0.0, ref))


@pytest.mark.slow
def test_pendulum_ipm_iteration_counts():
    """The oracle loops reproduce the counts the survey measured with an independent restatement
    (pendulum N=50 -- seq 79 iterations, par 70 outer / 87 KKT solves)."""
    from oracle import noc_oracle as O, problems as PR
    prob = O.NumpyProblem(PR.pendulum_ocp(0.02))
    u0 = 0.1 * np.random.default_rng(1).normal(size=(50, 1))
    x0 = np.array([0.1, -0.1])
    U, it, solves = O.par_interior_point_optimal_control(prob, u0, x0)
    assert (it, solves) == (70, 87)
    cost = prob.total_cost(O.rollout(prob.dynamics, U, x0), U, 0.0)
    assert abs(cost - 178.3114456) < 1e-5


def test_golden_fixtures_reproduced():
    from oracle import noc_oracle as O
    gold = np.load(GOLDEN)
    tags = sorted({k.split("/")[0] for k in gold.files if k.startswith("lq_")})
    assert len(tags) == 6
    for tag in tags:
        case = {k.split("/")[-1]: gold[k] for k in gold.files if k.startswith(tag + "/in/")}
        ref = oracle_batch(case)
        for k in ("dx", "du", "pred", "K", "d", "S", "v"):
            assert _maxrel(ref[k], gold[f"{tag}/out/{k}"]) < 1e-12, (tag, k)
    # cart-pole linearisation
    from oracle import problems as PR
    prob = O.NumpyProblem(PR.cartpole_ocp(1.0 / 20))
    L = O.linearize(prob, gold["cart20/x"], gold["cart20/u"], 0.1)
    for k in ("A", "B", "Q", "R", "M", "r", "P"):
        assert _maxrel(L[k], gold[f"cart20/{k}"]) < 1e-12, k


def test_golden_v3_schedule_solves_reproduced():
    """golden_v3 (whole solves the GPU schedule tests are held to, tests/test_schedules_oracle_gpu.py):
    the oracle regenerates two cart30 rows (par; seq for one) and one pend150 row -- counts exactly,
    controls and final cost to 1e-12 -- and the rows are the seeded draws the fixture names."""
    import sys
    from oracle import noc_oracle as O, problems as PR
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "ip-parallel-optimal-control_amd"))
    from noc import problems
    gold = np.load(os.path.join(os.path.dirname(GOLDEN), "golden_v3.npz"))
    draws = {"cart30": ("cartpole", 30, 24, 6), "cart200": ("cartpole", 200, 256, 11),
             "pend150": ("pendulum", 150, 8, 3)}
    for tag, (name, N, batch, seed) in draws.items():
        x0, u0 = problems.initial_conditions(name, N, batch, seed=seed)
        rows = gold[f"{tag}/rows"]
        assert np.array_equal(gold[f"{tag}/x0"], x0[rows]) and np.array_equal(gold[f"{tag}/u0"], u0[rows])
        exempt = rows == (int(gold["cart200/heavy_row"]) if tag == "cart200" else -1)
        assert np.all(gold[f"{tag}/min_margin"][~exempt] >= 64) and exempt.sum() <= 1
    assert list(gold["cart30/rows"]) == list(range(16))
    for tag, tocp, k, seq in (("cart30", PR.cartpole_ocp(1.0 / 30), 2, False),
                              ("cart30", PR.cartpole_ocp(1.0 / 30), 15, True),
                              ("pend150", PR.pendulum_ocp(1.0 / 150), 3, False)):
        prob = O.NumpyProblem(tocp)
        g = lambda key: gold[f"{tag}/{key}"][k]
        U, it, solves = O.par_interior_point_optimal_control(prob, g("u0"), g("x0"), terminal="stage0")
        assert (it, solves) == (int(g("par_iters")), int(g("par_kkt_solves"))), (tag, k)
        assert _maxrel(U, g("par_u")) < 1e-12, (tag, k)
        cost = prob.total_cost(O.rollout(prob.dynamics, U, g("x0")), U, 0.0)
        assert abs(cost - g("par_cost")) <= 1e-12 * abs(cost)
        if seq:
            Us, its = O.seq_interior_point_optimal_control(prob, g("u0"), g("x0"))
            assert its == int(g("seq_iters")) and _maxrel(Us, g("seq_u")) < 1e-12


def test_golden_v2_newton_blocks_reproduced():
    """golden_v2 (real c2 / c3 Newton blocks, faithful S:42-90 steps): the oracle regenerates the
    committed blocks and steps, and the faithful and symmetrised Riccati agree on them to 1e-12
    (so the GPU's symmetric-S scan is held to the faithful reference at 1e-10)."""
    import os
    from oracle import noc_oracle as O, problems as PR
    gold = np.load(os.path.join(os.path.dirname(GOLDEN), "golden_v2.npz"))
    for tag, tocp in (("pend100", PR.pendulum_ocp(1.0 / 100)), ("cart200", PR.cartpole_ocp(1.0 / 200))):
        prob = O.NumpyProblem(tocp)
        g = lambda k: gold[f"{tag}/{k}"]
        for b in range(2):
            X = O.rollout(prob.dynamics, g("u0")[b], g("x0")[b])
            assert _maxrel(X, g("x")[b]) < 1e-13
            L = O.linearize(prob, X, g("u0")[b], 0.1)
            for k in ("A", "B", "Q", "R", "M", "r", "P"):
                assert _maxrel(L[k], g(k)[b]) < 1e-12, (tag, k)
            blocks = [g(k)[b] for k in ("A", "B", "Q", "R", "M", "r", "P")]
            dx, du, pred, feas, K, d, _, _ = O.kkt_solve(*blocks, g("reg")[b], symmetrize=False)
            for k, v in (("dx", dx), ("du", du), ("pred", pred), ("K", K), ("d", d)):
                assert _maxrel(v, g(k)[b]) < 1e-12, (tag, k)
            sdx, sdu = O.kkt_solve(*blocks, g("reg")[b], symmetrize=True)[:2]
            assert _maxrel(sdx, dx) < 1e-12 and _maxrel(sdu, du) < 1e-12
