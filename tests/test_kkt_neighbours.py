"""Preconditions of tests/test_kkt_neighbours_gpu.py, checked on the CPU, and the pivot census of
the committed real Newton blocks.

kernel_model.phase2_pivot_census restates the device's accept test for the combine's elimination
without row exchanges (csrc/small_linalg.h lu_np_solve) along the device's phase-2 tree.  For every
case of neighbour_cases.CASES it must find what makes the GPU test able to fail: a wave in which one
trajectory's combine fails the test while, at the same level, a wave-mate's combine passes it
although partial pivoting would exchange rows; and a trajectory that fails nowhere.  The model is
a precondition on the inputs only; it is never compared with the path the device took.
"""
import numpy as np
import pytest

import kernel_model as KM
import neighbour_cases as NC


def test_lu_np_ok_and_pp_would_swap_on_hand_made_matrices():
    I = np.eye(3)
    assert KM.lu_np_ok(I) and not KM.pp_would_swap(I)
    # |x00| = 0.6 >= 0.5 * 1.0: accepted without an exchange, yet partial pivoting takes row 1
    X = np.array([[0.6, 0.1, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]])
    assert KM.lu_np_ok(X) and KM.pp_would_swap(X)
    assert not KM.lu_np_ok(X, tau=0.7) and not KM.pp_would_swap(X, ratio=2.0)
    # |x00| = 0.4 < 0.5: rejected; a zero column is rejected too (colmax > 0)
    X[0, 0] = 0.4
    assert not KM.lu_np_ok(X) and KM.pp_would_swap(X)
    assert not KM.lu_np_ok(np.zeros((2, 2)))
    # the test looks at the ELIMINATED matrix: the second pivot 1 - 0.9 * 0.9 / 1 = 0.19 < 0.5 * 0.9
    Y = np.array([[1.0, 0.9, 0.0], [0.9, 1.0, 0.0], [0.0, 0.9, 1.0]])
    assert not KM.lu_np_ok(Y) and KM.pp_would_swap(Y)


def test_census_walks_the_sklansky_tree():
    """log2(L) levels with L / 2 combining lanes each; a lane with an empty chunk holds the
    identity (C = 0, so X = I: passes, no exchange).  N = 7 stages over 32 lanes: at level 0 only
    lanes 0, 2, 4, 6 combine a non-empty chunk."""
    data = NC.make_case(NC.CASES[0])
    levels = NC.census(data, 0, 8)
    assert len(levels) == 3 and all(0 <= f + s <= 4 for f, s in levels)
    wide = NC.census(data, 0, 32)
    assert len(wide) == 5 and sum(wide[0]) <= 4


@pytest.mark.parametrize("case", NC.CASES, ids=NC.IDS)
def test_case_has_a_failing_trajectory_beside_a_passing_one_that_would_swap(case):
    nx, nu, N, lanes, B, seed = case
    data = NC.make_case(case)
    failing, clean, witnesses = NC.classify(case, data)
    # the margins imply the device's own threshold: failing at 0.45 fails at 0.5, passing at
    # 0.55 passes at 0.5, a 1.1x larger entry is a larger entry
    exact = [NC.census(data, b, lanes) for b in range(B)]
    for b in failing:
        assert sum(f for f, _ in exact[b]) > 0
    for b in clean:
        assert sum(f for f, _ in exact[b]) == 0
    assert witnesses, "no wave mixes a failing combine with a passing one that would swap"
    for w, lev, f, m in witnesses:
        assert f // (64 // lanes) == m // (64 // lanes) == w and f != m
        assert exact[f][lev][0] > 0 and exact[m][lev][1] > 0
    # the control: a trajectory that never leaves lu_np_solve when solved alone -- and the
    # witnesses' wave-mates are such trajectories, so masking every failing one keeps them
    assert clean and set(clean).isdisjoint(failing)
    assert all(m in clean for _, _, _, m in witnesses)
    assert len(failing) < B


def test_case_list_covers_the_shapes():
    assert {c[:2] for c in NC.CASES} == {(4, 1), (8, 4)}
    assert {c[3] for c in NC.CASES} == {8, 16, 32} and {c[2] for c in NC.CASES} == {7, 19, 37}
    assert {c[4] for c in NC.CASES} == {5, 9}
    assert sum(NC.AFFINE.values()) * 2 == len(NC.CASES)
    for shape in [(4, 1), (8, 4)]:
        assert {c[3] for c in NC.CASES if c[:2] == shape} == {8, 16, 32}


def test_track_limit_family_newton_blocks_never_fail():
    """The registered nx = 4 family of tests/custom_families.py (cartpole_track_limit) on the
    inputs of its solve tests (N = 50, seed 3): the linearised blocks of the first six KKT solves
    of the par Newton loop at the first barrier parameter (oracle restatement; regularisation
    schedule and terminal block Q[0] as P:73, P:116-118, accepted and rejected steps alike) have
    no failing combine at any lane count, with the PASS_TAU margin.  So the interior-point
    solvers never reach the pivoting fallback on it, and tests/test_families_gpu.py needs no
    neighbour case."""
    pytest.importorskip("torch")
    from oracle import noc_oracle as O
    import custom_families as CF
    from noc import problems
    N, bp = 50, 0.1
    x0s, u0s = problems.initial_conditions("cartpole", N, 2, seed=3)
    prob = O.NumpyProblem(CF.cartpole_track_limit_torch(1.0 / N))
    for b in range(2):
        U, X, rp, r_inc = u0s[b], O.rollout(prob.dynamics, u0s[b], x0s[b]), 1.0, 2.0
        accepted = 0
        for _ in range(6):
            cost = prob.total_cost(X, U, bp)
            L = O.linearize(prob, X, U, bp)
            blocks = (L["A"], L["B"], L["Q"], L["R"], L["M"], L["r"], L["Q"][0])
            reg = rp * float(np.linalg.norm(L["cu"]))
            for lanes in (8, 16, 32, 64):
                levels = KM.phase2_pivot_census(*blocks, reg, L=lanes, tau=NC.PASS_TAU)
                assert sum(f for f, _ in levels) == 0, (b, lanes, levels)
            K, d, _, _, pred, feas = O.riccati_bwd(*blocks, reg)
            du, dx = O.riccati_fwd(L["A"], L["B"], K, d)
            new_cost = prob.total_cost(X + dx, U + du, bp) if prob.feasible(X + dx, U + du) else np.inf
            gain = (new_cost - cost) / pred
            if gain > 0 and feas:
                rp, r_inc, X, U = rp * max(1.0 / 3.0, 1.0 - (2.0 * gain - 1.0) ** 3), 2.0, X + dx, U + du
                accepted += 1
            else:
                rp, r_inc = rp * r_inc, 2 * r_inc
        assert accepted >= 2  # the walk moved: blocks of several iterates were counted


# passing-but-swapped combines per level on the committed blocks (measured; failing: none)
GOLDEN_SWAPS = {("cart200", 8): [0, 0, 0], ("cart200", 16): [0, 0, 0, 0],
                ("cart200", 32): [0, 0, 0, 0, 0], ("cart200", 64): [0, 0, 0, 0, 0, 0],
                ("cart20", 8): [0, 2, 4], ("cart20", 16): [0, 1, 2, 6],
                ("cart20", 32): [0, 0, 1, 6, 13], ("cart20", 64): [0, 0, 1, 6, 6, 0]}


@pytest.mark.parametrize("tag,B", [("cart200", 2), ("cart20", 1)])
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_real_cartpole_newton_blocks_never_fail_the_threshold_test(tag, B, lanes):
    """The recorded fact behind DESIGN §3.10's 'the pivoting fallback never runs' at c3: on the
    committed first-Newton-step blocks of the cart-pole problems (cart200: c3's N = 200, two
    trajectories; cart20: N = 20) NO combine of the phase-2 tree fails the threshold test, at any
    lane count (c3 runs 32 lanes), not even with the margin PASS_TAU = 0.55.  On cart200 partial
    pivoting would exchange no row either; on cart20 it would in up to 20 of 31 combines
    (GOLDEN_SWAPS) -- passing combines of the kind a failing wave-mate used to drag through the
    pivoting solve."""
    data = NC.golden_blocks(tag)
    assert data["A"].shape[0] == B and data["A"].shape[-1] == 4
    for b in range(B):
        assert [f for f, _ in NC.census(data, b, lanes, tau=NC.PASS_TAU)] == [0] * len(GOLDEN_SWAPS[tag, lanes])
        assert [s for _, s in NC.census(data, b, lanes)] == GOLDEN_SWAPS[tag, lanes]
