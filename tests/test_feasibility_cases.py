"""Preconditions on the inputs of tests/test_kkt_feasibility_gpu.py (CPU, long double): the
planted stage has the pivots it claims, with a margin; everything that is meant to be clean is
positive definite, with a margin; positions(N, L) lands in the lane and wave it claims; the
oracle's flags are the expected ones.  None of this is an oracle for the device's path.

Margins (conditions on the inputs, not tolerances): every |pivot| and |lambda_min| of a planted
Quu >= 0.1; lambda_min(Quu) >= 1e-3 at every stage of a clean row and at every stage after the
planted one.  The device forms the same Quu in fp64 from the same fp64 inputs, so its pivots differ
from these by rounding (1e-13 at the worst conditioning seen here), far inside either margin."""
import functools

import numpy as np
import pytest

import feasibility_cases as FC
from lq_cases import oracle_batch

LD = np.longdouble
PLANTED_MARGIN = 0.1
CLEAN_MARGIN = 1e-3


def ldl_pivots(W):
    """D of W = L D L' without pivoting (plain loops, long double)."""
    W = np.asarray(W, dtype=LD)
    n = W.shape[0]
    Lm = np.eye(n, dtype=LD)
    D = np.zeros(n, dtype=LD)
    for j in range(n):
        D[j] = W[j, j] - sum(Lm[j, t] * Lm[j, t] * D[t] for t in range(j))
        for i in range(j + 1, n):
            Lm[i, j] = (W[i, j] - sum(Lm[i, t] * Lm[j, t] * D[t] for t in range(j))) / D[j]
    return D


def lam_min(W):
    return float(np.linalg.eigvalsh(np.asarray(W, dtype=np.float64)).min())


def header_owner(N, L, s):
    """The lane that owns stage s, restated from include/noc_hip.h by walking the chunks: lanes
    l < N % L own N / L + 1 stages, the others N / L, contiguous in time."""
    at = 0
    for l in range(L):
        n = N // L + (1 if l < N % L else 0)
        if at <= s < at + n:
            return l
        at += n
    raise AssertionError((N, L, s))


@functools.lru_cache(maxsize=None)
def made(case):
    nx, nu, L, N, affine, kind = case
    return FC.batch(nx, nu, N, L, kind, FC.seed_of(nx, nu, L, N), affine)


def test_case_grid_is_what_the_gpu_tests_claim():
    grid = {(nx, nu, L, N) for nx, nu, L, N, _ in FC.GRID}
    for nx, nu in ((2, 1), (4, 1), (8, 4)):
        for L in (8, 16, 32, 64):
            assert {(nx, nu, L, L - 1), (nx, nu, L, 2 * L + 3)} <= grid
        assert {(nx, nu, 1, 7), (nx, nu, 1, 37)} <= grid
        for N in (40, 100, 150):
            assert ((nx, nu, 128, N) in grid) == (nx <= 4)
    assert sum(g[4] for g in FC.GRID) * 2 == len(FC.GRID)
    for nx, nu, L, N, aff, kind in FC.CASES:
        assert kind in FC.KINDS and (nu == 4 or kind not in ("mid_pivot", "last_pivot"))
    assert {c[5] for c in FC.CASES if c[1] == 4} == set(FC.KINDS)
    assert {c[5] for c in FC.CASES if c[1] == 1} == {"neg", "zero", "nan"}
    assert max(2 * len(FC.positions(N, L)) + 1 for _, _, L, N, _ in FC.GRID) <= 13


@pytest.mark.parametrize("N,L", sorted({(N, L) for _, _, L, N, _ in FC.GRID}))
def test_positions_land_where_they_claim(N, L):
    claims = FC.positions(N, L, claims=True)
    stages = [s for s, _ in claims]
    assert stages == FC.positions(N, L) and len(set(stages)) == len(stages)
    assert all(0 <= s < N for s in stages)
    if L == 1:
        assert stages == [0, N // 2, N - 1]
        return
    for s, lane in claims:
        assert header_owner(N, L, s) == lane, (s, lane)
    owner = {s: l for s, l in claims}
    lens = [N // L + (1 if l < N % L else 0) for l in range(L)]
    last_full = max(l for l in range(L) if lens[l] > 0)
    if L == 128:
        assert owner[stages[0]] < 64
        if N == 40:
            assert len(stages) == 1 and all(header_owner(N, L, s) < 64 for s in range(N))
        else:
            assert len(stages) == 3
            assert 64 < owner[stages[1]] <= last_full          # wave 1, not its first lane
            assert owner[stages[2]] == 64 and header_owner(N, L, stages[2] - 1) == 63  # the join
        return
    assert 0 in stages and N - 1 in stages
    # the last stage of lane 0's chunk and the first of lane 1's are neighbours across a lane
    # boundary; a middle lane that is neither the first nor the last non-empty one
    b0 = max(s for s in range(N) if header_owner(N, L, s) == 0)
    assert b0 in stages and b0 + 1 in stages and header_owner(N, L, b0 + 1) == 1
    assert any(0 < l < last_full for l in owner.values())
    assert owner[N - 1] == last_full
    if N == L - 1:
        assert last_full == L - 2 and lens[L - 1] == 0           # the empty last lane
    else:
        assert sorted(set(lens)) == [2, 3]                       # ragged chunks


@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_planted_stage_and_clean_margins(case):
    nx, nu, L, N, affine, kind = case
    data, planted, clean, flags = made(case)
    pos = FC.positions(N, L)
    chains = FC.clean_chains(nx, nu, N, L, FC.seed_of(nx, nu, L, N), affine)
    assert len(planted) == len(pos) and len(clean) == len(pos) + 1
    assert data["A"].shape[0] == 2 * len(pos) + 1 <= 13
    assert list(flags) == [b % 2 == 0 for b in range(len(flags))]
    base = FC.batch(nx, nu, N, L, None, FC.seed_of(nx, nu, L, N), affine)[0]
    # clean rows: untouched by the planting, positive definite at every stage
    for b in clean:
        for k in data:
            assert np.array_equal(data[k][b], base[k][b]), (k, b)
        assert min(lam_min(q) for q in chains[b][0].values()) >= CLEAN_MARGIN
    for b, s in zip(planted, pos):
        # only stage s of the row differs from the clean data; the stages after it are clean and
        # positive definite (their Quu does not see stage s)
        keep = np.arange(N) != s
        for k in data:
            if k in ("A", "B", "Q", "R", "M", "r", "q", "c"):
                assert np.array_equal(data[k][b][keep], base[k][b][keep]), (k, b)
            else:
                assert np.array_equal(data[k][b], base[k][b]), (k, b)
        assert all(lam_min(chains[b][0][k]) >= CLEAN_MARGIN for k in range(s + 1, N))
        S = chains[b][1][s + 1]
        Bs, Rs = np.asarray(data["B"][b, s], dtype=LD), np.asarray(data["R"][b, s], dtype=LD)
        Quu = Rs + LD(data["reg"][b]) * np.eye(nu, dtype=LD) + Bs.T @ S @ Bs
        if kind == "nan":
            assert np.isnan(data["R"][b, s, 0, 0]) and np.isnan(data["R"][b, s]).sum() == 1
            continue
        if kind == "zero":
            S64 = np.asarray(S, dtype=np.float64)
            q64 = (data["R"][b, s] + data["reg"][b] * np.eye(nu)) + data["B"][b, s].T @ S64 @ data["B"][b, s]
            assert np.all(q64 == 0.0) and np.all(Quu == 0)
            assert np.any(data["M"][b, s] != 0.0)
            continue
        assert np.array_equal(data["R"][b, s], data["R"][b, s].T)
        piv = ldl_pivots(Quu)
        lam = np.linalg.eigvalsh(np.asarray(Quu, dtype=np.float64))
        assert np.all(np.abs(piv) >= PLANTED_MARGIN) and abs(lam.min()) >= PLANTED_MARGIN
        assert lam.min() < 0
        if kind == "neg":
            assert np.all(piv < 0) and np.allclose(np.asarray(Quu, float), -2 * np.eye(nu), atol=1e-12)
        else:
            want = np.array(FC.PIVOTS[kind])
            assert np.allclose(np.asarray(piv, float), want, rtol=0, atol=1e-9), piv
            assert np.all(np.diag(np.asarray(Quu, float)) > 0.9)
            if kind == "mid_pivot":
                assert list(np.sign(want)) == [1, 1, -1, 1]
            else:
                assert list(np.sign(want)) == [1, 1, 1, -1]
                assert all(np.linalg.det(np.asarray(Quu, float)[:k, :k]) > 0.1 for k in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def clean_oracle_flags(nx, nu, L, N, affine):
    base = FC.batch(nx, nu, N, L, None, FC.seed_of(nx, nu, L, N), affine)[0]
    return oracle_batch(base)["feasible"].astype(int)


@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_oracle_flags_are_the_expected_ones(case):
    """neg, mid_pivot, last_pivot: the oracle's eigenvalue test on the whole batch.  zero, nan: the
    expectation for the planted rows is the header's contract (the oracle would invert a singular
    matrix / take eigvalsh of NaN), so the oracle runs on the clean rows only."""
    nx, nu, L, N, affine, kind = case
    data, planted, clean, flags = made(case)
    if kind in ("zero", "nan"):
        got = clean_oracle_flags(nx, nu, L, N, affine)[clean]
        assert list(got) == [1] * len(clean) == list(flags[clean])
        assert list(flags[planted]) == [0] * len(planted)
    else:
        assert list(oracle_batch(data)["feasible"].astype(int)) == list(flags)


@pytest.mark.parametrize("grid", [g for g in FC.GRID if g[0] >= 4 and g[2] in (8, 16, 32)],
                         ids=lambda g: "%dx%d-L%d-N%d" % g[:4])
def test_a_clean_row_has_a_combine_that_partial_pivoting_would_swap(grid):
    """Why the bit-identity of the clean rows bites at nx >= 4, lanes < 64: a NaN (or 1/0) wave-mate
    fails the wave-wide vote of combine_sklansky at every level, so the whole wave redoes its
    combines with lu_pp_solve, while a clean row solved alone redoes only the levels it fails
    itself.  Every such batch holds a clean row with a planted wave-mate and a tree level at which
    none of its own combines fails (PASS_TAU margin) while one passes with a larger entry below
    the pivot (SWAP_RATIO margin) -- a level where partial pivoting in lu_pp_solve would exchange
    rows for it in the batch and not alone (the model of tests/neighbour_cases.py; a precondition
    on the inputs)."""
    import neighbour_cases as NC
    nx, nu, L, N, affine = grid
    data, planted, clean, flags = FC.batch(nx, nu, N, L, None, FC.seed_of(nx, nu, L, N), affine)
    per = 64 // L
    witnesses = []
    for b in clean:
        wave = range((b // per) * per, min(len(flags), (b // per + 1) * per))
        if any(m in planted for m in wave):
            levels = NC.census(data, b, L, tau=NC.PASS_TAU, ratio=NC.SWAP_RATIO)
            witnesses += [(b, lev) for lev, (f, s) in enumerate(levels) if f == 0 and s > 0]
    assert witnesses


@pytest.mark.parametrize("name,L,N", FC.COMPACT_GRID)
def test_compact_case_blocks_are_positive_definite(name, L, N):
    """The compact-scan cases plant into first-Newton-step blocks of the built-in families.  Here
    the oracle's linearisation of the same points (reg = ||cu||, P = the final cost's Hessian, as
    noc_ipm_prepare at NOC_MODE_PAR) is held to the clean margin; the device's blocks equal these
    to rounding, and the GPU test repeats the check on the blocks it actually solves."""
    pytest.importorskip("torch")
    from oracle import noc_oracle as O, problems as PR
    from noc import problems
    B = 2 * len(FC.positions(N, L)) + 1
    x0s, u0 = problems.initial_conditions(name, N, B, seed=FC.COMPACT_SEED)
    prob = O.NumpyProblem((PR.cartpole_ocp if name == "cartpole" else PR.pendulum_ocp)(1.0 / N))
    rows = []
    for b in range(B):
        lin = O.linearize(prob, O.rollout(prob.dynamics, u0[b], x0s[b]), u0[b], 0.1)
        rows.append(dict({k: lin[k] for k in ("A", "B", "Q", "R", "M", "P")},
                         reg=float(np.linalg.norm(lin["cu"]))))
    case = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    assert case["R"].shape == (B, N, 1, 1)
    for b in range(B):
        assert min(lam_min(q) for q in FC.value_chain(case, b, 0)[0].values()) >= CLEAN_MARGIN
