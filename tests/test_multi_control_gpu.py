"""Every nx <= 4 solver path with more than one control: the three families of
tests/custom_families.py -- vectored_cartpole (4, 2), reaction_pendulum (3, 2, traced costs, a
coupled control constraint) and triple_drive_pendulum (2, 3, nu > nx) -- through the family device
code, the fused linearise, the KKT scan at every lane count, whole interior-point solves
(persistent, wide four-wave and launch-per-phase), interior-point DDP and the per-trajectory parameter record.

References and tolerances (the project's own, see the neighbouring files):
  * compute_derivatives, final_cost_grad, nonlin_rollout: the 50-digit mpmath reference of
    tests/multi_control_cases.py, 1e-12 of the field's own maximum per trajectory (no floor of 1);
    structurally zero fields exactly 0.0; total_cost within (N + 16) 2^-53 S.
  * fused linearise: oracle.linearize on the torch restatement, 1e-10, R and M as full matrices.
  * KKT step: lq_cases.rand_lq + oracle_batch at the three shapes, 1e-10, feasible equal.
  * whole solves: the oracle loops from the starts stored in multi_control_cases (every decision
    of the oracle at a 1e-6 relative margin, counts unchanged by a 1e-14 move of the start):
    identical iterations and KKT solves, controls 1e-6; the wide kernel at N = 129 likewise;
    persistent against launch-per-phase 1e-12; DDP as tests/test_ddp.py.
  * per-trajectory parameters: bit-identical, row for row, to the row solved alone with a family
    that carries its record.

Largest error observed on an MI355X (gfx950), printed before each assertion (pytest -s):
  compute_derivatives (three families): cx 1.5e-16  cu 2.2e-16  cxx 2.0e-16  cuu 2.1e-16
    cxu 8.7e-17  fx 2.3e-16  fu 1.7e-16  fxx 2.7e-16  fuu 2.6e-16  fxu 4.0e-16; zeros exact
  final-cost Hessian 0 (exact); total_cost 1.7e-16 of |cost|, 0.036 of its bound
  nonlin_rollout, per stage 8.2e-17
  fused linearise (lanes 64 and 8, par and seq): A 2.1e-16  B 1.1e-16  Q 8.0e-16  R 5.6e-16
    M 1.4e-15  r 1.2e-15  P 0  cost 1.9e-16
  KKT step, natural: dx 5.4e-15  du 3.7e-15  K 4.0e-15  d 2.8e-15  S 2.9e-15  v 4.1e-15
    pred 1.5e-15; tiled: dx 4.2e-15  du 6.7e-15; 256-register instance: du 2.4e-15
  whole solves: controls 5.8e-15 against the oracle loop, counts identical
  DDP: controls 6.1e-13, cost 1.2e-16
No kernel was found wrong.  (A start whose DDP path amplifies rounding until the counts part is
excluded by an oracle-only rule: see multi_control_cases.)
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import feasibility_cases as F  # noqa: E402
import multi_control_cases as C  # noqa: E402
from lq_cases import rand_lq, oracle_batch  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
RTOL = 1e-10
SHAPES = [C.SHAPE[n] for n in C.NAMES]
NAME_OF = {C.SHAPE[n]: n for n in C.NAMES}


def _report(what, field, err):
    print(f"observed {what} {field} {err:.3e}")
    return err


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64,
                                                  device="cuda")


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def ownerr(a, b):
    """max |a - b| over the reference's own maximum (no floor of 1)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / float(np.max(np.abs(b))))


def _lib_of(name):
    from noc import _lib
    return _lib.load_for(C.ocp(name).family)


def _problem(name, dt):
    from oracle import noc_oracle as O
    return O.NumpyProblem(C.torch_ocp(name, dt))


# --------------------------------------------------------------------------------------------------
# a. family device code
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_compute_derivatives_at_generic_points(name):
    from noc.par_interior_point_newton import compute_derivatives
    X, U, bp = C.generic_case(name)
    d = compute_derivatives(C.ocp(name), X, U, bp)
    torch.cuda.synchronize()
    ref = C.reference_derivatives(name)
    for k in C.FIELDS:
        got = _np(getattr(d, k))
        assert got.shape == ref[k].shape, (k, got.shape)
        for b in range(C.B):
            err = _report(f"derivatives[{name}]", k, C.own_max_error(got[b], ref[k][b]))
            assert err < TOL, (k, b, err)
    for k in C.ZERO_FIELDS[name]:
        assert not np.any(_np(getattr(d, k))), k
    # zeros inside a field are exact too, and the Hessians are symmetric bit for bit
    for k in C.FIELDS:
        got = _np(getattr(d, k))
        assert not np.any(got[ref[k] == 0.0]), k
    for k in ("cxx", "cuu", "fxx", "fuu"):
        got = _np(getattr(d, k))
        assert _bits_equal(got, np.swapaxes(got, -1, -2)), k


@pytest.mark.parametrize("name", C.NAMES)
def test_final_cost_grad_and_hessian(name):
    from noc.costates import final_cost_grad
    X, _, _ = C.generic_case(name)
    nx = C.SHAPE[name][0]
    xN = X.reshape(-1, nx)
    g, H = final_cost_grad(C.ocp(name), xN, hessian=True)
    torch.cuda.synchronize()
    _, rg, rH = C.final_grad_hess(name, xN)
    assert _report(f"final[{name}]", "grad", C.own_max_error(_np(g), rg)) < TOL
    assert _report(f"final[{name}]", "hess", C.own_max_error(_np(H), rH)) < TOL
    assert not np.any(_np(H)[rH == 0.0])


def _violations(name):
    """(trajectory, stage, state-or-control, index, value): one planted violation each"""
    import custom_families as CF
    ub = C.control_bounds(name)
    out = [("u", 1, float(np.nextafter(ub[1], np.inf))), ("u", 1, -float(np.nextafter(ub[1], np.inf)))]
    if name == C.C_NAME:
        out += [("u", 2, float(np.nextafter(ub[2], np.inf))), ("u", 2, -ub[2] * 1.5)]
    if name == C.B_NAME:
        out += [("coupled", None, None), ("x", 2, CF.RP_TORQUE * (1.0 + 1e-12))]
    return out


@pytest.mark.parametrize("name", C.NAMES)
def test_total_cost_and_feasibility(name):
    import custom_families as CF
    from noc.par_interior_point_newton import check_traj_feasibility, total_cost
    X, U, bp = C.generic_case(name)
    ocp = C.ocp(name)
    cost = _np(total_cost(ocp, X, U, bp))
    ok = _np(check_traj_feasibility(ocp, X, U))
    ref, bound = C.total_cost(name, X, U, bp)
    for b in range(C.B):
        _report(f"total_cost[{name}]", f"row {b} |err| / bound", abs(cost[b] - ref[b]) / bound[b])
        _report(f"total_cost[{name}]", f"row {b} |err| / |cost|", abs(cost[b] - ref[b]) / abs(ref[b]))
        assert abs(cost[b] - ref[b]) <= bound[b], (b, cost[b], ref[b], bound[b])
    assert ok.all() and C.feasible(name, X, U).all()
    for i, (what, j, v) in enumerate(_violations(name)):
        X2, U2 = X.copy(), U.copy()
        k = (5 * i + 2) % C.N if i % 2 else C.N - 1
        if what == "u":
            U2[1, k, j] = v
            if name == C.B_NAME:   # keep the coupled constraint out of it
                U2[1, k, 1 - j] = -1.0
        elif what == "x":
            X2[1, k, j] = v
        else:   # two ulps of RP_SUPPLY beyond u0 + u1 = RP_SUPPLY (the fp64 sum is exact: one ulp
            # of u1 would round back onto the constraint), both boxes respected
            U2[1, k] = [3.0, CF.RP_SUPPLY - 3.0 + 2.0 ** -49]
            assert U2[1, k, 0] + U2[1, k, 1] == CF.RP_SUPPLY + 2.0 ** -49
        want = C.feasible(name, X2, U2)
        assert list(want) == [True, False, True], (what, j, v)
        got = _np(check_traj_feasibility(ocp, X2, U2))
        assert np.array_equal(got, want), (what, j, v, got)


@pytest.mark.parametrize("name", C.NAMES)
def test_zero_gain_rollout_stage_by_stage(name):
    from noc.par_interior_point_newton import nonlin_rollout
    X, U, _ = C.generic_case(name)
    nx, nu = C.SHAPE[name]
    K = np.zeros((C.B, C.N, nu, nx))
    k = np.zeros((C.B, C.N, nu))
    xn, un = nonlin_rollout(C.ocp(name), K, k, X, U)
    xn, un = _np(xn), _np(un)
    assert _bits_equal(un, U) and _bits_equal(xn[:, 0], X[:, 0]) and np.all(np.isfinite(xn))
    steps = C.derivatives(name, xn, U, np.zeros(C.B) + 0.1)["step"]
    for b in range(C.B):
        assert _report(f"rollout[{name}]", "x", C.own_max_error(xn[b, 1:], steps[b])) < TOL


# --------------------------------------------------------------------------------------------------
# b. fused linearise
# --------------------------------------------------------------------------------------------------
def _fused_start(name):
    rng = np.random.default_rng(C._SEED[name] + 200)
    nx, nu = C.SHAPE[name]
    x0 = C._states(name, rng, C.B)
    if name == C.B_NAME:
        x0[:, 2] *= 0.1
    U = 0.6 * C.control_bounds(name) * rng.uniform(-1.0, 1.0, size=(C.B, C.N, nu))
    return x0, U


@pytest.mark.parametrize("mode", ["par", "seq"])
@pytest.mark.parametrize("lanes", [64, 8])
@pytest.mark.parametrize("name", C.NAMES)
def test_fused_linearisation_matches_autodiff(name, lanes, mode):
    from noc import _lib
    from noc.ipm import BatchedIPM
    from oracle import noc_oracle as O
    fam = C.ocp(name).family
    x0, U = _fused_start(name)
    eng = BatchedIPM(fam, C.N, C.B, lanes=lanes)
    assert eng.lanes == lanes
    eng.load(U, x0)
    eng.init(bp0=0.1)
    eng.prepare(mode=_lib.MODE_PAR if mode == "par" else _lib.MODE_SEQ,
                terminal=_lib.TERMINAL_FINAL_COST)
    nat = eng.natural_blocks()
    torch.cuda.synchronize()
    prob = _problem(name, C.DT)
    X = _np(eng.t["x"])
    what = f"fused[{name},lanes={lanes},{mode}]"
    for b in range(C.B):
        assert relerr(X[b], O.rollout(prob.dynamics, U[b], x0[b])) < 1e-12
        assert prob.feasible(X[b], U[b])
        L = O.linearize(prob, X[b], U[b], 0.1)
        for k in ("A", "B", "Q", "R", "M", "r", "P"):
            got = _np(nat[k][b])
            assert got.shape == L[k].shape, (k, got.shape, L[k].shape)
            assert _report(what, k, ownerr(got, L[k])) < RTOL, (k, b)
        cost = prob.total_cost(X[b], U[b], 0.1)
        assert _report(what, "cost", abs(eng.t["cost"][b].item() - cost) / abs(cost)) < RTOL


# --------------------------------------------------------------------------------------------------
# c. the KKT step on the new shapes
# --------------------------------------------------------------------------------------------------
def _solve(case, lanes, **kw):
    from noc import lqt
    g = lambda k: dev(case.get(k))
    res = lqt.kkt_solve(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), reg=g("reg"),
                        x0=g("x0"), q=g("q"), c=g("c"), p=g("p"), lanes=lanes, **kw)
    torch.cuda.synchronize()
    return res


def _check(out, ref, what, keys=("dx", "du", "K", "d", "S", "v", "pred")):
    for k in keys:
        err = _report(what, k, relerr(_np(getattr(out, k)), ref[k]))
        assert err < RTOL, (what, k, err)
    assert np.array_equal(_np(out.feasible).astype(bool), ref["feasible"].astype(bool)), what


def _horizons(L):
    return sorted({1, max(2, L // 2 - 1), L + 1, 2 * L + 3} if L > 1 else {1, 7, 45})


def _lane_counts(nx, nu):
    return [8, 16, 32, 64, 128] + ([1] if (nx, nu) == (4, 2) else [])


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("nx,nu,lanes", [(nx, nu, L) for nx, nu in SHAPES for L in _lane_counts(nx, nu)])
def test_kkt_matches_oracle(nx, nu, lanes, affine):
    """N < L, N = 1, N = L + 1 and a ragged 2 L + 3; B = 3 (the 512-register instance at 32 / 64)"""
    _lib_of(NAME_OF[(nx, nu)])
    for N in _horizons(lanes):
        case = rand_lq(6000 + 100 * nx + 10 * nu + N + lanes + int(affine), 3, N, nx, nu, affine=affine)
        _check(_solve(case, lanes, want_value=True), oracle_batch(case),
               f"kkt[{nx},{nu},L={lanes},N={N},{'affine' if affine else 'plain'}]")


@pytest.mark.parametrize("nx,nu,lanes", [(nx, nu, L) for nx, nu in SHAPES for L in (8, 16, 32, 64, 128)])
def test_tiled_kkt_matches_oracle(nx, nu, lanes):
    from noc import lqt
    _lib_of(NAME_OF[(nx, nu)])
    for N in _horizons(lanes):
        case = rand_lq(6500 + 100 * nx + 10 * nu + N + lanes, 3, N, nx, nu)
        ref = oracle_batch(case)
        g = lambda k: dev(case[k])
        tb = lqt.to_tiled(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"), lanes)
        out = lqt.kkt_solve_tiled(tb, reg=g("reg"), want_value=True)
        torch.cuda.synchronize()
        what = f"tiled[{nx},{nu},L={lanes},N={N}]"
        _check(out, ref, what, keys=("dx", "du", "S", "v", "pred"))
        K = lqt.untile(out.K, (3, N, nu, nx), lanes)
        d = lqt.untile(out.d, (3, N, nu), lanes)
        assert relerr(_np(K), ref["K"]) < RTOL and relerr(_np(d), ref["d"]) < RTOL, what


@pytest.mark.parametrize("lanes", [64, 32])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_kkt_small_register_instance(nx, nu, lanes):
    """B large enough that the waves exceed 4 x multi_processor_count: the 256-register instance
    (B = 3 above runs the 512-register one); N small, a sample against the oracle and the B = 3
    rows checked in both; nothing in the ABI says which instance ran, so the selection itself rests
    on the documented rule)."""
    _lib_of(NAME_OF[(nx, nu)])
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    B = (simds * 64) // lanes + 64 // lanes + 5          # waves = ceil(B lanes / 64) > simds
    N = lanes + 1
    case = rand_lq(6800 + nx + nu + lanes, B, N, nx, nu, affine=True)
    out = _solve(case, lanes, want_value=True)
    sample = sorted({0, 1, 2, B // 2, B - 2, B - 1})
    sub = {k: v[sample] for k, v in case.items()}
    ref = oracle_batch(sub)
    what = f"kkt256[{nx},{nu},L={lanes}]"
    for k in ("dx", "du", "K", "d", "S", "v", "pred"):
        assert _report(what, k, relerr(_np(getattr(out, k))[sample], ref[k])) < RTOL, (what, k)
    assert np.array_equal(_np(out.feasible)[sample].astype(bool), ref["feasible"].astype(bool))
    assert bool(torch.all(out.feasible == 1))
    few = _solve({k: v[:3] for k, v in case.items()}, lanes, want_value=True)
    _check(few, oracle_batch({k: v[:3] for k, v in case.items()}), what + " B=3")


@pytest.mark.parametrize("bwd_lanes,fwd_lanes", [(16, 32), (8, 128), (128, 64), (64, 8), (128, 128)])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_split_bwd_fwd_entry_points(nx, nu, bwd_lanes, fwd_lanes):
    from noc import lqt
    _lib_of(NAME_OF[(nx, nu)])
    case = rand_lq(7000 + 10 * nx + nu, 3, 37, nx, nu, affine=True)
    g = lambda k: dev(case.get(k))
    ref = oracle_batch(case)
    K, d, S, v, pred, feas = lqt.bwd_pass(g("A"), g("B"), g("Q"), g("R"), g("M"), g("r"), g("P"),
                                          reg=g("reg"), q=g("q"), c=g("c"), p=g("p"), lanes=bwd_lanes)
    du, dx = lqt.fwd_pass(g("A"), g("B"), K, d, x0=g("x0"), c=g("c"), lanes=fwd_lanes)
    torch.cuda.synchronize()
    for k, got in (("K", K), ("d", d), ("S", S), ("v", v), ("pred", pred), ("dx", dx), ("du", du)):
        assert relerr(_np(got), ref[k]) < RTOL, k
    assert bool(torch.all(feas == 1))


@pytest.mark.parametrize("lanes", [64, 32, 128])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_kkt_without_gains(nx, nu, lanes):
    """K = d = NULL where noc_kkt_gains_on_chip is 1 (asserted: these horizons fit)"""
    from noc import lqt
    _lib_of(NAME_OF[(nx, nu)])
    N = lanes + 1
    assert lqt.gains_on_chip(nx, nu, N, lanes)
    case = rand_lq(7100 + nx + nu + lanes, 3, N, nx, nu, affine=True)
    res = _solve(case, lanes, want_gains=False)
    assert res.K is None and res.d is None
    ref = oracle_batch(case)
    for k in ("dx", "du", "pred"):
        assert relerr(_np(getattr(res, k)), ref[k]) < RTOL, k
    assert np.array_equal(_np(res.feasible).astype(bool), ref["feasible"].astype(bool))


# LDL' pivots of (1 - a) I + a 11': nu = 2: 1, 1 - a^2; nu = 3: 1, 1 - a^2, (1 - a)(1 + 2 a)/(1 + a)
LAST_PIVOT_A = {2: 1.5, 3: -0.6}      # pivots 1, -1.25 and 1, 0.64, -0.8: only the last is negative


def _plant_last_pivot(case, b, s):
    nu = case["B"].shape[-1]
    a = LAST_PIVOT_A[nu]
    T = ((1.0 - a) * np.eye(nu) + a * np.ones((nu, nu))).astype(F.LD)
    S = F.value_chain(case, b, s + 1)[1][s + 1]
    Bs = np.asarray(case["B"][b, s], dtype=F.LD)
    R = T - F.LD(case["reg"][b]) * np.eye(nu, dtype=F.LD) - Bs.T @ S @ Bs
    case["R"][b, s] = np.asarray((R + R.T) / 2, dtype=np.float64)


@pytest.mark.parametrize("lanes", [8, 64, 128])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_planted_indefinite_last_pivot(nx, nu, lanes):
    """Quu = (1 - a) I + a 11' with every LDL' pivot but the last positive, planted in a stage of
    lane 0, of a middle lane and of the last lane (at 128 lanes: of wave 0, of wave 1 and at the
    join); the flag equals the oracle's and the clean batch-mates equal their solo solve bit for
    bit."""
    _lib_of(NAME_OF[(nx, nu)])
    N = 2 * lanes + 3
    pos = F.positions(N, lanes)
    Bt = 2 * len(pos) + 1
    case = rand_lq(7300 + 10 * nx + nu + lanes, Bt, N, nx, nu)
    clean = {k: v.copy() for k, v in case.items()}
    for i, s in enumerate(pos):
        _plant_last_pivot(case, 2 * i + 1, s)
    ref = oracle_batch(case)
    want = np.ones(Bt, dtype=bool)
    want[1::2] = False
    assert np.array_equal(ref["feasible"].astype(bool), want)
    out = _solve(case, lanes, want_value=True)
    assert np.array_equal(_np(out.feasible).astype(bool), want), (_np(out.feasible), pos)
    rows = list(range(0, Bt, 2))
    for k in ("dx", "du", "K", "d", "pred"):
        assert relerr(_np(getattr(out, k))[rows], ref[k][rows]) < RTOL, k
    solo = _solve({k: v[2:3] for k, v in clean.items()}, lanes, want_value=True)
    for k in ("dx", "du", "K", "d", "S", "v", "pred"):
        assert torch.equal(getattr(out, k)[2:3], getattr(solo, k)), k


# --------------------------------------------------------------------------------------------------
# d. whole interior-point solves
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["par", "seq"])
@pytest.mark.parametrize("name", C.NAMES)
def test_solve_matches_the_oracle_loop(name, mode):
    from noc.par_interior_point_newton import par_interior_point_optimal_control
    from noc.seq_interior_point_newton import seq_interior_point_optimal_control
    from oracle import noc_oracle as O
    seed, iters, solves = C.SOLVE_STARTS[name][mode]
    N, B = C.SOLVE_N, C.SOLVE_B
    x0, u0 = C.solve_start(name, N, B, seed)
    ocp = C.ocp(name, 1.0 / N)
    lib = _lib_of(name)
    assert lib.noc_ipm_solve_supported(ctypes.byref(ocp.family.to_c()), N, 64) == 1
    prob = _problem(name, 1.0 / N)
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


@pytest.mark.parametrize("name", C.NAMES)
def test_persistent_equals_launch_per_phase(name):
    from noc import _lib
    from noc.ipm import BatchedIPM
    seed = C.SOLVE_STARTS[name]["par"][0]
    N, B = C.SOLVE_N, C.SOLVE_B
    x0, u0 = C.solve_start(name, N, B, seed)
    fam = C.ocp(name, 1.0 / N).family
    res = []
    for persistent in (True, False):
        eng = BatchedIPM(fam, N, B, lanes=64, persistent=persistent)
        eng.load(u0, x0)
        eng.solve()
        torch.cuda.synchronize()
        res.append([_np(t) for t in eng.result()] + [_np(eng.t["phase"])])
    (Up, itp, sp, php), (Um, itm, sm, phm) = res
    assert np.all(php == _lib.PHASE_DONE) and np.array_equal(itp, itm) and np.array_equal(sp, sm)
    err = float(np.max(np.abs(Up - Um))) / max(1.0, float(np.max(np.abs(Um))))
    assert _report(f"persistent[{name}]", "U", err) <= 1e-12


_ONE_WAVE_CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = {paths!r}
import multi_control_cases as C
from noc.ipm import BatchedIPM
name, out = sys.argv[1], sys.argv[2]
x0, u0 = C.solve_start(name, C.WIDE_N, C.SOLVE_B, C.SOLVE_STARTS[name]["wide"][0])
eng = BatchedIPM(C.ocp(name, 1.0 / C.WIDE_N).family, C.WIDE_N, C.SOLVE_B, lanes=64, persistent=True)
eng.load(u0, x0)
eng.solve()
torch.cuda.synchronize()
U, it, s = (t.cpu().numpy() for t in eng.result())
np.savez(out, U=U, it=it, s=s)
"""


@pytest.mark.parametrize("name", C.NAMES)
def test_wide_kernel_matches_the_oracle_and_the_one_wave_kernel(name, tmp_path, monkeypatch):
    """The four-wave kernel (ipm_wide.hip) at the smallest N > 128 the persistent solve supports
    (129 for all three families: asserted), B = 2: the oracle's iterations and KKT solves, controls
    within 1e-6 of the oracle's (recorded under tests/golden, pinned to a fresh oracle run on the
    CPU), and against the one-wave kernel forced by NOC_PERSIST_WIDE=0 in a fresh child process:
    same counts, controls within 1e-8 relative (tests/test_ipm_gpu.py's bound), and NOT bit for
    bit -- the library has no query that says which kernel ran, but the two associate their scans
    differently, so differing last bits show that the wide kernel did run and that its LDS
    budget excludes none of the three families at this horizon."""
    import os
    import subprocess
    import sys
    from noc import _lib
    from noc.ipm import BatchedIPM
    fam = C.ocp(name, 1.0 / C.WIDE_N).family
    lib = _lib_of(name)
    smallest = next(n for n in range(129, 4096)
                    if lib.noc_ipm_solve_supported(ctypes.byref(C.ocp(name, 1.0 / n).family.to_c()), n, 64) == 1)
    assert smallest == C.WIDE_N
    seed, iters, solves = C.SOLVE_STARTS[name]["wide"]
    x0, u0 = C.solve_start(name, C.WIDE_N, C.SOLVE_B, seed)
    monkeypatch.setenv("NOC_PERSIST_WIDE", "1")
    eng = BatchedIPM(fam, C.WIDE_N, C.SOLVE_B, lanes=64, persistent=True)
    eng.load(u0, x0)
    eng.solve()
    torch.cuda.synchronize()
    Uw, itw, sw = (_np(t) for t in eng.result())
    assert np.all(_np(eng.t["phase"]) == _lib.PHASE_DONE)
    assert list(itw) == list(iters) and list(sw) == list(solves), (itw, sw)
    Ur = C.wide_oracle_controls(name)
    assert _report(f"wide[{name}]", "U vs oracle", float(np.max(np.abs(Uw - Ur)))) < 1e-6
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [root, os.path.join(root, "tests"), os.path.join(root, "ip-parallel-optimal-control_amd")]
    out = str(tmp_path / "one_wave.npz")
    subprocess.run([sys.executable, "-c", _ONE_WAVE_CHILD.format(paths=paths), name, out], check=True,
                   env=dict(os.environ, NOC_PERSIST_WIDE="0"), timeout=120)
    with np.load(out) as z:
        Un, itn, sn = z["U"], z["it"], z["s"]
    assert np.array_equal(itn, itw) and np.array_equal(sn, sw), (itn, sn)
    err = float(np.max(np.abs(Uw - Un))) / max(1.0, float(np.max(np.abs(Un))))
    assert _report(f"wide[{name}]", "U vs one-wave", err) <= 1e-8
    assert not _bits_equal(Uw, Un), "the wide kernel did not run: bit-identical to the one-wave kernel"


# --------------------------------------------------------------------------------------------------
# e. interior-point DDP
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_ddp_matches_the_oracle(name):
    from noc.differential_dynamic_programming import interior_point_ddp
    from oracle import noc_oracle as O
    seed, iters, passes = C.DDP_STARTS[name]
    N, B = C.DDP_N, C.DDP_B
    x0, u0 = C.solve_start(name, N, B, seed)
    ocp = C.ocp(name, 1.0 / N)
    assert _lib_of(name).noc_ddp_supported(ctypes.byref(ocp.family.to_c())) == 1
    U, its, info = interior_point_ddp(ocp, u0, x0, return_info=True)
    assert info["done"].all()
    prob = _problem(name, 1.0 / N)
    for b in range(B):
        Ur, itr, pr = O.interior_point_ddp(prob, u0[b], x0[b])
        assert (itr, pr) == (iters[b], passes[b])
        assert abs(int(its[b]) - itr) <= 1, (b, int(its[b]), itr)
        assert abs(int(info["passes"][b]) - pr) <= 1, (b, int(info["passes"][b]), pr)
        assert _report(f"ddp[{name}]", "U", float(np.max(np.abs(U[b] - Ur)))) < 1e-5, b
        X = O.rollout(prob.dynamics, U[b], x0[b])
        c = prob.total_cost(X, U[b], 0.8e-4)
        cr = prob.total_cost(O.rollout(prob.dynamics, Ur, x0[b]), Ur, 0.8e-4)
        assert _report(f"ddp[{name}]", "cost", abs(c - cr) / max(1.0, abs(cr))) <= 1e-9, b
        assert prob.feasible(X, U[b])


# --------------------------------------------------------------------------------------------------
# f. per-trajectory parameters
# --------------------------------------------------------------------------------------------------
def _rows(name, Bt):
    from noc import TrajectoryParams
    rng = np.random.default_rng(C._SEED[name] + 300)
    spec = C.SPEC[name]
    nx, nu = C.SHAPE[name]
    goal = np.array(spec["goal"]) + 0.2 * rng.normal(size=(Bt, nx))
    wx = np.array(spec["wx"]) * rng.uniform(0.5, 2.0, size=(Bt, nx))
    wf = np.array(spec["wf"]) * rng.uniform(0.5, 2.0, size=(Bt, nx))
    wu = np.array(spec["wu"]) * rng.uniform(0.5, 2.0, size=(Bt, nu))
    ub = spec["u_bound"] * rng.uniform(0.7, 1.5, size=Bt)
    assert all(len(set(r)) == nu for r in wu)
    return TrajectoryParams(goal=goal, wx=wx, wu=wu, wf=wf, u_bound=ub)


def _solo_ocp(name, p, b, dt):
    """the family carrying trajectory b's record as its own parameters"""
    from noc import families
    import custom_families as CF
    spec = dict(C.SPEC[name], goal=list(p.goal[b]), wx=list(p.wx[b]), wu=list(p.wu[b]),
                wf=list(p.wf[b]), u_bound=float(p.u_bound[b]))
    ode = {C.A_NAME: CF.vectored_cartpole_ode, C.C_NAME: CF.triple_drive_pendulum_ode}[name]
    return families.register_family(name, ode, dt=dt, build=False, **spec)


@pytest.mark.parametrize("name", C.PARAMETRISED)
def test_params_derivatives_row_for_row(name):
    from noc.par_interior_point_newton import compute_derivatives
    X, U, bp = C.generic_case(name)
    p = _rows(name, C.B)
    U = U * (p.u_bound / C.SPEC[name]["u_bound"])[:, None, None]
    d = compute_derivatives(C.ocp(name), X, U, bp, params=p)
    for b in range(C.B):
        solo = compute_derivatives(_solo_ocp(name, p, b, C.DT), X[b:b + 1], U[b:b + 1], bp[b:b + 1])
        for k in C.FIELDS:
            assert torch.equal(getattr(d, k)[b:b + 1], getattr(solo, k)), (k, b)
    assert bool(torch.isfinite(d.cuu).all())


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "phases"])
@pytest.mark.parametrize("name", C.PARAMETRISED)
def test_params_solve_row_for_row(name, persistent):
    from noc.ipm import BatchedIPM
    N, B = C.SOLVE_N, 3
    x0, u0 = C.solve_start(name, N, B, C.SOLVE_STARTS[name]["par"][0])
    p = _rows(name, B)
    fam = C.ocp(name, 1.0 / N).family
    lib = _lib_of(name)
    assert lib.noc_traj_params_supported(ctypes.byref(fam.to_c()), N, 64) == 1
    eng = BatchedIPM(fam, N, B, lanes=64, persistent=persistent, compact=False)
    eng.load(u0, x0)
    eng.load_params(p)
    eng.solve()
    torch.cuda.synchronize()
    Ub, itb, sb = (_np(t) for t in eng.result())
    for b in range(B):
        one = BatchedIPM(_solo_ocp(name, p, b, 1.0 / N).family, N, 1, lanes=64, persistent=persistent,
                         compact=False)
        one.load(u0[b:b + 1], x0[b:b + 1])
        one.solve()
        torch.cuda.synchronize()
        U1, it1, s1 = (_np(t) for t in one.result())
        assert it1[0] == itb[b] and s1[0] == sb[b], (b, it1, itb, s1, sb)
        assert _bits_equal(U1[0], Ub[b]), b


@pytest.mark.parametrize("name", C.PARAMETRISED)
def test_params_ddp_row_for_row(name):
    from noc.differential_dynamic_programming import interior_point_ddp
    N, B = C.DDP_N, 3
    x0, u0 = C.solve_start(name, N, B, C.DDP_STARTS[name][0])
    p = _rows(name, B)
    U, its, info = interior_point_ddp(C.ocp(name, 1.0 / N), u0, x0, return_info=True, params=p)
    for b in range(B):
        U1, it1, info1 = interior_point_ddp(_solo_ocp(name, p, b, 1.0 / N), u0[b:b + 1], x0[b:b + 1],
                                            return_info=True)
        assert int(it1[0]) == int(its[b]) and int(info1["passes"][0]) == int(info["passes"][b])
        assert _bits_equal(np.asarray(U1)[0], np.asarray(U)[b]), b


def test_params_refused_for_the_traced_cost_family():
    from noc import _lib
    from noc.ipm import BatchedIPM
    from noc import TrajectoryParams
    fam = C.ocp(C.B_NAME, 1.0 / C.SOLVE_N).family
    lib = _lib_of(C.B_NAME)
    assert lib.noc_traj_params_supported(ctypes.byref(fam.to_c()), C.SOLVE_N, 64) == 0
    eng = BatchedIPM(fam, C.SOLVE_N, 2, lanes=64, compact=False)
    with pytest.raises(_lib.NocError, match="unsupported family"):
        eng.load_params(TrajectoryParams(goal=np.zeros((2, 3))))
