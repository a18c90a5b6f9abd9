"""The built-in families' device code (csrc/ipm_family.h: Fam<KIND, NX, NU>; csrc/families_gen.h:
gen::*_ode, _ode_jac, _ode_hess_l) away from the rest state, against the 50-digit mpmath reference
of tests/family_cases.py: angles over +-30 rad and on the wrap edges, |velocities| up to 12,
controls within 1e-9 of the bound, bp from 0.1 to 1e-8, and the per-trajectory-parameter twin.
Only single-pass entry points and the engine's linearise step run here: no solve loops from these
deliberately wild starts.

Tolerance: 1e-12 of the field's own maximum over a trajectory (no floor of 1) -- the tolerance of
tests/test_blocks_dense_gpu.py and ten times the oracle-vs-mpmath agreement that
tests/test_family_cases.py pins on the CPU at every point used here.  cu and cuu are also held
element by element (their terms wu u, bp / (u_bound - u), -bp / (u + u_bound) share u's sign, so no
element cancels).  Structurally zero fields (fuu, cxu, the off-diagonals of cxx; fxu for the
pendulum; fxx, fxu for the linear family) must be exactly 0.0.

total_cost is a 25-term sum: it is held to the fp64 evaluation's own bound (N + 16) 2^-53 S, S the
sum of the magnitudes of the pieces (family_cases.total_cost states where the 16 comes from).

Where wrap_angle is the only arithmetic the result is bit-identical to the reference on the whole
edge list (family_cases.same_bits; the reference has one zero): with goal 0 and weight 1, cx's
angle component and the final gradient's ARE wrap_angle(a); with the family's own goal and weight
they are fl(w fl(wrap(a) - goal)), two correctly rounded operations on exact inputs.

Largest error observed on an MI355X (gfx950), relative to the field's own maximum, per field over
all cases of this file (printed before each assertion, pytest -s):
  compute_derivatives, generic points (pendulum, cart-pole, linear2; shared and params=):
    cx 1.3e-16  cu 1.9e-16  cuu 1.9e-16  fx 2.0e-16  fu 2.1e-16  fxx 1.4e-16  fxu 2.3e-16
    cu element by element 3.2e-15 (pendulum), cuu element by element 2.9e-16
  compute_derivatives, edge angles:
    cx 1.4e-16  cu 2.0e-16  cuu 1.8e-16  fx 3.1e-16  fu 1.0e-16  fxx 2.6e-16  fxu 1.3e-16
  final_cost_grad                 1.0e-16 (Hessian bit-identical)
  total_cost                      2.0e-16 of |cost|, 0.045 of its bound
  nonlin_rollout, per stage       1.6e-16
  fused prepare (lanes 64 and 8): x 3.2e-17  A 3.3e-16  B 2.1e-16  Q 8.3e-16  R 1.1e-16
                                  M 9.3e-16  r 2.1e-16  P 0  cost 2.1e-16  hu 2.1e-16  gnorm 4.3e-16
cxx, cxu, fuu (and the other structural zeros) were exact; every bit-identity held.  wrap_angle at
a = -0.0, -2 pi, -4 pi gave -0.0, +0.0, -0.0 (see family_cases: the sign of a zero remainder).
No field needs more than 1e-12, and no kernel was found wrong.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import family_cases as C

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _report(what, field, err):
    print(f"observed {what} {field} {err:.3e}")
    return err


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check_fields(what, name, d, ref):
    """the ten fields of every trajectory against the reference; structural zeros exact"""
    fam = C.ocp(name).family
    for k in C.FIELDS:
        got = _np(getattr(d, k))
        for b in range(got.shape[0]):
            err = _report(what, k, C.own_max_error(got[b], ref[k][b]))
            assert err < TOL, (k, b, err)
    for k in ("cu", "cuu"):
        got, want = _np(getattr(d, k)), ref[k]
        err = _report(what, k + "_elementwise", float(np.max(np.abs(got - want) / np.abs(want))))
        assert err < TOL, (k, err)
    zero = ["fuu", "cxu"] + {"pendulum": ["fxu"], "cartpole": [], "linear2": ["fxu", "fxx"]}[name]
    for k in zero:
        assert not np.any(_np(getattr(d, k))), k
    cxx = _np(d.cxx)
    off = ~np.eye(fam.nx, dtype=bool)
    assert not np.any(cxx[..., off])
    if name == "linear2":
        assert _bits_equal(_np(d.fx)[0, 0], fam.A) and _bits_equal(_np(d.fu)[0, 0], fam.B)


@pytest.mark.parametrize("twin", [False, True], ids=["shared", "params"])
@pytest.mark.parametrize("name", C.NAMES)
def test_compute_derivatives_at_generic_points(name, twin):
    from noc.par_interior_point_newton import compute_derivatives
    c = C.generic_case(name, twin)
    d = compute_derivatives(C.ocp(name), c.X, c.U, c.bp, params=c.params)
    torch.cuda.synchronize()
    _check_fields(f"derivatives[{name}{',params' if twin else ''}]", name, d,
                  C.reference_derivatives(name, "generic", twin))


def _two_roundings(w, a, goal):
    """fl(w * fl(wrap(a) - goal)): the kernel's two operations, each correctly rounded"""
    from mpmath import mp, mpf
    with mp.workdps(C.DPS):
        e = float(C.wrap_mp(mpf(float(a))) - mpf(float(goal)))
        return float(mpf(float(w)) * mpf(e))


def _unit_params(name, Bt):
    from noc import TrajectoryParams
    nx = C.ocp(name).family.nx
    return TrajectoryParams(goal=np.zeros((Bt, nx)), wx=np.ones((Bt, nx)), wf=np.ones((Bt, nx)))


@pytest.mark.parametrize("twin", [False, True], ids=["shared", "params"])
@pytest.mark.parametrize("name", C.NONLINEAR)
def test_compute_derivatives_on_the_edge_angles(name, twin):
    from noc.par_interior_point_newton import compute_derivatives
    c = C.edge_case(name, twin)
    w = C.angle_index(name)
    n = len(C.EDGE_ANGLES)
    d = compute_derivatives(C.ocp(name), c.X, c.U, c.bp, params=c.params)
    torch.cuda.synchronize()
    _check_fields(f"derivatives_edge[{name}{',params' if twin else ''}]", name, d,
                  C.reference_derivatives(name, "edge", twin))
    # the wrap is the only inexact step of cx's angle component: bit-identical
    rows = C.family_rows(name, C.B, c.params)
    want = np.array([[_two_roundings(r["wx"][w], a, r["goal"][w]) for a in C.EDGE_ANGLES] for r in rows])
    assert C.same_bits(_np(d.cx)[:, :, w], want)
    # goal 0, weight 1: the component is wrap_angle(a) itself
    du = compute_derivatives(C.ocp(name), c.X, c.U, c.bp, params=_unit_params(name, C.B))
    wrapped = np.array([C.wrap_f64(a) for a in C.EDGE_ANGLES])
    got = _np(du.cx)[:, :, w]
    print("observed wrap_angle at -0.0, -2 pi, -4 pi:", [float(got[0, i]) for i in (1, 3, 5)])
    assert C.same_bits(got, np.broadcast_to(wrapped, (C.B, n)))


@pytest.mark.parametrize("twin", [False, True], ids=["shared", "params"])
@pytest.mark.parametrize("name", C.NAMES)
def test_final_cost_grad_and_hessian(name, twin):
    """at the edge angles (the generic points for the linear family), with and without params="""
    from noc import TrajectoryParams
    from noc.costates import final_cost_grad
    nonlinear = name in C.NONLINEAR
    c = (C.edge_case if nonlinear else C.generic_case)(name, twin)
    n = c.X.shape[1] - 1
    fam = C.ocp(name).family
    xN = c.X[:, :n].reshape(C.B * n, fam.nx)
    params = None
    if twin:  # trajectory b's row for each of its n states
        params = TrajectoryParams(**{k: np.repeat(np.asarray(getattr(c.params, k)), n, axis=0)
                                     for k in ("goal", "wx", "wu", "wf", "u_bound")})
    g, H = final_cost_grad(C.ocp(name), xN, hessian=True, params=params)
    torch.cuda.synchronize()
    _, rg, rH = C.final_grad_hess(name, xN, params)
    what = f"final[{name}{',params' if twin else ''}]"
    assert _report(what, "grad", C.own_max_error(_np(g), rg)) < TOL
    assert _bits_equal(_np(H), rH)  # diag(wf): no arithmetic at all
    g1 = final_cost_grad(C.ocp(name), xN, params=params)
    assert torch.equal(g1, g)
    if nonlinear:
        w = fam.wrap_index
        rows = C.family_rows(name, C.B * n, params)
        want = np.array([_two_roundings(r["wf"][w], x[w], r["goal"][w]) for r, x in zip(rows, xN)])
        assert C.same_bits(_np(g)[:, w], want)
        gu = final_cost_grad(C.ocp(name), xN, params=_unit_params(name, C.B * n))
        assert C.same_bits(_np(gu)[:, w], np.array([C.wrap_f64(x[w]) for x in xN]))


@pytest.mark.parametrize("twin", [False, True], ids=["shared", "params"])
@pytest.mark.parametrize("name", C.NAMES)
def test_total_cost_and_feasibility(name, twin):
    from noc.par_interior_point_newton import check_traj_feasibility, total_cost
    c = C.generic_case(name, twin)
    ocp = C.ocp(name)
    cost = _np(total_cost(ocp, c.X, c.U, c.bp, params=c.params))
    ok = _np(check_traj_feasibility(ocp, c.X, c.U, params=c.params))
    ref, bound = C.total_cost(name, c.X, c.U, c.bp, c.params)
    what = f"total_cost[{name}{',params' if twin else ''}]"
    for b in range(C.B):
        _report(what, f"row {b} |err| / bound", abs(cost[b] - ref[b]) / bound[b])
        _report(what, f"row {b} |err| / |cost|", abs(cost[b] - ref[b]) / abs(ref[b]))
        assert abs(cost[b] - ref[b]) <= bound[b], (b, cost[b], ref[b], bound[b])
    assert np.array_equal(ok, C.feasible(name, c.U, c.params)) and ok.all()
    # one ulp beyond its own bound, in the last stage of the middle trajectory only
    ub = C.family_rows(name, C.B, c.params)[1]["u_bound"]
    U2 = c.U.copy()
    U2[1, -1, 0] = -np.nextafter(ub, np.inf)
    ok2 = _np(check_traj_feasibility(ocp, c.X, U2, params=c.params))
    assert np.array_equal(ok2, C.feasible(name, U2, c.params)) and list(ok2) == [True, False, True]


@pytest.mark.parametrize("name", C.NAMES)
def test_zero_gain_rollout_stage_by_stage(name):
    """nonlin_rollout with K = 0, k = 0 is one dynamics step per stage from x_0: every stage is
    checked against the reference's step from the device's own x_k, so the chaotic dynamics
    amplify nothing."""
    from noc.par_interior_point_newton import nonlin_rollout
    c = C.generic_case(name)
    fam = C.ocp(name).family
    K = np.zeros((C.B, C.N, fam.nu, fam.nx))
    k = np.zeros((C.B, C.N, fam.nu))
    xn, un = nonlin_rollout(C.ocp(name), K, k, c.X, c.U)
    xn, un = _np(xn), _np(un)
    assert _bits_equal(un, c.U) and _bits_equal(xn[:, 0], c.X[:, 0])
    assert np.all(np.isfinite(xn))
    steps = C.euler_steps(name, xn[:, :-1], c.U)
    for b in range(C.B):
        assert _report(f"rollout[{name}]", "x", C.own_max_error(xn[b, 1:], steps[b])) < TOL


@pytest.mark.parametrize("name", C.NAMES)
def test_control_exactly_at_the_bound(name):
    """u == u_bound in one stage of the middle trajectory: feasible (the reference's <=), an
    infinite barrier, and the other trajectories untouched."""
    from noc.par_interior_point_newton import (check_traj_feasibility, compute_derivatives,
                                               total_cost)
    c = C.generic_case(name)
    ocp = C.ocp(name)
    U = c.U.copy()
    U[1, 7, 0] = ocp.family.u_bound
    d = compute_derivatives(ocp, c.X, U, c.bp)
    cost = _np(total_cost(ocp, c.X, U, c.bp))
    ok = _np(check_traj_feasibility(ocp, c.X, U))
    assert ok.all()
    assert cost[1] == np.inf and np.all(np.isfinite(cost[[0, 2]]))
    assert _np(d.cu)[1, 7, 0] == np.inf and _np(d.cuu)[1, 7, 0, 0] == np.inf
    keep = [0, 2]
    d2 = compute_derivatives(ocp, c.X[keep], U[keep], c.bp[keep])
    for k in C.FIELDS:
        assert torch.equal(getattr(d, k)[keep], getattr(d2, k)), k
        assert bool(torch.isfinite(getattr(d2, k)).all()), k
    assert _bits_equal(cost[keep], _np(total_cost(ocp, c.X[keep], U[keep], c.bp[keep])))
    # the stage's other fields are what they are without the barrier's pole
    ref = C.reference_derivatives(name)
    for k in ("cx", "fx", "fxx"):
        assert C.own_max_error(_np(getattr(d, k))[1, 6], ref[k][1, 6]) < TOL


@pytest.mark.parametrize("lanes", [64, 8])
@pytest.mark.parametrize("name", C.NONLINEAR)
def test_fused_linearisation_from_a_generic_start(name, lanes):
    """BatchedIPM.load / init / prepare: the fused rollout, linearise, costate and assemble bodies
    from x0 on the wrap edges with controls to 0.999 u_bound; blocks against the reference
    linearisation at the device's own X; compact and dense instances bit-identical."""
    from noc import _lib
    from noc.ipm import BatchedIPM
    fam = C.ocp(name).family
    x0, U = C.fused_start(name)
    bp = np.full(C.B, 0.1)
    got = {}
    for compact in (True, False):
        eng = BatchedIPM(fam, C.N, C.B, lanes=lanes, compact=compact)
        assert eng.compact == compact and eng.lanes == lanes
        eng.load(U, x0)
        eng.init(bp0=0.1)
        eng.prepare(mode=_lib.MODE_PAR, terminal=_lib.TERMINAL_FINAL_COST)
        torch.cuda.synchronize()
        out = {k: _np(v) for k, v in eng.natural_blocks().items()}
        out.update({k: _np(eng.t[k]).copy() for k in ("x", "u", "cost", "hu", "gnorm")})
        got[compact] = out
    for k in got[True]:
        assert _bits_equal(got[True][k], got[False][k]), k
    g = got[False]
    X = g["x"]
    what = f"fused[{name},lanes={lanes}]"
    assert _bits_equal(g["u"], U) and _bits_equal(X[:, 0], x0) and np.all(np.isfinite(X))
    steps = C.euler_steps(name, X[:, :-1], U)
    ref = C.reference_linearisation(name, X, U, bp)
    for b in range(C.B):
        assert _report(what, "x", C.own_max_error(X[b, 1:], steps[b])) < TOL
        for k in ("A", "B", "Q", "R", "M", "r", "P"):
            err = _report(what, k, C.own_max_error(g[k][b], ref[k][b]))
            assert err < TOL, (k, b, err)
        assert _report(what, "cost", abs(g["cost"][b] - ref["cost"][b]) / abs(ref["cost"][b])) < TOL
        hu = float(np.max(np.abs(ref["r"][b])))
        assert _report(what, "hu", abs(g["hu"][b] - hu) / hu) < TOL
        gn = float(np.linalg.norm(ref["cu"][b]))
        assert _report(what, "gnorm", abs(g["gnorm"][b] - gn) / gn) < TOL
