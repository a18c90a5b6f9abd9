"""Generic-state cases for the built-in families' device code, with a 50-digit reference
(test infrastructure; CPU only: nothing here imports torch or touches a device).

Reference.  The pendulum and cart-pole ODEs (examples/pendulum_runtime.py:59-72,
cartpole_runtime.py:54-81), the parametrised quadratic stage cost with the box log barrier
(PR:40-50 / CR:36-45 / LD:34-37), the final cost (PR:30-37 / CR:27-33) and wrap_angle
(noc/utils.py:8-10) are written once in mpmath at 50 digits.  Every constant is built from its fp64
value (mpf(9.81), mpf(6.283185307179586), mpf(dt)) and every input is converted from the fp64 value
the kernel receives (the family descriptor's own goal / weights / bound, or the packed
per-trajectory record), so both sides see the same numbers.  The dynamics' Jacobians and second
derivatives are mpmath.diff partials -- numerical differentiation at 50 digits, independent of the
sympy generator (noc/_codegen.py) and of the torch.func oracle (oracle/problems.py) -- with Euler's
delta + dt J and dt H applied on top; the cost gradients and Hessians are closed forms.  Results
are rounded to fp64 at the very end.

wrap_angle is C fmod by the double 2 pi, then + 2 pi if the remainder is negative and non-zero
(jnp.remainder).  wrap_f64 gives that value rounded to a double, to be compared bit for bit
(same_bits).  mpmath has one zero, so the reference cannot say which zero a remainder of zero is,
and same_bits takes -0.0 and +0.0 as the same number.  The implementations do differ there, at
a = -0.0, -2 pi, -4 pi and nowhere else: C fmod and jnp.remainder give -0.0 at all three,
np.remainder (noc.utils.wrap_angle) +0.0 at all three, and the devices' wrap_angle / noc_pymod
-0.0, +0.0, -0.0 (the fast path's a - copysign(2 pi, a) is x - x = +0.0).  No value depends on it:
the wrapped angle enters only as wrap - goal, which is the same double either way unless goal is
0, and then it is that zero's sign.

Points.  B = 3 trajectories x N = 24 stages per family, seeded; stage states are drawn directly
(compute_derivatives accepts any X), not rolled out:
  * angle: two stages of three uniform in +-30 rad, every third uniform in +-4 pi, so that each of
    the five wrap regions (a <= -4 pi, (-4 pi, 0), [0, 2 pi), [2 pi, 4 pi), >= 4 pi) holds at least
    8 stages (a plain +-30 draw leaves 7.5 expected in each inner period);
  * cart-pole cart velocity +-8, pole velocity +-12, pendulum velocity +-10, cart position +-3;
  * controls u_bound (1 - 1e-6) U(-1, 1), with stages 3, 9 at +-u_bound (1 - 1e-6) and stages 15,
    21 at +-u_bound (1 - 1e-9) in every trajectory;
  * bp = 0.1, 1e-4, 1e-8 for the three trajectories.
The per-trajectory-parameter twin keeps the states and the control fractions and gives each row
its own goal, wx, wu, wf and u_bound (noc.TrajectoryParams); a row's near-bound stages sit at its
own bound.  The linear family (double_integrators(1, 0.1, constrained=True)) varies only in its
cost and barrier terms.

EDGE_ANGLES is the fixed edge list for the angle slot.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
from mpmath import mp, mpf

TWO_PI = 6.283185307179586  # csrc/ipm_family.h: kTwoPi
DPS = 50
B, N = 3, 24
DT = 1.0 / N
LINEAR_STEP = 0.1
BP = np.array([0.1, 1e-4, 1e-8])
NEAR_STAGES = {3: 1.0 - 1e-6, 9: -(1.0 - 1e-6), 15: 1.0 - 1e-9, 21: -(1.0 - 1e-9)}

PENDULUM_CONSTANTS = dict(gravity=9.81, length=1.0, mass=1.0, damping=1e-3)
CARTPOLE_CONSTANTS = dict(gravity=9.81, pole_length=0.5, cart_mass=10.0, pole_mass=1.0)

_BASE = [0.0, -0.0, TWO_PI, -TWO_PI, 2.0 * TWO_PI, -2.0 * TWO_PI]
EDGE_ANGLES = np.array(
    _BASE
    + [float(np.nextafter(a, s)) for a in _BASE for s in (np.inf, -np.inf)]
    + [-1e-300, TWO_PI + 1e-3, -(TWO_PI + 1e-3), 13.0, -13.0, 1000.0, -1000.0])

NAMES = ("pendulum", "cartpole", "linear2")
NONLINEAR = ("pendulum", "cartpole")
FIELDS = ("cx", "cu", "cxx", "cuu", "cxu", "fx", "fu", "fxx", "fuu", "fxu")


# --------------------------------------------------------------------------------------------------
# families: the project's own descriptors (the fp64 values the kernels receive)
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ocp(name):
    from noc import problems
    if name == "pendulum":
        return problems.pendulum(DT)
    if name == "cartpole":
        return problems.cartpole(DT)
    if name == "linear2":
        return problems.double_integrators(1, LINEAR_STEP, constrained=True)
    raise ValueError(name)


def angle_index(name):
    return ocp(name).family.wrap_index


# --------------------------------------------------------------------------------------------------
# the 50-digit reference
# --------------------------------------------------------------------------------------------------
def _m(v):
    """the mpf of an fp64 input; an mpf passes through unrounded (tests/ddp_pass_cases.py hands the
    stage functions below the states of a 50-digit rollout)"""
    return v if isinstance(v, mpf) else mpf(float(v))


def wrap_mp(a):
    """wrap_angle of an mpf: C fmod by the double 2 pi (exact at this precision for |a| << 1e30),
    + 2 pi where the remainder is negative."""
    p = mpf(TWO_PI)
    r = a - int(a / p) * p  # int() truncates towards zero, as fmod's quotient does
    return r + p if r < 0 else r


def wrap_f64(a):
    """wrap_angle of the double a, rounded to a double."""
    with mp.workdps(DPS):
        return float(wrap_mp(mpf(float(a))))


def same_bits(a, b):
    """a and b are the same doubles bit for bit, -0.0 and +0.0 taken as one number (the reference
    has one zero; see the module docstring)."""
    a, b = (np.asarray(v, dtype=np.float64) + 0.0 for v in (a, b))  # -0.0 + 0.0 is +0.0
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def ode_functions(name, constants=None):
    """One scalar mpmath function of (x_0 .. x_{nx-1}, u) per state derivative."""
    if name == "pendulum":                       # PR:59-72
        c = dict(PENDULUM_CONSTANTS, **(constants or {}))
        g, l, m, d = (_m(c[k]) for k in ("gravity", "length", "mass", "damping"))
        return [lambda th, om, u: om,
                lambda th, om, u: -g / l * mp.sin(th) + (u - d * om) / (m * l ** 2)]
    if name == "cartpole":                       # CR:54-81
        c = dict(CARTPOLE_CONSTANTS, **(constants or {}))
        g, pl, mc, mpole = (_m(c[k]) for k in ("gravity", "pole_length", "cart_mass", "pole_mass"))
        mt = mc + mpole

        def cart_acc(x, th, xd, thd, a):
            s, co = mp.sin(th), mp.cos(th)
            return (a + mpole * s * (pl * thd ** 2 + g * co)) / (mc + mpole * s ** 2)

        def pole_acc(x, th, xd, thd, a):
            s, co = mp.sin(th), mp.cos(th)
            return (-a * co - mpole * pl * thd ** 2 * co * s - mt * g * s) / (
                pl * mc + pl * mpole * s ** 2)

        return [lambda x, th, xd, thd, a: xd, lambda x, th, xd, thd, a: thd, cart_acc, pole_acc]
    raise ValueError(name)


def _f64(a):
    """mpf object array -> fp64.  Magnitudes below 1e-40 are the noise floor of differentiating
    numerically at 50 digits (a second derivative of something linear comes out as ~1e-60, not 0)
    and are returned as exact zeros, so that a structurally zero field has a zero reference."""
    return np.array([float(mp.chop(v, tol=1e-40)) for v in np.ravel(np.array(a, dtype=object))],
                    dtype=np.float64).reshape(np.shape(a))


def _unit(n, *idx):
    o = [0] * n
    for i in idx:
        o[i] += 1
    return tuple(o)


def stage_dynamics(name, x, u, constants=None, jac=True, hess=True, dt=None):
    """Discrete dynamics at one stage in mpf object arrays: (x+, fx, fu, fxx, fuu, fxu), the
    shapes of noc.Derivatives without the stage axis.  Euler families: x + dt f, delta + dt J,
    dt H with J, H from mpmath.diff; the linear family: A x + B u with its own fp64 A, B."""
    fam = ocp(name).family
    nx, nu = fam.nx, fam.nu
    z = [_m(v) for v in np.concatenate((np.ravel(x), np.ravel(u)))]
    nz = nx + nu
    J = np.full((nx, nz), mpf(0), dtype=object)
    H = np.full((nx, nz, nz), mpf(0), dtype=object)
    if name == "linear2":
        A, Bm = np.asarray(fam.A, np.float64), np.asarray(fam.B, np.float64)
        for i in range(nx):
            for j in range(nx):
                J[i, j] = _m(A[i, j])
            for j in range(nu):
                J[i, nx + j] = _m(Bm[i, j])
        xn = np.array([sum((J[i, j] * z[j] for j in range(nz)), mpf(0)) for i in range(nx)], dtype=object)
        return xn, J[:, :nx], J[:, nx:], H[:, :nx, :nx], H[:, nx:, nx:], H[:, :nx, nx:]
    fns = ode_functions(name, constants)
    dt = _m(fam.dt if dt is None else dt)
    xn = np.array([z[i] + dt * fns[i](*z) for i in range(nx)], dtype=object)
    for i, f in enumerate(fns):
        for j in range(nz):
            if jac:
                J[i, j] = dt * mp.diff(f, z, _unit(nz, j))
            if hess:
                for k in range(j, nz):
                    H[i, j, k] = H[i, k, j] = dt * mp.diff(f, z, _unit(nz, j, k))
    fx = J[:, :nx].copy()
    for i in range(nx):
        fx[i, i] = fx[i, i] + 1
    return xn, fx, J[:, nx:], H[:, :nx, :nx], H[:, nx:, nx:], H[:, :nx, nx:]


def _err(name, x, goal):
    w = angle_index(name)
    return np.array([(wrap_mp(_m(v)) if i == w else _m(v)) - _m(goal[i]) for i, v in enumerate(x)],
                    dtype=object)


def stage_cost_terms(name, x, u, bp, row):
    """(stage cost, sum of the magnitudes of its pieces) as mpf."""
    e = _err(name, x, row["goal"])
    quad = sum((_m(w) * t * t for w, t in zip(row["wx"], e)), mpf(0)) / 2
    quad += sum((_m(w) * _m(v) ** 2 for w, v in zip(row["wu"], u)), mpf(0)) / 2
    ub, c, mag = _m(row["u_bound"]), quad, quad
    if ub > 0:
        for v in u:
            la, lb = mp.log(ub - _m(v)), mp.log(_m(v) + ub)
            c -= _m(bp) * (la + lb)
            mag += _m(bp) * (abs(la) + abs(lb))
    return c, mag


def stage_cost_derivs(name, x, u, bp, row):
    """cx, cu, cxx, cuu, cxu in closed form (mpf object arrays)."""
    fam = ocp(name).family
    nx, nu = fam.nx, fam.nu
    e = _err(name, x, row["goal"])
    zero = mpf(0)
    cx = np.array([_m(row["wx"][i]) * e[i] for i in range(nx)], dtype=object)
    cxx = np.full((nx, nx), zero, dtype=object)
    for i in range(nx):
        cxx[i, i] = _m(row["wx"][i])
    cu = np.full((nu,), zero, dtype=object)
    cuu = np.full((nu, nu), zero, dtype=object)
    ub, b = _m(row["u_bound"]), _m(bp)
    for j in range(nu):
        v = _m(u[j])
        cu[j] = _m(row["wu"][j]) * v
        cuu[j, j] = _m(row["wu"][j])
        if ub > 0:
            cu[j] += b / (ub - v) - b / (v + ub)
            cuu[j, j] += b / (ub - v) ** 2 + b / (v + ub) ** 2
    return cx, cu, cxx, cuu, np.full((nx, nu), zero, dtype=object)


def final_cost_terms(name, x, row):
    e = _err(name, x, row["goal"])
    c = sum((_m(w) * t * t for w, t in zip(row["wf"], e)), mpf(0)) / 2
    g = np.array([_m(w) * t for w, t in zip(row["wf"], e)], dtype=object)
    Hm = np.full((len(x), len(x)), mpf(0), dtype=object)
    for i, w in enumerate(row["wf"]):
        Hm[i, i] = _m(w)
    return c, g, Hm


def family_rows(name, Bt, params=None):
    """goal, wx, wu, wf, u_bound of each trajectory as the kernels receive them: the packed
    per-trajectory record, or the family descriptor's own values."""
    from noc import TrajectoryParams
    from noc.traj_params import pack
    fam = ocp(name).family
    rec = pack(params if params is not None else TrajectoryParams(), fam, Bt)
    nx, nu = fam.nx, fam.nu
    return [dict(goal=r[0:nx], wx=r[8:8 + nx], wu=r[16:16 + nu], wf=r[20:20 + nx], u_bound=r[28])
            for r in rec]


def derivatives(name, X, U, bp, params=None, constants=None):
    """The ten noc.Derivatives fields, (Bt, N, ...) fp64, of states X (Bt, N+1, nx) and controls U
    (Bt, N, nu) with bp (Bt,), each trajectory under its own parameter row."""
    X, U = np.asarray(X, np.float64), np.asarray(U, np.float64)
    rows = family_rows(name, X.shape[0], params)
    out = {k: [] for k in FIELDS}
    with mp.workdps(DPS):
        for b in range(X.shape[0]):
            per = {k: [] for k in FIELDS}
            for k in range(U.shape[1]):
                c = stage_cost_derivs(name, X[b, k], U[b, k], bp[b], rows[b])
                d = stage_dynamics(name, X[b, k], U[b, k], constants)[1:]
                for key, v in zip(FIELDS, c + d):
                    per[key].append(_f64(v))
            for key in FIELDS:
                out[key].append(np.stack(per[key]))
    return {k: np.stack(v) for k, v in out.items()}


def fxx_only(name, X, U, constants=None, dt=None):
    """fxx (N, nx, nx, nx) of one trajectory (the sensitivity demonstration)."""
    with mp.workdps(DPS):
        return np.stack([_f64(stage_dynamics(name, X[k], U[k], constants, jac=False, dt=dt)[3])
                         for k in range(len(U))])


def final_grad_hess(name, xN, params=None):
    """(final cost, gradient, Hessian) of terminal states xN (Bt, nx), fp64."""
    xN = np.asarray(xN, np.float64)
    rows = family_rows(name, xN.shape[0], params)
    with mp.workdps(DPS):
        t = [final_cost_terms(name, x, r) for x, r in zip(xN, rows)]
        return (np.array([float(v[0]) for v in t]), np.stack([_f64(v[1]) for v in t]),
                np.stack([_f64(v[2]) for v in t]))


def total_cost(name, X, U, bp, params=None):
    """(cost, bound) per trajectory.  bound is the fp64 evaluation's own error bound against the
    exact sum: any summation order of the N + 1 terms errs by at most N u S with u = 2^-53 and S the
    sum of the magnitudes of the pieces (the quadratic parts, bp |log|), and each piece carries at
    most 16 further roundings of relative size u (nx <= 4 squares, weights and adds; a log within
    2 ulp; the product with bp): bound = (N + 16) u S."""
    X, U = np.asarray(X, np.float64), np.asarray(U, np.float64)
    rows = family_rows(name, X.shape[0], params)
    cost, bound = [], []
    with mp.workdps(DPS):
        for b in range(X.shape[0]):
            c, mag = final_cost_terms(name, X[b, -1], rows[b])[0], mpf(0)
            mag += abs(c)
            for k in range(U.shape[1]):
                ck, mk = stage_cost_terms(name, X[b, k], U[b, k], bp[b], rows[b])
                c, mag = c + ck, mag + mk
            cost.append(float(c))
            bound.append(float((U.shape[1] + 16) * mpf(2) ** -53 * mag))
    return np.array(cost), np.array(bound)


def feasible(name, U, params=None):
    """all(constraints <= 0): the reference's closed comparison (P:45-47)."""
    U = np.asarray(U, np.float64)
    rows = family_rows(name, U.shape[0], params)
    return np.array([bool(np.all(U[b] - r["u_bound"] <= 0.0) and np.all(-U[b] - r["u_bound"] <= 0.0))
                     for b, r in enumerate(rows)])


def euler_steps(name, X, U):
    """x_k -> dynamics(x_k, u_k) for every stage of X (Bt, N, nx), U (Bt, N, nu): one reference
    step from each given state, fp64."""
    with mp.workdps(DPS):
        return np.stack([np.stack([_f64(stage_dynamics(name, x, u, jac=False, hess=False)[0])
                                   for x, u in zip(Xb, Ub)]) for Xb, Ub in zip(X, U)])


def linearisation(name, X, U, bp):
    """The LQ blocks of one Newton step at (X, U) (S:98-101 / P:145-149; terminal Hessian of the
    final cost): A, B, Q, R, M, r, P, cu and the total cost, with the costates recomputed here at 50
    digits.  X (Bt, N+1, nx), U (Bt, N, nu), bp (Bt,); fp64 results."""
    X, U = np.asarray(X, np.float64), np.asarray(U, np.float64)
    Bt, Nn = U.shape[0], U.shape[1]
    rows = family_rows(name, Bt)
    keys = ("A", "B", "Q", "R", "M", "r", "P", "cu")
    out = {k: [] for k in keys}
    with mp.workdps(DPS):
        for b in range(Bt):
            st = [stage_cost_derivs(name, X[b, k], U[b, k], bp[b], rows[b])
                  + stage_dynamics(name, X[b, k], U[b, k])[1:] for k in range(Nn)]
            _, lam, P = final_cost_terms(name, X[b, -1], rows[b])
            per = {k: [None] * Nn for k in keys}
            for k in range(Nn - 1, -1, -1):
                cx, cu, cxx, cuu, cxu, fx, fu, fxx, fuu, fxu = st[k]
                per["A"][k], per["B"][k], per["cu"][k] = fx, fu, cu
                per["r"][k] = cu + fu.T.dot(lam)
                per["Q"][k] = cxx + np.tensordot(lam, fxx, axes=(0, 0))
                per["R"][k] = cuu + np.tensordot(lam, fuu, axes=(0, 0))
                per["M"][k] = cxu + np.tensordot(lam, fxu, axes=(0, 0))
                lam = cx + fx.T.dot(lam)
            for k in keys:
                out[k].append(_f64(P) if k == "P" else np.stack([_f64(v) for v in per[k]]))
    res = {k: np.stack(v) for k, v in out.items()}
    res["cost"], res["cost_bound"] = total_cost(name, X, U, bp)
    return res


# --------------------------------------------------------------------------------------------------
# the points
# --------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    X: np.ndarray            # (Bt, N+1, nx)
    U: np.ndarray            # (Bt, N, nu)
    bp: np.ndarray           # (Bt,)
    params: Optional[object] = None   # noc.TrajectoryParams of the twin


_SEED = {"pendulum": 2024, "cartpole": 2025, "linear2": 2026}

_TWIN = {
    "pendulum": dict(goal=[[math.pi, 0.0], [2.5, 0.3], [0.7, -0.2]],
                     wx=[[1.0, 0.1], [2.0, 0.3], [0.5, 0.05]], wu=[[1e-3], [5e-3], [2e-2]],
                     wf=[[1.0, 0.1], [3.0, 0.2], [7.0, 0.4]], u_bound=[5.0, 3.0, 8.0]),
    "cartpole": dict(goal=[[0.0, math.pi, 0.0, 0.0], [0.4, 2.0, 0.1, -0.3], [-1.1, 4.5, -0.2, 0.6]],
                     wx=[[1.0, 10.0, 0.1, 0.1], [2.0, 3.0, 0.4, 0.7], [0.3, 17.0, 0.02, 0.9]],
                     wu=[[1e-3], [4e-3], [3e-2]],
                     wf=[[1.0, 10.0, 0.1, 0.1], [5.0, 2.0, 0.6, 0.3], [0.7, 31.0, 0.05, 1.3]],
                     u_bound=[50.0, 20.0, 75.0]),
    "linear2": dict(goal=[[0.0, 0.0], [0.6, -0.4], [-1.3, 0.2]],
                    wx=[[100.0, 1.0], [30.0, 2.0], [7.0, 0.5]], wu=[[0.1], [0.03], [0.4]],
                    wf=[[100.0, 1.0], [60.0, 3.0], [11.0, 0.8]], u_bound=[5.0, 2.0, 9.0]),
}


def _states(name, rng, n):
    """n states of family `name` at generic points."""
    if name == "linear2":
        return rng.uniform(-3.0, 3.0, size=(n, 2))
    k = np.arange(n)
    ang = np.where(k % 3 == 0, rng.uniform(-2.0 * TWO_PI, 2.0 * TWO_PI, n), rng.uniform(-30.0, 30.0, n))
    if name == "pendulum":
        return np.stack((ang, rng.uniform(-10.0, 10.0, n)), axis=1)
    return np.stack((rng.uniform(-3.0, 3.0, n), ang, rng.uniform(-8.0, 8.0, n),
                     rng.uniform(-12.0, 12.0, n)), axis=1)


def _fractions(rng, Bt, Nn):
    """u / u_bound: (1 - 1e-6) U(-1, 1), the NEAR_STAGES of every trajectory at the bound."""
    F = (1.0 - 1e-6) * rng.uniform(-1.0, 1.0, size=(Bt, Nn, 1))
    for k, f in NEAR_STAGES.items():
        F[:, k, 0] = f
    return F


@functools.lru_cache(maxsize=None)
def generic_case(name, twin=False) -> Case:
    from noc import TrajectoryParams
    rng = np.random.default_rng(_SEED[name])
    nx = ocp(name).family.nx
    X = _states(name, rng, B * (N + 1)).reshape(B, N + 1, nx)
    F = _fractions(rng, B, N)
    if twin:
        params = TrajectoryParams(**{k: np.array(v) for k, v in _TWIN[name].items()})
        ub = np.array(_TWIN[name]["u_bound"])[:, None, None]
    else:
        params, ub = None, ocp(name).family.u_bound
    return Case(name, X, ub * F, BP.copy(), params)


@functools.lru_cache(maxsize=None)
def edge_case(name, twin=False) -> Case:
    """One stage per edge angle in each of B trajectories (the other components and the controls
    generic, the controls within 0.9 u_bound), plus a terminal state."""
    from noc import TrajectoryParams
    rng = np.random.default_rng(_SEED[name] + 100)
    fam = ocp(name).family
    n = len(EDGE_ANGLES)
    X = _states(name, rng, B * (n + 1)).reshape(B, n + 1, fam.nx)
    X[:, :n, fam.wrap_index] = EDGE_ANGLES
    F = 0.9 * rng.uniform(-1.0, 1.0, size=(B, n, 1))
    if twin:
        params = TrajectoryParams(**{k: np.array(v) for k, v in _TWIN[name].items()})
        ub = np.array(_TWIN[name]["u_bound"])[:, None, None]
    else:
        params, ub = None, fam.u_bound
    return Case(name, X, ub * F, BP.copy(), params)


@functools.lru_cache(maxsize=None)
def fused_start(name):
    """(x0 (B, nx), controls (B, N, 1)) for BatchedIPM.load: angles -4 pi and 2 pi + 1e-3 from the
    edge list and 29.5, generic velocities, controls up to 0.999 u_bound."""
    rng = np.random.default_rng(_SEED[name] + 200)
    fam = ocp(name).family
    x0 = _states(name, rng, B)
    x0[:, fam.wrap_index] = [-2.0 * TWO_PI, TWO_PI + 1e-3, 29.5]
    U = fam.u_bound * 0.999 * rng.uniform(-1.0, 1.0, size=(B, N, 1))
    U[:, 5, 0] = fam.u_bound * 0.999 * np.array([1.0, -1.0, 1.0])
    return x0, U


@functools.lru_cache(maxsize=None)
def reference_derivatives(name, kind="generic", twin=False):
    c = (generic_case if kind == "generic" else edge_case)(name, twin)
    return derivatives(name, c.X, c.U, c.bp, c.params)


_LIN_CACHE = {}


def reference_linearisation(name, X, U, bp):
    """linearisation(), computed once per distinct (X, U, bp): the engine's variants (lanes,
    compact or dense) must roll out the same states."""
    key = (name, np.asarray(X).tobytes(), np.asarray(U).tobytes(), np.asarray(bp).tobytes())
    if key not in _LIN_CACHE:
        _LIN_CACHE[key] = linearisation(name, X, U, bp)
    return _LIN_CACHE[key]


def own_max_error(got, ref):
    """max |got - ref| relative to the field's own maximum (no floor); an identically zero
    reference demands exact zeros."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    diff = float(np.max(np.abs(got - ref))) if ref.size else 0.0
    if scale == 0.0:
        return 0.0 if diff == 0.0 else math.inf
    return diff / scale
