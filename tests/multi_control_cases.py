"""Cases for the three multi-control families of tests/custom_families.py, with a 50-digit
reference (test infrastructure; CPU only: nothing here imports torch or touches a device).

Families: vectored_cartpole (nx, nu) = (4, 2), parametrised cost; reaction_pendulum (3, 2), traced
costs with a coupled control constraint and a state constraint; triple_drive_pendulum (2, 3),
parametrised cost, more controls than states.

Reference.  Each family's ODE, its stage cost (with the log barrier), final cost and constraints
are restated once in mpmath at 50 digits, every constant built from its fp64 value and every input
converted from the fp64 value the kernel receives.  All ten compute_derivatives fields are
mpmath.diff partials (numerical differentiation at 50 digits) of those scalar functions, with
Euler's delta + dt J and dt H on top: independent of the sympy generator (noc/_codegen.py) and of
the torch.func oracle.  wrap_angle is family_cases.wrap_mp.  Results are rounded to fp64 at the end.

Points.  B = 3 trajectories x N = 24 stages per family, seeded, drawn directly, not rolled out:
angles over +-30 rad (every third within +-4 pi), velocities to +-12; controls feasible, each
control within 1e-6 and 1e-9 (relative) of a bound in some stage (NEAR below); for the reaction
pendulum stages 15 and 21 sit within 1e-9 and 1e-6 of the coupled constraint u0 + u1 <= 5, and
stage 12 within 1e-6 of the motor-torque (state) limit.  bp = 0.1, 1e-4, 1e-8, one per trajectory.

ZOO is a host-only (4, 2) "function zoo" for the generated code: every entry of
noc._codegen._UFUNCS, integer powers 1..9 and -1..-8, +-1/2, two non-integer powers and `%`.

SOLVE_STARTS / DDP_STARTS are the seeds of the whole-solve cases of tests/test_multi_control_gpu.py
with the oracle's counts (tests/test_multi_control_cases.py re-derives and asserts them): only
seeds at which every accept / reject and stopping decision of the oracle loop keeps a relative
margin of at least 1e-6 from its threshold, and at which the oracle counts the same when the start
controls are moved by PERTURB = 1e-14 (relative) either way.  The second rule is there because these loops
amplify a difference of a few ulps from pass to pass, so on a path of hundreds of passes the counts
can part although every single decision is clear.
"""
import functools
import math

import numpy as np
from mpmath import mp, mpf

import custom_families as CF
from family_cases import (BP, DPS, TWO_PI, FIELDS, _f64, _m, _unit, own_max_error,  # noqa: F401
                          same_bits, wrap_mp)

B, N = 3, 24
DT = CF.MULTI_CONTROL_DT
NAMES = tuple(CF.MULTI_CONTROL)
A_NAME, B_NAME, C_NAME = NAMES
SHAPE = {A_NAME: (4, 2), B_NAME: (3, 2), C_NAME: (2, 3)}
PARAMETRISED = (A_NAME, C_NAME)
SPEC = {A_NAME: CF.VC, C_NAME: CF.TD}
_SEED = {A_NAME: 3101, B_NAME: 3102, C_NAME: 3103}

# fields that are identically zero per family (must be exactly 0.0 on the device)
ZERO_FIELDS = {A_NAME: ("cxu",), B_NAME: (), C_NAME: ("cxu",)}


@functools.lru_cache(maxsize=None)
def ocp(name, dt=DT):
    """the registered family's OCP (its library is pre-built by build(); nothing is compiled here)"""
    return CF.MULTI_CONTROL[name][0](dt, build=False)


def torch_ocp(name, dt=DT):
    return CF.MULTI_CONTROL[name][1](dt)


# --------------------------------------------------------------------------------------------------
# the 50-digit restatement
# --------------------------------------------------------------------------------------------------
def ode_functions(name):
    """One scalar mpmath function of (x_0 .. x_{nx-1}, u_0 .. u_{nu-1}) per state derivative."""
    if name == A_NAME:
        g, pl, mc, mpole = (_m(v) for v in CF.VC_PHYS)
        k, lev = _m(CF.VC_GAIN), _m(CF.VC_LEVER)

        def cart_acc(x, th, xd, thd, u0, u1):
            s, c = mp.sin(th), mp.cos(th)
            return (u0 * mp.cos(k * u1) + mpole * s * (pl * thd ** 2 + g * c)) / (mc + mpole * s ** 2)

        def pole_acc(x, th, xd, thd, u0, u1):
            s, c = mp.sin(th), mp.cos(th)
            return (-u0 * mp.cos(k * u1) * c - mpole * pl * thd ** 2 * c * s - (mc + mpole) * g * s
                    + lev * u0 * mp.sin(k * u1)) / (pl * mc + pl * mpole * s ** 2)

        return [lambda x, th, xd, thd, u0, u1: xd, lambda x, th, xd, thd, u0, u1: thd,
                cart_acc, pole_acc]
    if name == B_NAME:
        g, d, lag = _m(9.81), _m(0.1), _m(0.05)
        return [lambda a, w, t, u0, u1: w,
                lambda a, w, t, u0, u1: -g * mp.sin(a) - d * w + t + _m(0.5) * u1 * mp.cos(a),
                lambda a, w, t, u0, u1: (u0 - t) / lag - _m(0.2) * u0 * u1]
    if name == C_NAME:
        g, l, d = _m(9.81), _m(1.0), _m(1e-2)
        g0, g1, g2 = (_m(v) for v in CF.TD_GAINS)
        return [lambda a, w, u0, u1, u2: w,
                lambda a, w, u0, u1, u2: -g / l * mp.sin(a) - d * w + g0 * u0 + g1 * mp.tanh(u1)
                + g2 * u2 * mp.cos(a)]
    raise ValueError(name)


def constraint_values(name, x, u):
    """the constraint vector (feasible iff every entry <= 0) as mpf"""
    x, u = [_m(v) for v in x], [_m(v) for v in u]
    if name == B_NAME:
        return [u[0] - _m(CF.RP_U0), -u[0] - _m(CF.RP_U0), u[1] - _m(CF.RP_U1), -u[1] - _m(CF.RP_U1),
                u[0] + u[1] - _m(CF.RP_SUPPLY), x[2] - _m(CF.RP_TORQUE), -x[2] - _m(CF.RP_TORQUE)]
    ub = _m(SPEC[name]["u_bound"])
    return [v - ub for v in u] + [-v - ub for v in u]


def _err(name, x):
    if name == B_NAME:
        goal, w = CF._RP_GOAL, 0
    else:
        goal, w = SPEC[name]["goal"], SPEC[name]["wrap_index"]
    return [(wrap_mp(_m(v)) if i == w else _m(v)) - _m(goal[i]) for i, v in enumerate(x)]


def stage_cost_terms(name, x, u, bp):
    """(stage cost, sum of the magnitudes of its pieces) as mpf"""
    e = _err(name, x)
    u = [_m(v) for v in u]
    if name == B_NAME:
        pieces = [_m(w) * t * t / 2 for w, t in zip(CF._RP_WX, e)]
        pieces += [_m(w) * v * v / 2 for w, v in zip(CF._RP_WU, u)]
        pieces += [_m(CF.RP_CROSS_U) * u[0] * u[1], _m(CF.RP_CROSS_VEL) * _m(x[1]) * u[1],
                   _m(CF.RP_CROSS_SIN) * mp.sin(_m(x[0])) * u[1], _m(CF.RP_QUARTIC) * _m(x[1]) ** 4]
    else:
        pieces = [_m(w) * t * t / 2 for w, t in zip(SPEC[name]["wx"], e)]
        pieces += [_m(w) * v * v / 2 for w, v in zip(SPEC[name]["wu"], u)]
    pieces += [-_m(bp) * mp.log(-g) for g in constraint_values(name, x, u)]
    return sum(pieces, mpf(0)), sum((abs(p) for p in pieces), mpf(0))


def final_cost_value(name, x):
    wf = CF._RP_WF if name == B_NAME else SPEC[name]["wf"]
    return sum((_m(w) * t * t for w, t in zip(wf, _err(name, x))), mpf(0)) / 2


def _partials(f, z, first=True, second=True):
    """gradient (nz,) and Hessian (nz, nz) of a scalar mpmath function by mpmath.diff"""
    nz = len(z)
    g = np.full((nz,), mpf(0), dtype=object)
    H = np.full((nz, nz), mpf(0), dtype=object)
    for j in range(nz):
        if first:
            g[j] = mp.diff(f, z, _unit(nz, j))
        if second:
            for k in range(j, nz):
                H[j, k] = H[k, j] = mp.diff(f, z, _unit(nz, j, k))
    return g, H


def ode_partials(name, x, u):
    """(f, J, H) of the ODE right-hand side itself: f (nx,), J (nx, nz), H (nx, nz, nz), mpf"""
    nx, nu = SHAPE[name]
    z = [_m(v) for v in np.concatenate((np.ravel(x), np.ravel(u)))]
    fns = ode_functions(name)
    f = np.array([fn(*z) for fn in fns], dtype=object)
    J = np.full((nx, nx + nu), mpf(0), dtype=object)
    H = np.full((nx, nx + nu, nx + nu), mpf(0), dtype=object)
    for i, fn in enumerate(fns):
        J[i], H[i] = _partials(fn, z)
    return f, J, H


def stage_fields(name, x, u, bp, dt=DT):
    """the ten fields of one stage plus x+ (mpf object arrays), FIELDS order then x+"""
    nx, nu = SHAPE[name]
    z = [_m(v) for v in np.concatenate((np.ravel(x), np.ravel(u)))]
    g, H = _partials(lambda *a: stage_cost_terms(name, a[:nx], a[nx:], bp)[0], z)
    f, J, Hd = ode_partials(name, x, u)
    h = _m(dt)
    fx = h * J[:, :nx]
    for i in range(nx):
        fx[i, i] = fx[i, i] + 1
    xn = np.array([z[i] + h * f[i] for i in range(nx)], dtype=object)
    return (g[:nx], g[nx:], H[:nx, :nx], H[nx:, nx:], H[:nx, nx:], fx, h * J[:, nx:],
            h * Hd[:, :nx, :nx], h * Hd[:, nx:, nx:], h * Hd[:, :nx, nx:], xn)


def derivatives(name, X, U, bp, dt=DT):
    """The ten noc.Derivatives fields (Bt, N, ...) fp64 and the Euler steps under key 'step'."""
    X, U = np.asarray(X, np.float64), np.asarray(U, np.float64)
    keys = FIELDS + ("step",)
    out = {k: [] for k in keys}
    with mp.workdps(DPS):
        for b in range(X.shape[0]):
            per = {k: [] for k in keys}
            for k in range(U.shape[1]):
                for key, v in zip(keys, stage_fields(name, X[b, k], U[b, k], bp[b], dt)):
                    per[key].append(_f64(v))
            for key in keys:
                out[key].append(np.stack(per[key]))
    return {k: np.stack(v) for k, v in out.items()}


def final_grad_hess(name, xN):
    """(final cost, gradient, Hessian) of terminal states xN (Bt, nx), fp64"""
    with mp.workdps(DPS):
        c, g, H = [], [], []
        for x in np.asarray(xN, np.float64):
            z = [_m(v) for v in x]
            gg, HH = _partials(lambda *a: final_cost_value(name, a), z)
            c.append(float(final_cost_value(name, z)))
            g.append(_f64(gg))
            H.append(_f64(HH))
    return np.array(c), np.stack(g), np.stack(H)


def total_cost(name, X, U, bp):
    """(cost, bound) per trajectory; bound = (N + 16) 2^-53 S as family_cases.total_cost"""
    cost, bound = [], []
    with mp.workdps(DPS):
        for b in range(len(X)):
            c = final_cost_value(name, X[b][-1])
            mag = abs(c)
            for k in range(len(U[b])):
                ck, mk = stage_cost_terms(name, X[b][k], U[b][k], bp[b])
                c, mag = c + ck, mag + mk
            cost.append(float(c))
            bound.append(float((len(U[b]) + 16) * mpf(2) ** -53 * mag))
    return np.array(cost), np.array(bound)


def max_constraint(name, X, U):
    """the largest constraint value over the stages of each trajectory (fp64 of the mpf value):
    a trajectory is feasible iff it is <= 0 (x_N is not tested)"""
    with mp.workdps(DPS):
        return np.array([float(max(max(constraint_values(name, x, u)) for x, u in zip(Xb[:-1], Ub)))
                         for Xb, Ub in zip(X, U)])


def feasible(name, X, U):
    return max_constraint(name, X, U) <= 0.0


# --------------------------------------------------------------------------------------------------
# the points
# --------------------------------------------------------------------------------------------------
# stage -> (control index, fraction of that control's own bound); index -1 is the last control
NEAR = {3: (0, 1.0 - 1e-6), 9: (1, -(1.0 - 1e-6)), 15: (-1, 1.0 - 1e-9), 21: (0, -(1.0 - 1e-9)),
        6: (1, 1.0 - 1e-9), 18: (0, 1.0 - 1e-9)}
COUPLED_STAGES = {15: 1e-9, 21: 1e-6}     # reaction pendulum: 1 - (u0 + u1) / RP_SUPPLY
TORQUE_STAGE = 12                         # reaction pendulum: torque = RP_TORQUE (1 - 1e-6)


def control_bounds(name):
    if name == B_NAME:
        return np.array([CF.RP_U0, CF.RP_U1])
    return np.full(SHAPE[name][1], SPEC[name]["u_bound"])


def _states(name, rng, n):
    k = np.arange(n)
    ang = np.where(k % 3 == 0, rng.uniform(-2.0 * TWO_PI, 2.0 * TWO_PI, n), rng.uniform(-30.0, 30.0, n))
    if name == A_NAME:
        return np.stack((rng.uniform(-3.0, 3.0, n), ang, rng.uniform(-8.0, 8.0, n),
                         rng.uniform(-12.0, 12.0, n)), axis=1)
    if name == B_NAME:
        return np.stack((ang, rng.uniform(-10.0, 10.0, n), rng.uniform(-5.9, 5.9, n)), axis=1)
    return np.stack((ang, rng.uniform(-10.0, 10.0, n)), axis=1)


@functools.lru_cache(maxsize=None)
def generic_case(name):
    """(X (B, N+1, nx), U (B, N, nu), bp (B,))"""
    rng = np.random.default_rng(_SEED[name])
    nx, nu = SHAPE[name]
    X = _states(name, rng, B * (N + 1)).reshape(B, N + 1, nx)
    ub = control_bounds(name)
    U = ub * (1.0 - 1e-6) * rng.uniform(-1.0, 1.0, size=(B, N, nu))
    if name == B_NAME:   # keep the generic stages well inside the coupled constraint
        over = U[..., 0] + U[..., 1] > 0.9 * CF.RP_SUPPLY
        U[..., 1] = np.where(over, -np.abs(U[..., 1]), U[..., 1])
    for k, (j, f) in NEAR.items():
        U[:, k, j] = ub[j] * f
        if name == B_NAME:   # the other control pulls away from the coupled constraint
            U[:, k, 1 - (j % nu)] = -np.abs(U[:, k, 1 - (j % nu)])
    if name == B_NAME:
        for k, gap in COUPLED_STAGES.items():
            U[:, k, 0] = 3.0 + 0.25 * np.arange(B)
            U[:, k, 1] = CF.RP_SUPPLY * (1.0 - gap) - U[:, k, 0]
        X[:, TORQUE_STAGE, 2] = CF.RP_TORQUE * (1.0 - 1e-6) * np.array([1.0, -1.0, 1.0])
    return X, U, BP.copy()


@functools.lru_cache(maxsize=None)
def reference_derivatives(name):
    X, U, bp = generic_case(name)
    return derivatives(name, X, U, bp)


# --------------------------------------------------------------------------------------------------
# the function zoo (host only): every _UFUNCS entry, the printer's power cases and `%`
# --------------------------------------------------------------------------------------------------
ZOO_SHAPE = (4, 2)
_ZOO_POS = [1.0 / math.factorial(n) for n in range(1, 10)]            # x ** 1 .. x ** 9
_ZOO_NEG = [0.5 ** n for n in range(1, 9)]                            # (1 + x) ** -1 .. ** -8


def zoo_ode(state, action):
    x0, x1, x2, x3 = state
    u0, u1 = np.atleast_1d(action)
    f0 = np.sin(x0) * np.tan(x1) + np.arcsin(x2) * u0 + x3 ** 9 / (1.0 + u1 ** 2)
    f1 = np.cos(x1 * u0) * np.arccos(x0) + np.arctan(x2 * u1) + np.arctan2(x3, u0)
    f2 = np.sinh(x0) * np.cosh(u1) + np.tanh(x1 * x2) + np.exp(-x3 * u0) + np.log(x0 + u1)
    f3 = np.sqrt(x1 + u0) + 1.0 / np.sqrt(x2 + u1) + (x3 + u0) ** 1.5 + (x0 + x2) ** (1.0 / 3.0)
    f3 = f3 + sum(a * x1 ** n for n, a in enumerate(_ZOO_POS, 1))
    f3 = f3 + sum(a * (1.0 + x2 * u1) ** (-n) for n, a in enumerate(_ZOO_NEG, 1))
    return np.hstack((f0, f1, f2, f3))


def zoo_constraints(state, action):
    u = np.atleast_1d(action)
    return np.hstack((u - 1.0, -u))


def zoo_final_cost(state):
    return 0.5 * ((11.0 * state[1]) % (2.0 * np.pi)) ** 2 + state[0] ** 2 * state[3]


def zoo_stage_cost(state, action, bp):
    u = np.atleast_1d(action)
    c = 0.5 * ((11.0 * state[1]) % (2.0 * np.pi) - 1.0) ** 2 + 0.1 * u[0] ** 2 + 0.2 * u[1] ** 2
    c = c + 0.05 * u[0] * u[1] * state[3] + 0.3 * state[0] * u[1]
    return c - bp * np.sum(np.log(-zoo_constraints(state, action)))


def zoo_ode_mp():
    m, pos, neg = _m, [_m(a) for a in _ZOO_POS], [_m(a) for a in _ZOO_NEG]
    third = m(1.0 / 3.0)
    return [
        lambda x0, x1, x2, x3, u0, u1: mp.sin(x0) * mp.tan(x1) + mp.asin(x2) * u0 + x3 ** 9 / (1 + u1 ** 2),
        lambda x0, x1, x2, x3, u0, u1: mp.cos(x1 * u0) * mp.acos(x0) + mp.atan(x2 * u1) + mp.atan2(x3, u0),
        lambda x0, x1, x2, x3, u0, u1: mp.sinh(x0) * mp.cosh(u1) + mp.tanh(x1 * x2) + mp.exp(-x3 * u0)
        + mp.log(x0 + u1),
        lambda x0, x1, x2, x3, u0, u1: mp.sqrt(x1 + u0) + 1 / mp.sqrt(x2 + u1) + (x3 + u0) ** m(1.5)
        + (x0 + x2) ** third + sum((a * x1 ** n for n, a in enumerate(pos, 1)), mpf(0))
        + sum((a * (1 + x2 * u1) ** (-n) for n, a in enumerate(neg, 1)), mpf(0))]


def zoo_stage_cost_mp(x, u, bp):
    w = wrap_mp(11 * x[1])
    c = (w - 1) ** 2 / 2 + _m(0.1) * u[0] ** 2 + _m(0.2) * u[1] ** 2
    c += _m(0.05) * u[0] * u[1] * x[3] + _m(0.3) * x[0] * u[1]
    return c - _m(bp) * (mp.log(1 - u[0]) + mp.log(1 - u[1]) + mp.log(u[0]) + mp.log(u[1]))


def zoo_final_cost_mp(x):
    return wrap_mp(11 * x[1]) ** 2 / 2 + x[0] ** 2 * x[3]


def zoo_points(n=12):
    """states in (0.15, 0.85)^4, controls in (0.1, 0.9)^2: inside every function's domain"""
    rng = np.random.default_rng(3200)
    return rng.uniform(0.15, 0.85, size=(n, 4)), rng.uniform(0.1, 0.9, size=(n, 2))


# --------------------------------------------------------------------------------------------------
# generated header on the host
# --------------------------------------------------------------------------------------------------
HOST_MAIN = r"""
#include <cstdio>
#include <vector>
using namespace noc::gen;
static void put(const char* tag, const double* v, int n) {
  std::printf("%s", tag);
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}
int main(int argc, char** argv) {
  const int nx = NX, nu = NU, nz = NX + NU;
  std::FILE* f = std::fopen(argv[1], "r");
  int n;
  if (!f || std::fscanf(f, "%d", &n) != 1) return 2;
  for (int p = 0; p < n; ++p) {
    double x[NX], u[NU], l[NX], bp;
    for (int i = 0; i < nx; ++i) if (std::fscanf(f, "%lf", &x[i]) != 1) return 2;
    for (int i = 0; i < nu; ++i) if (std::fscanf(f, "%lf", &u[i]) != 1) return 2;
    for (int i = 0; i < nx; ++i) if (std::fscanf(f, "%lf", &l[i]) != 1) return 2;
    if (std::fscanf(f, "%lf", &bp) != 1) return 2;
    double o[NX], J[NX * (NX + NU)], H[(NX + NU) * (NX + NU)];
    custom_ode(x, u, o); put("ode", o, nx);
    custom_ode_jac(x, u, J); put("jac", J, nx * nz);
    custom_ode_hess_l(x, u, l, H); put("hess_l", H, nz * nz);
    if (kCustomCost) {
      double c = custom_stage_cost(x, u, bp); put("stage_cost", &c, 1);
      double cx[NX], cu[NU], Q[NX * NX], R[NU * NU], M[NX * NU];
      custom_stage_grad(x, u, bp, cx, cu); put("cx", cx, nx); put("cu", cu, nu);
      custom_stage_hess(x, u, bp, Q, R, M); put("cxx", Q, nx * nx); put("cuu", R, nu * nu);
      put("cxu", M, nx * nu);
      double fc = custom_final_cost(x); put("final_cost", &fc, 1);
      double g[NX], Hf[NX * NX];
      custom_final_grad(x, g); put("final_grad", g, nx);
      custom_final_hess(x, Hf); put("final_hess", Hf, nx * nx);
      double ok = custom_feasible(x, u) ? 1.0 : 0.0; put("feasible", &ok, 1);
      double var[NX * NX + NU * NU + NX * NU], cst[NX * NX + NU * NU + NX * NU];
      for (int i = 0; i < nx * nx + nu * nu + nx * nu; ++i) {
        var[i] = custom_cost_hess_var[i]; cst[i] = custom_cost_hess_const[i];
      }
      put("hess_var", var, nx * nx + nu * nu + nx * nu);
      put("hess_const", cst, nx * nx + nu * nu + nx * nu);
    }
  }
  return 0;
}
"""


def host_source(header, nx, nu):
    """the generated header without its #include lines, behind a stand-alone main"""
    body = "\n".join(l for l in header.splitlines() if not l.lstrip().startswith("#include"))
    return (f"#include <cmath>\n#include <math.h>\n#define NOC_DEV static inline\n"
            f"#define NX {nx}\n#define NU {nu}\n" + body + HOST_MAIN)


def run_on_host(cxx, workdir, header, nx, nu, X, U, L, bp):
    """compile and run; returns one dict of fp64 arrays per point"""
    import os
    import subprocess
    src, exe, pts = (os.path.join(workdir, n) for n in ("gen_host.cpp", "gen_host", "points.txt"))
    with open(src, "w") as fh:
        fh.write(host_source(header, nx, nu))
    subprocess.run([cxx, "-O1", "-std=c++17", "-D_GNU_SOURCE", "-ffp-contract=off", "-o", exe, src,
                    "-lm"], check=True)
    with open(pts, "w") as fh:
        fh.write(f"{len(X)}\n")
        for x, u, l, b in zip(X, U, L, bp):
            fh.write(" ".join(repr(float(v)) for v in (*x, *u, *l, b)) + "\n")
    out = subprocess.run([exe, pts], check=True, capture_output=True, text=True).stdout
    res, first = [], None
    for line in out.splitlines():
        tag, *vals = line.split()
        first = first or tag
        if tag == first:
            res.append({})
        res[-1][tag] = np.array([float(v) for v in vals])
    return res


def host_reference(fns, stage_cost, final_cost, nx, nu, x, u, l, bp):
    """what the generated functions compute at one point, from mpmath.diff at 50 digits (fp64)"""
    with mp.workdps(DPS):
        z = [_m(v) for v in (*x, *u)]
        nz = nx + nu
        J = np.full((nx, nz), mpf(0), dtype=object)
        Hl = np.full((nz, nz), mpf(0), dtype=object)
        for i, fn in enumerate(fns):
            g, H = _partials(fn, z)
            J[i] = g
            Hl = Hl + _m(l[i]) * H
        ref = dict(ode=_f64([fn(*z) for fn in fns]), jac=_f64(J).ravel(), hess_l=_f64(Hl).ravel())
        if stage_cost is not None:
            g, H = _partials(lambda *a: stage_cost(a[:nx], a[nx:], bp), z)
            gf, Hf = _partials(lambda *a: final_cost(a), z[:nx])
            ref.update(stage_cost=_f64([stage_cost(z[:nx], z[nx:], bp)]), cx=_f64(g[:nx]),
                       cu=_f64(g[nx:]), cxx=_f64(H[:nx, :nx]).ravel(), cuu=_f64(H[nx:, nx:]).ravel(),
                       cxu=_f64(H[:nx, nx:]).ravel(), final_cost=_f64([final_cost(z[:nx])]),
                       final_grad=_f64(gf), final_hess=_f64(Hf).ravel())
    return ref


# --------------------------------------------------------------------------------------------------
# whole-solve starts (the oracle's counts are re-derived by tests/test_multi_control_cases.py)
# --------------------------------------------------------------------------------------------------
MARGIN = 1e-6
PERTURB = 1e-14     # relative move of the start controls under which the oracle's counts must hold
SOLVE_N, SOLVE_B = 40, 2
DDP_N, DDP_B = 30, 2
WIDE_N = 129          # the smallest N > 128 (the GPU test asserts noc_ipm_solve_supported there)
_REST = {A_NAME: [0.0, 0.0, 0.0, 0.0], B_NAME: [0.1, -0.1, 0.0], C_NAME: [0.1, -0.1]}


def solve_start(name, Nn, Bt, seed):
    """(x0 (Bt, nx), u0 (Bt, Nn, nu)) of a whole-solve case"""
    rng = np.random.default_rng(seed)
    nx, nu = SHAPE[name]
    x0 = np.array(_REST[name]) + 0.01 * rng.normal(size=(Bt, nx))
    u0 = 0.1 * rng.normal(size=(Bt, Nn, nu))
    return x0, u0


# name -> mode -> (seed, iterations per trajectory, KKT solves per trajectory (par only))
SOLVE_STARTS = {
    A_NAME: {"par": (41, (142, 127), (228, 201)), "seq": (42, (217, 192), None),
             "wide": (41, (228, 128), (414, 201))},
    B_NAME: {"par": (41, (55, 56), (67, 69)), "seq": (41, (67, 66), None),
             "wide": (41, (57, 56), (66, 65))},
    C_NAME: {"par": (41, (73, 67), (89, 83)), "seq": (41, (72, 70), None),
             "wide": (41, (67, 66), (82, 81))},
}
# name -> (seed, iterations per trajectory, backward passes per trajectory)
DDP_STARTS = {A_NAME: (42, (111, 105), (207, 191)), B_NAME: (41, (52, 51), (72, 70)),
              C_NAME: (41, (62, 62), (90, 90))}


def wide_oracle_controls(name):
    """the par oracle's controls (SOLVE_B, WIDE_N, nu) from the "wide" start, recorded under
    tests/golden/ (tests/test_multi_control_cases.py holds them against a fresh oracle run)"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_control_wide.npz")
    with np.load(path) as z:
        return z[name]
