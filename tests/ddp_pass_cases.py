"""The first backward passes of interior-point DDP at one barrier value (D:98-186), restated in high
precision, and the seeded cases on which the one-launch kernel (ddp_solve_kernel, csrc/ddp_persistent.hip) is held to
them.  A helper, not a test: CPU only, nothing here imports torch or touches a device.

Reference.  reference_passes(name, x0, u0, bp, K) follows oracle.noc_oracle.ddp statement for
statement and stops after K backward passes:
  * dynamics, Euler step, stage and final cost, their derivatives and the wrapped angle are the
    50-digit mpmath functions of tests/family_cases.py (stage_dynamics, stage_cost_derivs,
    stage_cost_terms, final_cost_terms -- the stage-level bodies of its derivatives, total_cost,
    final_grad_hess and euler_steps), handed mpf states so that nothing is rounded to fp64 along a
    rollout; the parameter rows are family_rows';
  * the backward recursion is tests/dense_block_cases.py: ddp_bwd_ld in np.longdouble (the built-in
    families' Hessians are symmetric, so its full and upper Quu forms coincide); derivatives go in
    and gains come out as a double plus a double remainder, which a long double holds exactly;
  * the rollouts, the cost sums, the feasibility comparison and the gain are mpmath.
It keeps what the kernel keeps: the failure multiplier inside a retry loop is the OUTER iteration's
reg_inc while r_inc doubles per failure (D:132-133), rp is clipped to [1e-16, 1e16] (D:135), the
shrink is max(1/3, 1 - c (c c)) with c = 2 gain - 1 (D:131), the last trial becomes the nominal
trajectory accepted or not (D:154), and derivatives and cost are re-evaluated only when a new outer
iteration starts (D:109-112).  Per pass it returns it, inner, cost, new_cost, pred, gain, success,
rp after the update, |Hu|_inf and the trial (TX, TU), rounded to fp64 at the very end, plus the
margins the CPU test holds (tests/test_ddp_pass_cases.py): the smallest Quu pivot over |Quu| (nu = 1:
the pivot is Quu itself) and the trial controls' relative distance from the box.

Cases (CASES, fixed by seed).  Horizons are the shapes at which Chunks(N, 64) changes form -- N = 1,
2 (63, 62 idle lanes), 63, 64 (one stage per lane), 65 (one lane with two), 130 (3 / 2) -- for the
pendulum, {1, 65} for the cart-pole and {2, 65} for family_cases' linear2 (the NOC_FAMILY_LINEAR
branches, no Hessian record); dt = 1 / N as noc.problems.make_problem defines it (linear2: its own
step 0.1).  Starts are away from rest: x0 uniform in +-3 per component, u0 = frac u_bound U(-1, 1)
with frac cycling through 0.3, 0.9, 0.999, 1 - 1e-6 over the cases, bp in {0.1, 1e-3}, K = 3.
TWIN_CASES are the rows of one heterogeneous batch per family (goal, wx, wu, wf, u_bound per
trajectory, family_cases._TWIN) for noc_ddp_solve_params; TRACED_CASE starts the traced-cost
cart-pole of tests/custom_families.py (CXX, CUU, CXU of the record) whose cost -- the
parametrised one plus a quartic pole-rate penalty and the track limit inside the log barrier -- is
restated below in mpmath.  A case that breaks a decision margin of the CPU test is moved to its next
seed in _BUMP, never excused.

ORACLE_ERR[k] is the fp64 oracle's own error against this reference after k passes, measured over
every case in family_cases.own_max_error's measure; tests/test_ddp_pass_cases.py holds the table to
the measurement and tests/test_ddp_passes_gpu.py takes its bound from it.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
from mpmath import mp, mpf

import family_cases as F
from dense_block_cases import LD, ddp_bwd_ld

K = 3
FRACS = (0.3, 0.9, 0.999, 1.0 - 1e-6)
BPS = (0.1, 1e-3)
HORIZONS = {"pendulum": (1, 2, 63, 64, 65, 130), "cartpole": (1, 65), "linear2": (2, 65)}
TWIN_N = {"pendulum": 65, "cartpole": 65, "linear2": 65}
TWIN_BP = 0.1
TRACED_N, TRACED_BP = 65, 0.1
SCALARS = ("cost", "new_cost", "pred", "gain", "rp", "hu")   # compared within the bound
EXACT = ("it", "inner", "success")                          # compared exactly

# the fp64 oracle's error after k passes (tests/test_ddp_pass_cases.py::test_oracle_error_table)
ORACLE_ERR = {1: 2.5e-13, 2: 6e-14, 3: 5e-14}


def gpu_bound(k):
    """the bound of tests/test_ddp_passes_gpu.py after k passes: two orders over the oracle's own
    error (summation order, generated derivatives against autodiff), never below 1e-13"""
    return max(1e-13, 100.0 * ORACLE_ERR[k])


# --------------------------------------------------------------------------------------------------
# long double <-> mpf, exactly (a long double is a double plus a double remainder)
# --------------------------------------------------------------------------------------------------
def _ld(a):
    out = np.empty(np.shape(a), LD)
    flat = out.reshape(-1)
    for i, v in enumerate(np.ravel(np.array(a, dtype=object))):
        hi = float(v)
        flat[i] = LD(hi) + LD(float(v - mpf(hi)))
    return out


def _mpf(x):
    hi = float(x)
    return mpf(hi) + mpf(float(LD(x) - LD(hi)))


def _mp_array(a):
    a = np.asarray(a, LD)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(a.reshape(-1)):
        flat[i] = _mpf(v)
    return out


# --------------------------------------------------------------------------------------------------
# one trajectory's problem at 50 digits
# --------------------------------------------------------------------------------------------------
class Problem:
    """The parametrised problem of family `name` with horizon N: `row` is its goal / wx / wu / wf /
    u_bound (family_cases.family_rows), `constants` overrides of the ODE's constants."""

    def __init__(self, name, N, row, constants=None):
        self.name, self.N, self.row, self.constants = name, N, row, constants
        self.dt = None if name == "linear2" else 1.0 / N

    def step(self, x, u):
        return F.stage_dynamics(self.name, x, u, self.constants, jac=False, hess=False, dt=self.dt)[0]

    def derivs(self, x, u, bp):
        """the ten Derivatives fields of one stage, mpf object arrays in FIELDS order"""
        return (F.stage_cost_derivs(self.name, x, u, bp, self.row)
                + F.stage_dynamics(self.name, x, u, self.constants, dt=self.dt)[1:])

    def stage_cost(self, x, u, bp):
        return F.stage_cost_terms(self.name, x, u, bp, self.row)[0]

    def final(self, x):
        return F.final_cost_terms(self.name, x, self.row)

    def stage_feasible(self, x, u):
        ub = F._m(self.row["u_bound"])
        return all(v - ub <= 0 and -v - ub <= 0 for v in u)

    def box_margin(self, X, U):
        """smallest relative distance of a trial control from either face of its box"""
        ub = F._m(self.row["u_bound"])
        return float(min(abs(abs(v) - ub) for u in U for v in u) / ub)


class TracedCartpole(Problem):
    """tests/custom_families.py: cartpole_track_limit -- the cart-pole ODE with the parametrised
    cart-pole cost (wu = 1e-3, |u| <= 50), + 1e-3 thd^4, and -bp (log(L - x) + log(x + L)) of the
    track limit |x| <= L = X_LIMIT; x_k, k < N, must satisfy the limit too (P:45-47)."""
    LIMIT = 0.5
    QUARTIC = 1e-3

    def __init__(self, N):
        row = dict(goal=[0.0, math.pi, 0.0, 0.0], wx=[1e0, 1e1, 1e-1, 1e-1], wu=[1e-3],
                   wf=[1e0, 1e1, 1e-1, 1e-1], u_bound=50.0)
        super().__init__("cartpole", N, row)

    def derivs(self, x, u, bp):
        d = list(super().derivs(x, u, bp))
        cx, cxx = d[0].copy(), d[2].copy()
        L, b, q, p, v = mpf(self.LIMIT), F._m(bp), mpf(self.QUARTIC), F._m(x[0]), F._m(x[3])
        cx[0] += b / (L - p) - b / (p + L)
        cxx[0, 0] += b / (L - p) ** 2 + b / (p + L) ** 2
        cx[3] += 4 * q * v ** 3
        cxx[3, 3] += 12 * q * v ** 2
        d[0], d[2] = cx, cxx
        return tuple(d)

    def stage_cost(self, x, u, bp):
        L, p = mpf(self.LIMIT), F._m(x[0])
        return (super().stage_cost(x, u, bp) + mpf(self.QUARTIC) * F._m(x[3]) ** 4
                - F._m(bp) * (mp.log(L - p) + mp.log(p + L)))

    def stage_feasible(self, x, u):
        L, p = mpf(self.LIMIT), F._m(x[0])
        return super().stage_feasible(x, u) and p - L <= 0 and -p - L <= 0

    def box_margin(self, X, U):
        L = mpf(self.LIMIT)
        return min(super().box_margin(X, U), float(min(abs(abs(F._m(x[0])) - L) for x in X[:-1]) / L))


def _total_cost(prob, X, U, bp, skip=None):
    """final cost + sum of the stage costs (stage `skip` left out: the power check)"""
    c = prob.final(X[-1])[0]
    for t in range(prob.N):
        if t != skip:
            c += prob.stage_cost(X[t], U[t], bp)
    return c


def _feasible(prob, X, U):
    return all(prob.stage_feasible(X[t], U[t]) for t in range(prob.N))


def _sweep(prob, X, U, bp, zero=()):
    """Derivatives of every stage in long double; the fields named in `zero` replaced by zeros"""
    per = [prob.derivs(X[t], U[t], bp) for t in range(prob.N)]
    out = []
    for i, f in enumerate(F.FIELDS):
        a = _ld([p[i] for p in per])
        out.append(np.zeros_like(a) if f in zero else a)
    return tuple(out)


def _f64(a):
    return np.array([float(v) for v in np.ravel(np.array(a, dtype=object))]).reshape(np.shape(a))


def _passes(prob, x0, u0, bp, n_pass, zero=(), skip_stage=None):
    """oracle.noc_oracle.ddp (D:98-186) at 50 digits / long double, stopped after n_pass backward
    passes -> list of per-pass dicts (fp64).  zero, skip_stage: the deliberate defects of the power
    checks (derivative fields dropped; a stage left out of the nominal cost)."""
    N = prob.N
    with mp.workdps(F.DPS):
        U = [np.array([F._m(v) for v in u], dtype=object) for u in np.asarray(u0, np.float64)]
        X = [np.array([F._m(v) for v in x0], dtype=object)]
        for t in range(N):                                               # D:102
            X.append(prob.step(X[t], U[t]))
        reg_param, reg_inc = LD(1), LD(2)                                # D:102-103
        it, out = 0, []
        while len(out) < n_pass:
            cost = _total_cost(prob, X, U, bp, skip_stage)               # D:109
            derivs = _sweep(prob, X, U, bp, zero)                        # D:112
            _, g, H = prob.final(X[-1])                                  # D:58-59
            Vx, Vxx = _ld(g), _ld(H)
            rp, r_inc, inner = reg_param, reg_inc, 0
            while True:
                info = {}
                k, Kg, pred, feas, Hu = ddp_bwd_ld(Vx, Vxx, derivs, rp, info=info)
                km, Km = _mp_array(k), _mp_array(Kg)
                TX, TU, xh = [], [], X[0]
                for t in range(N):                                       # D:73-90
                    uh = U[t] + km[t] + Km[t].dot(xh - X[t])
                    TX.append(xh)
                    TU.append(uh)
                    xh = prob.step(xh, uh)
                TX.append(xh)
                ok = _feasible(prob, TX, TU)
                new_cost = _total_cost(prob, TX, TU, bp) if ok else mp.inf   # D:121-125
                gain = (new_cost - cost) / _mpf(pred)                    # D:126-127
                success = bool(gain > 0) and bool(feas)                  # D:128
                if success:
                    c = 2 * gain - 1
                    rp = rp * _ld([max(mpf(1) / 3, 1 - c * (c * c))])[0]  # D:131
                    r_inc = LD(2)
                else:
                    rp = rp * reg_inc                                    # the OUTER reg_inc (D:132)
                    r_inc = 2 * r_inc                                    # D:133
                clipped = not (LD(1e-16) < rp < LD(1e16))
                rp = min(max(rp, LD(1e-16)), LD(1e16))                   # D:135
                inner += 1
                out.append(dict(
                    it=it, inner=inner, cost=float(cost), new_cost=float(new_cost),
                    pred=float(pred), gain=float(gain), success=success, rp=float(rp),
                    hu=float(np.max(np.abs(Hu))), TX=_f64(TX), TU=_f64(TU), feas=bool(feas),
                    pivot=info["min_eig"] / info["max_Quu"], box=prob.box_margin(TX, TU),
                    clipped=clipped, retry_cap=inner > 500))
                if success or inner > 500 or len(out) >= n_pass:         # D:147-152
                    break
            X, U, reg_param, reg_inc = TX, TU, rp, r_inc                 # D:154-162
            it += 1
    return out


# --------------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    name: str                 # family of the dynamics
    N: int
    bp: float
    seed: int
    frac: float
    row: int = -1             # >= 0: row of the family's twin batch
    traced: bool = False

    def __str__(self):
        return self.id


_BASE_SEED = {"pendulum": 7100, "cartpole": 7300, "linear2": 7500}
# cases moved on from the seed their place in the list gives them: {id: seeds skipped}
# (all five took an accepted step that changed the cost by less than 1e-3 of it: N = 1, 2 at
# bp = 1e-3 converge within three Newton-like passes, and `gain` is then a quotient of rounding)
_BUMP = {"pendulum-N1-bp0.001": 1, "pendulum-N2-bp0.001": 1, "cartpole-N1-bp0.001": 2,
         "linear2-N2-bp0.1": 1, "cartpole-twin-row1": 1}
# cases with a pass rejected at a finite gain <= -0.05 (tests/test_ddp_pass_cases.py::test_census)
FINITE_REJECT_CASES = ("pendulum-twin-row2",)


def _make_cases():
    cases, i = [], 0
    for name in F.NAMES:
        for N in HORIZONS[name]:
            for bp in BPS:
                cid = f"{name}-N{N}-bp{bp:g}"
                seed = _BASE_SEED[name] + 10 * len(cases) + _BUMP.get(cid, 0)
                cases.append(Case(cid, name, N, bp, seed, FRACS[(i // 2 + i) % len(FRACS)]))
                i += 1
    return tuple(cases)


def _make_twins():
    out = []
    for name in F.NAMES:
        for row in range(3):
            cid = f"{name}-twin-row{row}"
            seed = _BASE_SEED[name] + 1000 + row + 10 * _BUMP.get(cid, 0)
            out.append(Case(cid, name, TWIN_N[name], TWIN_BP, seed, FRACS[row], row=row))
    return tuple(out)


CASES = _make_cases()
TWIN_CASES = _make_twins()
TRACED_CASE = Case("cartpole_track_limit-N%d" % TRACED_N, "cartpole", TRACED_N, TRACED_BP,
                   7900 + _BUMP.get("cartpole_track_limit", 0), 0.9, traced=True)
BY_ID = {c.id: c for c in CASES + TWIN_CASES + (TRACED_CASE,)}


@functools.lru_cache(maxsize=None)
def twin_params(name):
    from noc import TrajectoryParams
    return TrajectoryParams(**{k: np.array(v) for k, v in F._TWIN[name].items()})


def case_row(case):
    """goal / wx / wu / wf / u_bound of the case as the kernel receives them"""
    if case.traced:
        return TracedCartpole(case.N).row
    if case.row >= 0:
        return F.family_rows(case.name, 3, twin_params(case.name))[case.row]
    return F.family_rows(case.name, 1)[0]


def start(case, rep=0):
    """(x0 (nx,), u0 (N, nu)) of a case; rep > 0: further starts of the same shape (the batch test)"""
    fam = F.ocp(case.name).family
    rng = np.random.default_rng([case.seed, rep])
    x0 = rng.uniform(-3.0, 3.0, size=fam.nx)
    if case.traced:   # the cart starts on the track and slowly enough to stay there for 1 s
        x0[0], x0[2] = rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1)
    ub = float(case_row(case)["u_bound"])
    return x0, case.frac * ub * rng.uniform(-1.0, 1.0, size=(case.N, fam.nu))


def problem(case, constants=None):
    if case.traced:
        return TracedCartpole(case.N)
    return Problem(case.name, case.N, case_row(case), constants)


_CACHE = {}


def reference_passes(name, x0, u0, bp, n_pass, params=None, *, row=0, traced=False, constants=None,
                     zero=(), skip_stage=None):
    """The first n_pass backward passes from (x0 (nx,), u0 (N, nu)) at barrier value bp: a list of
    per-pass dicts.  params (noc.TrajectoryParams) with row: that row's own problem.  Results are
    cached per distinct input."""
    x0, u0 = np.asarray(x0, np.float64), np.asarray(u0, np.float64)
    key = (name, x0.tobytes(), u0.tobytes(), float(bp), n_pass, id(params) if params is not None
           else None, row, traced, tuple(sorted((constants or {}).items())), tuple(zero), skip_stage)
    if key not in _CACHE:
        N = u0.shape[0]
        if traced:
            prob = TracedCartpole(N)
        else:
            rows = F.family_rows(name, row + 1 if params is None else len(np.atleast_1d(
                np.asarray(params.u_bound))), params)
            prob = Problem(name, N, rows[row], constants)
        _CACHE[key] = _passes(prob, x0, u0, bp, n_pass, zero, skip_stage)
    return _CACHE[key]


def case_passes(case, **defect):
    """reference_passes of a Case (K passes; computed once per session).  defect: constants, zero,
    skip_stage of the power checks."""
    x0, u0 = start(case)
    return reference_passes(case.name, x0, u0, case.bp, K,
                            twin_params(case.name) if case.row >= 0 else None,
                            row=max(case.row, 0), traced=case.traced, **defect)


def errors(got, ref, fields=SCALARS + ("TX", "TU")):
    """own_max_error of every numerically compared field of one pass: got / ref are per-pass dicts
    with SCALARS, TX, TU.  An infinite reference value must be matched as such (error 0 or inf)."""
    out = {}
    for f in fields:
        g, r = np.asarray(got[f], np.float64), np.asarray(ref[f], np.float64)
        if np.all(np.isfinite(r)):
            out[f] = F.own_max_error(g, r)
        else:
            out[f] = 0.0 if np.array_equal(g, r) else math.inf
    return out
