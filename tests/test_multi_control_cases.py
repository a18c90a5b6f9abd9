"""CPU preconditions of tests/test_multi_control_gpu.py (tests/multi_control_cases.py).

  * Two independent derivations agree: at every generated point the fp64 torch.func oracle on the
    torch restatement (tests/custom_families.py) and the 50-digit mpmath reference agree within
    1e-13 per field, relative to the field's own maximum over a trajectory (no floor of 1); this
    licenses the GPU tolerance of 1e-12.  Observed worst agreement per field over the three
    families (printed, pytest -s):
      cx 7.4e-17  cu 2.2e-16  cxx 1.7e-16  cuu 2.1e-16  cxu 8.7e-17  fx 2.3e-16  fu 1.7e-16
      fxx 2.4e-16  fuu 2.7e-16  fxu 4.0e-16  step 1.2e-16  final grad 0  cost 1.7e-16
    and of the host-compiled generated code against mpmath: at most 2.4e-16 in any function.
  * The structure the families were written for is there at the points: two distinct fu columns,
    fxu non-zero in both (all) control columns, an fuu off-diagonal (vectored cart-pole) or
    diagonal (triple drive), a non-diagonal cuu, a non-zero second cxu column and constant as well
    as varying cost-Hessian entries (reaction pendulum), near-bound and near-coupled stages.
  * Every point is feasible by the mpmath constraints.
  * The generated device code, compiled for the host behind a stand-alone main, reproduces the
    mpmath reference at the GPU tolerance for the three families and for a function zoo (every
    _codegen._UFUNCS entry, powers 1..9, -1..-8, +-1/2, 3/2, 1/3 and `%`): the generator is not the
    suspect when a kernel fails.
  * The whole-solve starts of the GPU tests keep a relative margin of 1e-6 at every decision of the
    oracle loop (trial feasibility, gain > 0, the stopping test; Quu's definiteness is discrete and
    not watched), the oracle's counts are the recorded ones, and they do not change when the
    start controls move by 1e-14 (relative) either way.
"""
import shutil

import numpy as np
import pytest

import multi_control_cases as C

TOL = 1e-13
GPU_TOL = 1e-12


def _problem(name, dt=C.DT):
    from oracle import noc_oracle as O
    return O.NumpyProblem(C.torch_ocp(name, dt))


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_agrees_with_the_mpmath_reference(name):
    X, U, bp = C.generic_case(name)
    ref = C.reference_derivatives(name)
    cost, _ = C.total_cost(name, X, U, bp)
    _, g, H = C.final_grad_hess(name, X[:, -1])
    prob = _problem(name)
    worst = {}
    for b in range(C.B):
        d = prob.derivatives(X[b], U[b], bp[b])
        for k, v in zip(C.FIELDS, d):
            worst[k] = max(worst.get(k, 0.0), C.own_max_error(v, ref[k][b]))
        og, oH = prob.final_grad_hess(X[b, -1])
        worst["final_grad"] = max(worst.get("final_grad", 0.0), C.own_max_error(og, g[b]))
        worst["final_hess"] = max(worst.get("final_hess", 0.0), C.own_max_error(oH, H[b]))
        oc = prob.total_cost(X[b], U[b], bp[b])
        worst["cost"] = max(worst.get("cost", 0.0), abs(oc - cost[b]) / abs(cost[b]))
        on = np.stack([prob.dynamics(x, u) for x, u in zip(X[b, :-1], U[b])])
        worst["step"] = max(worst.get("step", 0.0), C.own_max_error(on, ref["step"][b]))
    print(f"observed oracle vs mpmath [{name}]:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < TOL, (k, v)


def test_structure_of_the_vectored_cartpole():
    ref = C.reference_derivatives(C.A_NAME)
    fu, fxu, fuu = ref["fu"], ref["fxu"], ref["fuu"]
    assert np.all(np.abs(fu[..., 2:, 0]) > 0) and np.all(np.abs(fu[..., 2:, 1]) > 0)
    # two distinct columns: not parallel at any point
    cross = fu[..., 2, 0] * fu[..., 3, 1] - fu[..., 3, 0] * fu[..., 2, 1]
    assert np.all(np.abs(cross) > 1e-9)
    for j in range(2):
        assert np.all(np.max(np.abs(fxu[..., :, :, j]), axis=(-1, -2)) > 0), j
    assert np.all(np.max(np.abs(fuu[..., :, 0, 1]), axis=-1) > 0)
    assert np.array_equal(fuu[..., 0, 1], fuu[..., 1, 0])
    cuu = ref["cuu"]
    assert not np.any(cuu[..., 0, 1]) and np.all(cuu[..., 0, 0] != cuu[..., 1, 1])
    assert not np.any(ref["cxu"])
    assert C.SPEC[C.A_NAME]["wu"][0] != C.SPEC[C.A_NAME]["wu"][1]
    assert C.SPEC[C.A_NAME]["u_bound"] > 0 and C.SPEC[C.A_NAME]["wrap_index"] == 1


def test_structure_of_the_reaction_pendulum():
    ref = C.reference_derivatives(C.B_NAME)
    assert np.all(np.abs(ref["cuu"][..., 0, 1]) > 0)               # the coupled barrier + cross term
    assert np.array_equal(ref["cuu"][..., 0, 1], ref["cuu"][..., 1, 0])
    assert np.all(np.abs(ref["cxu"][..., 1, 1]) > 0) and np.all(np.abs(ref["cxu"][..., 0, 1]) > 0)
    assert not np.any(ref["cxu"][..., :, 0])
    assert np.ptp(ref["cxu"][..., 1, 1]) < 1e-15 and np.ptp(ref["cxu"][..., 0, 1]) > 1e-4
    assert np.ptp(ref["cxx"][..., 2, 2]) > 0                       # the state constraint's barrier
    assert np.all(np.abs(ref["fuu"][..., 2, 0, 1]) > 0) and np.all(np.abs(ref["fxu"][..., 1, 0, 1]) > 0)
    # the generated structure: both halves of custom_cost_hess_var / _const are in use
    from noc import families
    import custom_families as CF
    hdr = families.generate_header("reaction_pendulum", CF.reaction_pendulum_ode, 3, 2, False,
                                   (CF.reaction_pendulum_stage_cost, CF.reaction_pendulum_final_cost,
                                    CF.reaction_pendulum_constraints))
    line = next(l for l in hdr.splitlines() if "custom_cost_hess_var[" in l)
    var = [int(v) for v in line[line.index("{") + 1:line.index("}")].split(",")]
    assert len(var) == 9 + 4 + 6 and 0 < sum(var) < len(var)
    Q, R, M = np.array(var[:9]).reshape(3, 3), np.array(var[9:13]).reshape(2, 2), np.array(var[13:]).reshape(3, 2)
    assert R.all() and M[0, 1] == 1 and M[1, 1] == 0 and not M[:, 0].any()
    assert Q[0, 0] == 1 and Q[1, 1] == 1 and Q[2, 2] == 1 and Q[0, 1] == 0 and Q[1, 2] == 0
    cline = next(l for l in hdr.splitlines() if "custom_cost_hess_const[" in l)
    cst = [float(v) for v in cline[cline.index("{") + 1:cline.index("}")].split(",")]
    assert cst[13 + 3] == CF.RP_CROSS_VEL and cst[1] == 0.0


def test_structure_of_the_triple_drive_pendulum():
    ref = C.reference_derivatives(C.C_NAME)
    assert C.SHAPE[C.C_NAME] == (2, 3)
    assert np.all(np.abs(ref["fuu"][..., 1, 1, 1]) > 0)             # tanh''
    off = ~np.eye(3, dtype=bool)
    assert not np.any(ref["fuu"][..., off]) and not np.any(ref["fuu"][..., 1, 0, 0])
    assert np.all(np.abs(ref["fxu"][..., 1, 0, 2]) > 0) and not np.any(ref["fxu"][..., 1, 0, :2])
    fu = ref["fu"][..., 1, :]
    assert np.all(np.abs(fu) > 0)
    assert len(set(C.SPEC[C.C_NAME]["wu"])) == 3
    d = np.stack([ref["cuu"][..., j, j] for j in range(3)], axis=-1)
    assert np.all(d > 0) and not np.any(ref["cuu"][..., off])


@pytest.mark.parametrize("name", C.NAMES)
def test_points_are_feasible_and_near_the_bounds(name):
    X, U, bp = C.generic_case(name)
    worst = C.max_constraint(name, X, U)
    assert np.all(worst < 0.0), worst
    ub = C.control_bounds(name)
    assert np.all(np.abs(U) < ub)
    rel = (ub - np.abs(U)) / ub
    for j in range(U.shape[-1]):   # every control: a stage within 1e-6 and one within 1e-9
        assert np.all((rel[..., j] < 2e-6).sum(axis=1) >= 1), j
        assert np.all((rel[..., j] < 2e-9).sum(axis=1) >= 1), j
    assert list(bp) == [0.1, 1e-4, 1e-8]
    th = X[..., {C.A_NAME: 1}.get(name, 0)]
    assert th.max() > 2 * C.TWO_PI and th.min() < -2 * C.TWO_PI    # several periods
    assert np.median(np.abs(X[..., -1])) > 1.0                      # away from rest
    if name == C.B_NAME:
        import custom_families as CF
        gap = 1.0 - (U[..., 0] + U[..., 1]) / CF.RP_SUPPLY
        for k, want in C.COUPLED_STAGES.items():
            assert np.all((gap[:, k] > 0) & (gap[:, k] < 2 * want)), (k, gap[:, k])
        assert np.all(1.0 - np.abs(X[:, C.TORQUE_STAGE, 2]) / CF.RP_TORQUE < 2e-6)


# --------------------------------------------------------------------------------------------------
# the generated code on the host
# --------------------------------------------------------------------------------------------------
def _host_compiler():
    return shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _check_host(what, got, ref, keys, groups):
    """keys against the reference at GPU_TOL of the key's own maximum over each group of points"""
    worst = {}
    for k in keys:
        for idx in groups:
            g = np.stack([got[i][k] for i in idx])
            r = np.stack([ref[i][k] for i in idx])
            worst[k] = max(worst.get(k, 0.0), C.own_max_error(g, r))
    print(f"observed host-compiled header vs mpmath [{what}]:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < GPU_TOL, (what, k, v)


_COST_KEYS = ("stage_cost", "cx", "cu", "cxx", "cuu", "cxu", "final_cost", "final_grad", "final_hess")


@pytest.mark.parametrize("name", C.NAMES)
def test_generated_header_on_the_host(name, tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    import custom_families as CF
    from noc import families
    nx, nu = C.SHAPE[name]
    traced = name == C.B_NAME
    costs = (CF.reaction_pendulum_stage_cost, CF.reaction_pendulum_final_cost,
             CF.reaction_pendulum_constraints) if traced else None
    ode = {C.A_NAME: CF.vectored_cartpole_ode, C.B_NAME: CF.reaction_pendulum_ode,
           C.C_NAME: CF.triple_drive_pendulum_ode}[name]
    hdr = families.generate_header(name, ode, nx, nu, False, costs)
    X, U, bp = C.generic_case(name)
    Xp, Up = X[:, :C.N].reshape(-1, nx), U.reshape(-1, nu)
    bpp = np.repeat(bp, C.N)
    L = np.random.default_rng(77).normal(size=Xp.shape)
    got = C.run_on_host(cxx, str(tmp_path), hdr, nx, nu, Xp, Up, L, bpp)
    assert len(got) == len(Xp)
    sc = (lambda x, u, b: C.stage_cost_terms(name, x, u, b)[0]) if traced else None
    fc = (lambda x: C.final_cost_value(name, x)) if traced else None
    ref = [C.host_reference(C.ode_functions(name), sc, fc, nx, nu, x, u, l, b)
           for x, u, l, b in zip(Xp, Up, L, bpp)]
    groups = [range(b * C.N, (b + 1) * C.N) for b in range(C.B)]
    _check_host(name, got, ref, ("ode", "jac", "hess_l") + (_COST_KEYS if traced else ()), groups)
    if traced:
        assert all(g["feasible"][0] == 1.0 for g in got)


def test_function_zoo_header_on_the_host(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    from noc import _codegen, families
    nx, nu = C.ZOO_SHAPE
    hdr = families.generate_header("zoo", C.zoo_ode, nx, nu, False,
                                   (C.zoo_stage_cost, C.zoo_final_cost, C.zoo_constraints))
    # the zoo is what it says: every ufunc of the tracer and the printer's power cases
    import inspect
    src = inspect.getsource(C.zoo_ode)
    for fn in _codegen._UFUNCS:
        assert f"np.{fn}(" in src, fn
    assert "pow(" in hdr and "sqrt(" in hdr and "noc_pymod(" in hdr
    Xp, Up = C.zoo_points()
    n = len(Xp)
    bpp = np.resize(C.BP, n)
    L = np.random.default_rng(78).normal(size=Xp.shape)
    got = C.run_on_host(cxx, str(tmp_path), hdr, nx, nu, Xp, Up, L, bpp)
    ref = [C.host_reference(C.zoo_ode_mp(), C.zoo_stage_cost_mp, C.zoo_final_cost_mp, nx, nu, x, u, l, b)
           for x, u, l, b in zip(Xp, Up, L, bpp)]
    _check_host("zoo", got, ref, ("ode", "jac", "hess_l") + _COST_KEYS, [range(n)])
    # the numpy callables themselves are the functions the reference restates
    for x, u, r in zip(Xp, Up, ref):
        assert C.own_max_error(C.zoo_ode(x, u), r["ode"]) < GPU_TOL
    assert all(g["feasible"][0] == 1.0 for g in got)


# --------------------------------------------------------------------------------------------------
# the whole-solve starts
# --------------------------------------------------------------------------------------------------
LAST_U = []    # the par oracle's controls of the last oracle_run, per trajectory


def oracle_run(name, mode, seed, perturb=0.0):
    """Run the oracle loop of one whole-solve case: (iterations, solves or passes or None per
    trajectory, the smallest relative margin of any decision).  Watched decisions: the trial's
    feasibility (largest constraint value against 0, in units of 1), gain > 0 (|gain| itself: an
    accepted step's gain is of order 1) and the stopping test |Hu|_inf < 1e-4 (against 1e-4)."""
    from oracle import noc_oracle as O
    ddp = mode == "ddp"
    Nn, Bt = (C.DDP_N, C.DDP_B) if ddp else (C.SOLVE_N, C.SOLVE_B)
    if mode == "wide":   # the par loop at the wide kernel's horizon
        Nn, mode = C.WIDE_N, "par"
    x0, u0 = C.solve_start(name, Nn, Bt, seed)
    u0 = u0 * (1.0 + perturb)
    margins = []

    class Watch(O.NumpyProblem):
        def __init__(self, t):
            super().__init__(t)
            self.base, self.after_feas, self.pred = None, False, None

        def total_cost(self, X, U, bp):
            c = super().total_cost(X, U, bp)
            if self.after_feas:
                if self.pred is not None:
                    margins.append(abs((c - self.base) / self.pred))
            else:
                self.base = c
            self.after_feas = False
            return c

        def feasible(self, X, U):
            g = float(np.max(self.pr.constraints_np(self.t, X[:-1], U)))
            margins.append(abs(g))
            self.after_feas = g <= 0
            return g <= 0

    def hu(v):
        margins.append(abs(float(v) - 1e-4) / 1e-4)

    def gain(t):
        if np.isfinite(t["new_cost"]):
            margins.append(abs(t["gain"]))

    its, cnt = [], []
    LAST_U.clear()
    for b in range(Bt):
        prob = Watch(C.torch_ocp(name, 1.0 / Nn))
        if mode == "par":
            tr = []
            Ub, it, s = O.par_interior_point_optimal_control(prob, u0[b], x0[b], terminal="stage0", trace=tr)
            LAST_U.append(Ub)
            for t in tr:
                hu(t["hu"])
                gain(t)
        elif ddp:
            orig = O.ddp

            def traced(p, U, x, bp, trace=None):
                tr = []
                out = orig(p, U, x, bp, trace=tr)
                for t in tr:
                    hu(t["hu"])
                    gain(t)
                return out
            O.ddp = traced
            try:
                _, it, s = O.interior_point_ddp(prob, u0[b], x0[b])
            finally:
                O.ddp = orig
        else:
            orig = O.seq_solution

            def watched(*a):
                out = orig(*a)
                hu(np.max(np.abs(out[4])))
                prob.pred = out[2]
                return out
            O.seq_solution = watched
            try:
                _, it = O.seq_interior_point_optimal_control(prob, u0[b], x0[b])
            finally:
                O.seq_solution = orig
            s = None
        its.append(int(it))
        cnt.append(None if s is None else int(s))
    return its, cnt, float(min(margins))


_STARTS = [(n, m) for n in C.NAMES for m in ("par", "seq", "ddp", "wide")]


@pytest.mark.parametrize("name,mode", _STARTS)
def test_solve_starts_keep_their_margin_and_counts(name, mode):
    seed, iters, counts = C.DDP_STARTS[name] if mode == "ddp" else C.SOLVE_STARTS[name][mode]
    its, cnt, margin = oracle_run(name, mode, seed)
    if mode == "wide":   # the stored controls of the GPU test are this oracle's (N = 129 is too
        # long a loop to repeat inside a GPU test)
        assert np.max(np.abs(np.stack(LAST_U) - C.wide_oracle_controls(name))) < 1e-9
    print(f"observed oracle [{name},{mode}] seed {seed}: iterations {its}, counts {cnt}, "
          f"smallest decision margin {margin:.2e}")
    assert margin >= C.MARGIN, margin
    assert its == list(iters)
    if counts is not None:
        assert cnt == list(counts)
    # the path itself is not at rounding level: these loops amplify a difference of a few ulps from
    # pass to pass (measured on the vectored cart-pole: a factor of ten every five DDP passes), so a
    # margin at each decision is not enough when there are hundreds of them; the oracle must count
    # the same from a start moved by PERTURB (some tens of ulps) either way
    for sign in (1.0, -1.0):
        its2, cnt2, _ = oracle_run(name, mode, seed, sign * C.PERTURB)
        assert (its2, cnt2) == (its, cnt), (sign, its2, cnt2)


def test_group_solve_refuses_the_shapes_it_cannot_run():
    """lanes = 1 needs nx dividing 64 and nu <= nx: (3, 2) and (2, 3) are refused, and so is the
    grouped tiled layout at (4, 2), the one of the three shapes that lanes = 1 accepts in the natural
    layout (noc_kkt_solve_tiled with lanes = 1; at (3, 2) and (2, 3) the refusal is checked through
    noc_kkt_solve); argument errors, before any launch (fake pointers)."""
    from noc import _lib
    args = (*([16] * 6), None, None, 16, None, None, None, None, 16, 16, 16, 16, 16, 16, None, None, None)
    for name in (C.B_NAME, C.C_NAME):
        lib = _lib.load_for(C.ocp(name).family)
        nx, nu = C.SHAPE[name]
        assert lib.noc_kkt_supported(nx, nu) == 1
        assert lib.noc_kkt_solve(nx, nu, 10, 4, 1, *args) < 0
        assert b"group solve" in lib.noc_last_error()
    lib = _lib.load_for(C.ocp(C.A_NAME).family)
    assert lib.noc_kkt_solve_tiled(4, 2, 10, 8, 1, *args) < 0 and b"grouped" in lib.noc_last_error()
    assert lib.noc_kkt_solve(4, 2, 10, 0, 1, *args) == 0    # (4, 2) itself is accepted (empty batch)
