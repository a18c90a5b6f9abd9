"""Cases of the RK4-family tests (tests/test_integrator_cases.py on the CPU,
tests/test_integrator_gpu.py on the device): the three families of tests/integrator_families.py at
dt = 0.05.

The reference of every comparison is the torch restatement (integrator_families.torch_ocp: the
ODE through oracle.problems.discretize_dynamics(ode, dt, 1)) under torch.func autodiff and the
numpy loops of oracle/noc_oracle.py.

Points: POINTS_B x POINTS_N = 8 generic points per family, laid out as POINTS_B trajectories of
POINTS_N stages so that compute_derivatives takes them as they are: states away from rest (angles
over more than a period, rates of order 1), u != 0, and in every trajectory one stage within 1e-6
(relative) of the control bound and one within 1e-3.

Whole solves: starts near the hanging rest state whose oracle loops converge, reach the control
bound, and keep every decision (trial feasibility, gain > 0, the stopping test) a relative MARGIN
from its threshold: the margin tests/multi_control_cases.py sets for registered-family solves.
The recorded counts are re-derived by tests/test_integrator_cases.py.
"""
import functools
import os

import numpy as np

import integrator_families as IF

DT = IF.DT
NAMES = list(IF.SPECS)
CART, PEND, VEC = NAMES
SHAPE = {n: (IF.SPECS[n][1]["nx"], IF.SPECS[n][1]["nu"]) for n in NAMES}
ANGLE = {CART: 1, PEND: 0, VEC: 1}      # the wrapped state
FIELDS = ("cx", "cu", "cxx", "cuu", "cxu", "fx", "fu", "fxx", "fuu", "fxu")
DYN_FIELDS = ("fx", "fu", "fxx", "fuu", "fxu")
POINTS_B, POINTS_N = 2, 4
POINTS_BP = 0.1
_SEED = {CART: 5100, PEND: 5200, VEC: 5300}


@functools.lru_cache(maxsize=None)
def ocp(name, build=True, integrator="rk4"):
    return IF.register(name, DT, build=build, integrator=integrator)


@functools.lru_cache(maxsize=None)
def problem(name, integrator="rk4"):
    from oracle import noc_oracle as O
    return O.NumpyProblem(IF.torch_ocp(name, DT, integrator))


def bound(name):
    return float(IF.SPECS[name][1]["u_bound"])


@functools.lru_cache(maxsize=None)
def points(name):
    """X (POINTS_B, POINTS_N + 1, nx), U (POINTS_B, POINTS_N, nu), lambda (POINTS_B, POINTS_N, nx)"""
    rng = np.random.default_rng(_SEED[name])
    nx, nu = SHAPE[name]
    X = rng.uniform(0.5, 2.0, size=(POINTS_B, POINTS_N + 1, nx)) * rng.choice([-1.0, 1.0], size=(
        POINTS_B, POINTS_N + 1, nx))
    X[..., ANGLE[name]] = rng.uniform(-7.0, 7.0, size=(POINTS_B, POINTS_N + 1))
    ub = bound(name)
    U = ub * rng.uniform(0.2, 0.9, size=(POINTS_B, POINTS_N, nu)) * rng.choice([-1.0, 1.0], size=(
        POINTS_B, POINTS_N, nu))
    U[:, 1] = ub * (1.0 - 1e-6)
    U[:, 2] = -ub * (1.0 - 1e-3)
    if nu > 1:   # the second control near the other side at another stage
        U[:, 1, 1] = 0.37 * ub
        U[:, 3, 1] = -ub * (1.0 - 1e-6)
    L = rng.normal(size=(POINTS_B, POINTS_N, nx))
    for a in (X, U, L):
        a.setflags(write=False)
    return X, U, L


@functools.lru_cache(maxsize=None)
def reference(name, integrator="rk4"):
    """torch.func at the points: the ten derivative fields (POINTS_B, POINTS_N, ...), `step`, and
    the lambda-contracted Hessian blocks hxx, huu, hxu"""
    X, U, L = points(name)
    prob = problem(name, integrator)
    out = {k: [] for k in FIELDS + ("step",)}
    for b in range(POINTS_B):
        for k, v in zip(FIELDS, prob.derivatives(X[b], U[b], POINTS_BP)):
            out[k].append(v)
        out["step"].append(np.stack([prob.dynamics(x, u) for x, u in zip(X[b, :-1], U[b])]))
    out = {k: np.stack(v) for k, v in out.items()}
    out["hxx"] = np.einsum("bki,bkijl->bkjl", L, out["fxx"])
    out["huu"] = np.einsum("bki,bkijl->bkjl", L, out["fuu"])
    out["hxu"] = np.einsum("bki,bkijl->bkjl", L, out["fxu"])
    return out


# --------------------------------------------------------------------------------------------------
# csrc/rk4_map.h on the host: the generated ODE functions + the composition behind a main
# --------------------------------------------------------------------------------------------------
HOST_MAIN = r"""
#include <cstdio>
struct Ode {
  static void rhs(const double* x, const double* u, double* f) { noc::gen::custom_ode(x, u, f); }
  static void rhs_jac(const double* x, const double* u, double* J) { noc::gen::custom_ode_jac(x, u, J); }
  static void rhs_hess_l(const double* x, const double* u, const double* l, double* H) {
    noc::gen::custom_ode_hess_l(x, u, l, H);
  }
};
static void put(const char* tag, const double* v, int n) {
  std::printf("%s", tag);
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}
int main(int argc, char** argv) {
  std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  int n;
  double h;
  if (!f || std::fscanf(f, "%d %lf", &n, &h) != 2) return 2;
  for (int p = 0; p < n; ++p) {
    double x[CASE_NX], u[CASE_NU], l[CASE_NX];
    for (int i = 0; i < CASE_NX; ++i) if (std::fscanf(f, "%lf", &x[i]) != 1) return 2;
    for (int i = 0; i < CASE_NU; ++i) if (std::fscanf(f, "%lf", &u[i]) != 1) return 2;
    for (int i = 0; i < CASE_NX; ++i) if (std::fscanf(f, "%lf", &l[i]) != 1) return 2;
    double xn[CASE_NX], fx[CASE_NX * CASE_NX], fu[CASE_NX * CASE_NU];
    double hxx[CASE_NX * CASE_NX] = {}, huu[CASE_NU * CASE_NU] = {}, hxu[CASE_NX * CASE_NU] = {};
    noc::rk4::step<Ode, CASE_NX, CASE_NU>(h, x, u, xn); put("step", xn, CASE_NX);
    noc::rk4::jac<Ode, CASE_NX, CASE_NU>(h, x, u, fx, fu); put("fx", fx, CASE_NX * CASE_NX); put("fu", fu, CASE_NX * CASE_NU);
    noc::rk4::add_hess_l<Ode, CASE_NX, CASE_NU>(h, x, u, l, hxx, huu, hxu);
    put("hxx", hxx, CASE_NX * CASE_NX); put("huu", huu, CASE_NU * CASE_NU); put("hxu", hxu, CASE_NX * CASE_NU);
  }
  return 0;
}
"""


def rk4_map_source():
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(os.path.dirname(here), "ip-parallel-optimal-control_amd", "csrc", "rk4_map.h")
    with open(path) as fh:
        return fh.read().replace("#pragma once", "")


def run_on_host(cxx, workdir, header, name):
    """compile the generated header + rk4_map.h for the host and evaluate the points; returns a
    dict of (POINTS_B, POINTS_N, ...) arrays"""
    import subprocess
    nx, nu = SHAPE[name]
    X, U, L = points(name)
    body = "\n".join(l for l in header.splitlines() if not l.lstrip().startswith(("#include", "#pragma")))
    src, exe, pts = (os.path.join(workdir, n) for n in ("rk4_host.cpp", "rk4_host", "points.txt"))
    with open(src, "w") as fh:
        fh.write(f"#include <cmath>\n#include <math.h>\n#define NOC_DEV static inline\n"
                 f"#define CASE_NX {nx}\n#define CASE_NU {nu}\n" + body + rk4_map_source() + HOST_MAIN)
    subprocess.run([cxx, "-O1", "-std=c++17", "-D_GNU_SOURCE", "-ffp-contract=off", "-o", exe, src,
                    "-lm"], check=True)
    with open(pts, "w") as fh:
        fh.write(f"{POINTS_B * POINTS_N} {DT!r}\n")
        for b in range(POINTS_B):
            for k in range(POINTS_N):
                fh.write(" ".join(repr(float(v)) for v in (*X[b, k], *U[b, k], *L[b, k])) + "\n")
    text = subprocess.run([exe, pts], check=True, capture_output=True, text=True).stdout
    shapes = dict(step=(nx,), fx=(nx, nx), fu=(nx, nu), hxx=(nx, nx), huu=(nu, nu), hxu=(nx, nu))
    got = {k: [] for k in shapes}
    for line in text.splitlines():
        tag, *vals = line.split()
        got[tag].append(np.array([float(v) for v in vals]).reshape(shapes[tag]))
    return {k: np.stack(v).reshape((POINTS_B, POINTS_N) + shapes[k]) for k, v in got.items()}


# --------------------------------------------------------------------------------------------------
# whole solves
# --------------------------------------------------------------------------------------------------
MARGIN = 1e-6        # tests/multi_control_cases.py: MARGIN
ACTIVE = 1e-2        # the bound counts as active where a control is within 1 % of it
SOLVE_N, SOLVE_B = 40, 3
DDP_N, DDP_B = 30, 2
WIDE_N, WIDE_B = 129, 1   # the smallest N > 128 (the GPU test asserts noc_ipm_solve_supported)
LINEARISE_N = 37          # no multiple of a lane count
_REST = {CART: [0.0, 0.0, 0.0, 0.0], PEND: [0.1, -0.1, 0.0], VEC: [0.0, 0.0, 0.0, 0.0]}


def solve_start(name, Nn, Bt, seed):
    """(x0 (Bt, nx), u0 (Bt, Nn, nu)) of a whole-solve case"""
    rng = np.random.default_rng(seed)
    nx, nu = SHAPE[name]
    x0 = np.array(_REST[name]) + 0.01 * rng.normal(size=(Bt, nx))
    u0 = 0.1 * rng.normal(size=(Bt, Nn, nu))
    return x0, u0


def shape_of(mode):
    return {"par": (SOLVE_N, SOLVE_B), "seq": (SOLVE_N, SOLVE_B), "ddp": (DDP_N, DDP_B),
            "wide": (WIDE_N, WIDE_B)}[mode]


# (name, mode) -> (seed, iterations per trajectory, KKT solves / backward passes per trajectory
# (None for seq)): filled from the oracle, re-derived by tests/test_integrator_cases.py
STARTS = {
    (CART, "par"): (41, (136, 111, 113), (211, 168, 176)),
    (PEND, "par"): (41, (74, 80, 75), (94, 103, 96)),
    (VEC, "par"): (41, (146, 165, 161), (203, 236, 219)),
    (CART, "seq"): (41, (185, 139, 145), None),
    (PEND, "seq"): (41, (90, 103, 94), None),
    (VEC, "seq"): (41, (194, 221, 201), None),
    (CART, "ddp"): (41, (108, 94), (203, 169)),
    (PEND, "ddp"): (41, (66, 63), (97, 93)),
    (CART, "wide"): (41, (254,), (432,)),
}


def wide_oracle_controls():
    """the par oracle's controls (WIDE_B, WIDE_N, nu) from the "wide" start, recorded under
    tests/golden/ (tests/test_integrator_cases.py holds them against a fresh oracle run)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "integrator_wide.npz")
    with np.load(path) as z:
        return z[CART]


def linearise_start(name):
    """x0 (POINTS_B, nx), U (POINTS_B, LINEARISE_N, nu) of the fused-linearise case: moving states,
    controls up to 0.6 of the bound"""
    rng = np.random.default_rng(_SEED[name] + 50)
    nx, nu = SHAPE[name]
    x0 = 0.5 * rng.normal(size=(POINTS_B, nx))
    U = 0.6 * bound(name) * rng.uniform(-1.0, 1.0, size=(POINTS_B, LINEARISE_N, nu))
    return x0, U


def oracle_run(name, mode, seed, keep_u=None):
    """The oracle loop of one whole-solve case: (iterations, solves or passes or None per
    trajectory, the smallest relative margin of any decision, the largest |u| / bound, the
    largest |Hu|_inf at which a trajectory's last barrier level stopped).  Watched
    decisions as in tests/test_multi_control_cases.py: the trial's feasibility (largest constraint
    value against 0), gain > 0 (|gain| itself) and the stopping test |Hu|_inf < 1e-4 (against
    1e-4).  keep_u: a list that receives the controls per trajectory."""
    from oracle import noc_oracle as O
    kind = "par" if mode == "wide" else mode
    Nn, Bt = shape_of(mode)
    x0, u0 = solve_start(name, Nn, Bt, seed)
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

    last_hu = []

    def hu(v):
        margins.append(abs(float(v) - 1e-4) / 1e-4)
        last_hu[:] = [float(v)]

    def gain(t):
        if np.isfinite(t["new_cost"]):
            margins.append(abs(t["gain"]))

    its, cnt, reach, stop = [], [], 0.0, 0.0
    for b in range(Bt):
        prob = Watch(IF.torch_ocp(name, DT))
        if kind == "par":
            tr = []
            Ub, it, s = O.par_interior_point_optimal_control(prob, u0[b], x0[b], terminal="stage0",
                                                             trace=tr)
            for t in tr:
                hu(t["hu"])
                gain(t)
        elif kind == "ddp":
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
                Ub, it, s = O.interior_point_ddp(prob, u0[b], x0[b])
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
                Ub, it = O.seq_interior_point_optimal_control(prob, u0[b], x0[b])
            finally:
                O.seq_solution = orig
            s = None
        its.append(int(it))
        cnt.append(None if s is None else int(s))
        reach = max(reach, float(np.max(np.abs(Ub))) / bound(name))
        stop = max(stop, last_hu[0])
        if keep_u is not None:
            keep_u.append(np.asarray(Ub))
    return its, cnt, float(min(margins)), reach, stop
