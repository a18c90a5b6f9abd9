"""register_family(integrator="rk4") on the CPU, and the preconditions of
tests/test_integrator_gpu.py (cases: tests/integrator_cases.py).

  * The argument errors; the host dynamics are noc.utils.runge_kutta bit for bit; the Euler header
    has no integrator line and the RK4 header is that text plus the one constant, in a build
    directory of its own.
  * csrc/rk4_map.h composed with the generated ODE functions, compiled for the host behind a
    stand-alone main, against torch.func on oracle.problems.discretize_dynamics(ode, dt, 1) at the
    8 points of every family: step, fx, fu and the lambda-contracted Hessian blocks for random
    lambda, 1e-12 of the field's own maximum per trajectory (both sides are fp64 evaluations of
    the same smooth map in some 10^3 operations: 10^3 eps = 2e-13).  Observed (pytest -s): at most
    4.4e-16 in any field of any family.
  * The GPU tests cannot pass on Euler code: at every point the RK4 and the Euler reference differ
    by more than 1e-4 in max-norm in the step, fx, fu, fxx, the whole second-derivative tensor and
    the whole lambda-contracted Hessian.  The fuu and fxu blocks taken alone cannot differ by that
    much for these ODEs at dt = 0.05: the cart-pole and the actuated pendulum are affine in u, so
    their Euler fuu is 0 and their RK4 fuu is of order h^5 (largest entry at the points: 9.0e-7 /
    3.2e-8; the pendulum's fxu: 5.1e-5), whatever the point.  Those blocks are held to what the
    GPU comparison needs instead: a difference of at least 10 times its tolerance of 1e-10
    (observed smallest: fuu 2.6e-7 / 5.5e-9 / 5.8e-5, fxu 1.6e-4 / 8.9e-6 / 1.3e-3 for cart-pole /
    pendulum / vectored cart-pole).
  * An entry of A that the ODE's pattern calls constant moves between two points: under RK4 the
    ODE's pattern is not the map's (csrc/block_struct.h).
  * Every whole-solve start converges on the oracle, ends with a control within 1 % of its bound,
    keeps the relative margin of 1e-6 at every decision and gives the recorded counts.
"""
import os
import shutil

import numpy as np
import pytest

import integrator_cases as C
import integrator_families as IF

HOST_TOL = 1e-12
GPU_DERIV_TOL = 1e-10


def _err(got, ref):
    """max |got - ref| over the reference's own maximum, per trajectory (no floor of 1)"""
    return max(float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref))


# --------------------------------------------------------------------------------------------------
# 1. the interface
# --------------------------------------------------------------------------------------------------
def _never_traced(state, action):
    raise AssertionError("the dynamics were traced before the arguments were checked")


def test_argument_errors_come_before_any_tracing():
    from noc import _lib, families
    spec = IF.SPECS[C.PEND][1]
    with pytest.raises(_lib.NocError, match="integrator"):
        families.register_family("bad", _never_traced, dt=0.05, integrator="heun", build=False, **spec)
    with pytest.raises(_lib.NocError, match="discrete"):
        families.register_family("bad", _never_traced, dt=0.05, integrator="rk4", discrete=True,
                                 build=False, **spec)
    for dt in (0.0, -0.05):
        with pytest.raises(_lib.NocError, match="dt > 0"):
            families.register_family("bad", _never_traced, dt=dt, integrator="rk4", build=False, **spec)
    with pytest.raises(_lib.NocError, match="integrator"):
        families.generate_header("bad", _never_traced, 3, 1, False, None, "midpoint")


@pytest.mark.parametrize("name", C.NAMES)
def test_host_dynamics_are_runge_kutta_bit_for_bit(name):
    from noc.utils import euler, runge_kutta
    ode = IF.SPECS[name][0]
    X, U, _ = C.points(name)
    rk, eu = C.ocp(name, build=False), C.ocp(name, build=False, integrator="euler")
    for x, u in zip(X[:, :-1].reshape(-1, X.shape[-1]), U.reshape(-1, U.shape[-1])):
        assert np.array_equal(rk.dynamics(x, u), runge_kutta(x, u, ode, C.DT))
        assert np.array_equal(eu.dynamics(x, u), euler(ode, C.DT)(x, u))
    assert rk.family.dt == C.DT and rk.family.kind == eu.family.kind


@pytest.mark.parametrize("name", C.NAMES)
def test_headers_differ_in_the_integrator_constant_alone(name):
    from noc import families
    ode, spec = IF.SPECS[name]
    nx, nu = C.SHAPE[name]
    plain = families.generate_header(name, ode, nx, nu, False)
    assert families.generate_header(name, ode, nx, nu, False, None, "euler") == plain
    assert "Integrator" not in plain     # the text of a family registered before the argument existed
    rk = families.generate_header(name, ode, nx, nu, False, None, "rk4")
    a, b = plain.splitlines(), rk.splitlines()
    extra = [l for l in b if l not in a]
    assert len(b) == len(a) + 1 and len(extra) == 1
    assert extra[0].startswith("constexpr int kCustomIntegrator = 1;")
    assert [l for l in b if l != extra[0]] == a
    assert b.index(extra[0]) == next(i for i, l in enumerate(a) if "kCustomDiscrete" in l) + 1
    # ... so the ODE's traced functions are exactly the Euler family's, in another build directory
    assert families.build_dir(name, rk, nx, nu) != families.build_dir(name, plain, nx, nu)
    assert os.path.dirname(C.ocp(name, build=False).family.lib_path) == families.build_dir(name, rk, nx, nu)


# --------------------------------------------------------------------------------------------------
# 2. the composition on the host
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_rk4_map_on_the_host_matches_autodiff(name, tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    from noc import families
    nx, nu = C.SHAPE[name]
    hdr = families.generate_header(name, IF.SPECS[name][0], nx, nu, False, None, "rk4")
    got = C.run_on_host(cxx, str(tmp_path), hdr, name)
    ref = C.reference(name)
    assert C.POINTS_B * C.POINTS_N >= 6
    for k in ("step", "fx", "fu", "hxx", "huu", "hxu"):
        assert got[k].shape == ref[k].shape, k
        err = _err(got[k], ref[k])
        print(f"observed host rk4_map vs torch.func [{name}] {k} {err:.1e}")
        assert err < HOST_TOL, (k, err)


@pytest.mark.parametrize("name", C.NAMES)
def test_points_are_generic(name):
    X, U, _ = C.points(name)
    ub = C.bound(name)
    assert np.all(np.abs(U) < ub) and np.all(np.abs(U) > 0.1 * ub)
    rel = (ub - np.abs(U)) / ub
    assert np.all((rel < 2e-6).any(axis=(1, 2))) and np.all((rel < 2e-3).any(axis=(1, 2)))
    assert np.all(np.abs(np.delete(X, C.ANGLE[name], axis=-1)) >= 0.5)   # away from rest
    assert np.ptp(X[..., C.ANGLE[name]]) > 2 * np.pi
    prob = C.problem(name)
    for b in range(C.POINTS_B):
        assert prob.feasible(X[b], U[b])


# --------------------------------------------------------------------------------------------------
# 3. Euler code cannot pass the GPU tests
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_rk4_and_euler_differ_at_every_point(name):
    rk, eu = C.reference(name), C.reference(name, "euler")
    n = C.POINTS_B * C.POINTS_N

    def gap(k):
        return np.abs(rk[k] - eu[k]).reshape(n, -1).max(axis=1)

    for k in ("step", "fx", "fu", "fxx"):
        print(f"observed RK4 - Euler [{name}] {k}: smallest over the points {gap(k).min():.2e}")
        assert np.all(gap(k) > 1e-4), (k, gap(k))
    second = np.maximum(np.maximum(gap("fxx"), gap("fxu")), gap("fuu"))
    contracted = np.maximum(np.maximum(gap("hxx"), gap("hxu")), gap("huu"))
    assert np.all(second > 1e-4) and np.all(contracted > 1e-4), (second, contracted)
    for k in ("fuu", "fxu"):   # see the module docstring: of order h^5 / h^3 for these ODEs
        print(f"observed RK4 - Euler [{name}] {k}: smallest over the points {gap(k).min():.2e}, "
              f"largest RK4 entry {np.abs(rk[k]).max():.2e}")
        assert np.all(gap(k) > 10 * GPU_DERIV_TOL * max(1.0, float(np.abs(rk[k]).max()))), (k, gap(k))
    # the costs are the same functions
    for k in ("cx", "cu", "cxx", "cuu", "cxu"):
        assert np.array_equal(rk[k], eu[k]), k


@pytest.mark.parametrize("name", C.NAMES)
def test_an_entry_the_ode_pattern_calls_constant_moves(name):
    from noc import families
    nx, nu = C.SHAPE[name]
    hdr = families.generate_header(name, IF.SPECS[name][0], nx, nu, False, None, "rk4")
    line = next(l for l in hdr.splitlines() if "custom_jac_var[" in l)
    var = np.array([int(v) for v in line[line.index("{") + 1:line.index("}")].split(",")])
    const_A = ~var.reshape(nx, nx + nu)[:, :nx].astype(bool)
    assert const_A.any()
    rk, eu = C.reference(name), C.reference(name, "euler")
    A, Ae = rk["fx"].reshape(-1, nx, nx), eu["fx"].reshape(-1, nx, nx)
    assert np.all(np.ptp(Ae, axis=0)[const_A] == 0.0)          # constants of the Euler map
    moved = np.ptp(A, axis=0) * const_A
    i, j = np.unravel_index(np.argmax(moved), moved.shape)
    print(f"observed [{name}]: A[{i}][{j}] is constant in the ODE's pattern and moves by {moved[i, j]:.2e}")
    assert moved[i, j] > 1e-6
    if name == C.CART:   # the row xdot = v: d x+ / d theta is 0 under Euler
        assert const_A[0, 1] and np.all(Ae[:, 0, 1] == 0.0) and np.ptp(A[:, 0, 1]) > 1e-6


# --------------------------------------------------------------------------------------------------
# 4. the whole-solve starts
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", sorted(C.STARTS))
def test_solve_starts_on_the_oracle(name, mode):
    seed, iters, counts = C.STARTS[(name, mode)]
    keep = []
    its, cnt, margin, reach, stop = C.oracle_run(name, mode, seed, keep_u=keep)
    print(f"observed oracle [{name},{mode}] seed {seed}: iterations {its}, counts {cnt}, smallest "
          f"decision margin {margin:.2e}, largest |u| / bound {reach:.6f}, |Hu| at the stop {stop:.2e}")
    assert stop < 1e-4                      # converged: the last barrier level met the stopping test
    assert all(i < 1000 for i in its)
    assert 1.0 - C.ACTIVE < reach < 1.0     # the bound is active at some stage
    assert margin >= C.MARGIN, margin
    assert its == list(iters)
    if counts is not None:
        assert cnt == list(counts)
    if mode == "wide":   # the controls the GPU test compares with (too long a loop to repeat there)
        assert np.max(np.abs(np.stack(keep) - C.wide_oracle_controls())) < 1e-9


def test_every_consumer_has_a_start():
    assert {m for _, m in C.STARTS} == {"par", "seq", "ddp", "wide"}
    assert {n for n, m in C.STARTS if m in ("par", "seq")} == set(C.NAMES)
    assert {n for n, m in C.STARTS if m == "ddp"} == {C.CART, C.PEND}
    assert [n for n, m in C.STARTS if m == "wide"] == [C.CART]
    assert C.SOLVE_B <= 4 and C.SOLVE_N <= 40 and C.DDP_N <= 40 and C.LINEARISE_N % 8 != 0
