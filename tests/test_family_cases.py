"""CPU preconditions of tests/test_families_generic_gpu.py (tests/family_cases.py).

  * Two independent derivations agree: on every generated point the fp64 torch.func oracle
    (oracle/problems.py) and the 50-digit mpmath reference agree within 1e-13 per field, relative
    to the field's own maximum over a trajectory (no floor of 1).  This licenses the GPU
    tolerance of 1e-12.  No generator range had to be narrowed for it.
  * Coverage is asserted, not hoped for: wrap regions, generic sin cos / velocity, near-bound
    controls.
  * The host wrap helpers (noc.utils.wrap_angle, noc/_codegen.py's noc_pymod compiled for the
    host) equal the reference's wrap_angle bit for bit on the edge list.
  * The new points see what the old ones cannot: the cart-pole's pole length times (1 + 1e-9)
    moves fxx by more than the GPU tolerance on the new points and by less than 1e-10 under the old
    max(1, .) measure on the rest-state rollout of test_api_gpu.
"""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import family_cases as C

TOL = 1e-13


def _oracle(name, case, b):
    """the torch oracle problem of trajectory b of a case"""
    from oracle import noc_oracle as O, problems as PR
    import traj_param_problems as TP
    base = {"pendulum": lambda: PR.pendulum_ocp(C.DT), "cartpole": lambda: PR.cartpole_ocp(C.DT),
            "linear2": lambda: PR.linear_ocp(1, C.LINEAR_STEP, constrained=True)}[name]()
    if case.params is None:
        return O.NumpyProblem(base)
    r = C.family_rows(name, C.B, case.params)[b]
    return O.NumpyProblem(TP._param_ocp(base, C.angle_index(name), r["goal"], r["wx"], r["wu"],
                                        r["wf"], r["u_bound"]))


# the linear family has no angle, so no edge case
_CASES = [(n, k) for n in C.NAMES for k in ("generic", "edge") if (n, k) != ("linear2", "edge")]


@pytest.mark.parametrize("twin", [False, True], ids=["shared", "params"])
@pytest.mark.parametrize("name,kind", _CASES)
def test_oracle_agrees_with_the_mpmath_reference(name, kind, twin):
    case = (C.generic_case if kind == "generic" else C.edge_case)(name, twin)
    ref = C.reference_derivatives(name, kind, twin)
    cost, _ = C.total_cost(name, case.X, case.U, case.bp, case.params)
    _, g, H = C.final_grad_hess(name, case.X[:, -1], case.params)
    steps = C.euler_steps(name, case.X[:, :-1], case.U)
    for b in range(C.B):
        prob = _oracle(name, case, b)
        d = prob.derivatives(case.X[b], case.U[b], case.bp[b])
        for k, v in zip(C.FIELDS, d):
            err = C.own_max_error(v, ref[k][b])
            assert err < TOL, (k, b, err)
        og, oH = prob.final_grad_hess(case.X[b, -1])
        assert C.own_max_error(og, g[b]) < TOL and C.own_max_error(oH, H[b]) < TOL
        oc = prob.total_cost(case.X[b], case.U[b], case.bp[b])
        assert abs(oc - cost[b]) < TOL * abs(cost[b]), (b, oc, cost[b])
        on = np.stack([prob.dynamics(x, u) for x, u in zip(case.X[b, :-1], case.U[b])])
        assert C.own_max_error(on, steps[b]) < TOL


@pytest.mark.parametrize("name", C.NONLINEAR)
def test_coverage_of_the_generic_points(name):
    case = C.generic_case(name)
    fam = C.ocp(name).family
    th = case.X[:, :C.N, fam.wrap_index].ravel()
    om = case.X[:, :C.N, fam.nx - 1].ravel()          # the angular velocity is the last state
    p = C.TWO_PI
    regions = [th <= -2 * p, (th > -2 * p) & (th < 0), (th >= 0) & (th < p),
               (th >= p) & (th < 2 * p), th >= 2 * p]
    assert sum(int(r.sum()) for r in regions) == th.size
    assert all(int(r.sum()) >= 8 for r in regions), [int(r.sum()) for r in regions]
    generic = (np.abs(np.sin(th) * np.cos(th)) > 0.3) & (np.abs(om) > 1.0)
    assert 2 * int(generic.sum()) >= th.size, int(generic.sum())
    for c in (case, C.generic_case(name, True)):
        ub = np.array([r["u_bound"] for r in C.family_rows(name, C.B, c.params)])[:, None, None]
        near = (ub - np.abs(c.U)) <= 1e-5 * ub
        assert np.all(np.abs(c.U) < ub)
        assert np.all(near.sum(axis=(1, 2)) >= 4), near.sum(axis=(1, 2))
        for k, f in C.NEAR_STAGES.items():  # both signs, both distances, at the row's own bound
            assert np.array_equal(c.U[:, k, 0], ub[:, 0, 0] * f)
    assert case.bp.max() == 0.1 and case.bp.min() == 1e-8


def test_linear_case_has_near_bound_controls():
    for twin in (False, True):
        c = C.generic_case("linear2", twin)
        ub = np.array([r["u_bound"] for r in C.family_rows("linear2", C.B, c.params)])[:, None, None]
        assert np.all(np.abs(c.U) < ub)
        assert np.all(((ub - np.abs(c.U)) <= 1e-5 * ub).sum(axis=(1, 2)) >= 4)


def test_edge_list():
    p = C.TWO_PI
    e = list(C.EDGE_ANGLES)
    for base in (0.0, p, -p, 2.0 * p, -2.0 * p):
        for v in (base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)):
            assert float(v) in e
    assert any(v == 0.0 and np.signbit(v) for v in e) and any(v == 0.0 and not np.signbit(v) for v in e)
    for v in (-1e-300, p + 1e-3, -(p + 1e-3), 13.0, -13.0, 1000.0, -1000.0):
        assert v in e
    # the reference's wrap on the list is C fmod's value (+ 2 pi where negative)
    want = np.fmod(C.EDGE_ANGLES, p)
    want = np.where(want < 0, want + p, want)
    got = np.array([C.wrap_f64(a) for a in C.EDGE_ANGLES])
    assert C.same_bits(got, want)
    assert not C.same_bits(np.nextafter(got, np.inf), want)
    # a zero remainder at exactly these angles: the only places where the implementations differ,
    # by the sign of that zero (tests/family_cases.py)
    assert [float(a) for a, w in zip(C.EDGE_ANGLES, got) if w == 0.0] == [0.0, -0.0, p, -p, 2 * p, -2 * p]


def test_host_wrap_angle_equals_the_reference_bit_for_bit():
    from noc.utils import wrap_angle
    want = np.array([C.wrap_f64(a) for a in C.EDGE_ANGLES])
    assert C.same_bits(wrap_angle(C.EDGE_ANGLES), want)
    for a, w in zip(C.EDGE_ANGLES, want):   # the scalar call of noc.problems
        assert C.same_bits(wrap_angle(float(a)), w), a


def test_noc_pymod_equals_the_reference_bit_for_bit(tmp_path):
    """noc/_codegen.py's PYMOD_DEVICE -- the text a traced cost's `%` is printed as -- compiled
    for the host as it stands (NOC_DEV defined away, no contraction) and called on the edge list."""
    from noc import _codegen
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "pymod.c"
    src.write_text("#include <math.h>\n#define NOC_DEV\n" + _codegen.PYMOD_DEVICE + "\n")
    lib = tmp_path / "libpymod.so"
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(lib), str(src),
                    "-lm"], check=True)
    fn = ctypes.CDLL(str(lib)).noc_pymod
    fn.restype, fn.argtypes = ctypes.c_double, (ctypes.c_double, ctypes.c_double)
    for a in C.EDGE_ANGLES:
        assert C.same_bits(fn(float(a), C.TWO_PI), C.wrap_f64(a)), a


def test_new_points_see_a_1e9_relative_change_the_rest_state_hides():
    """Pole length x (1 + 1e-9) in the reference's cart-pole.  On the generic points fxx moves by
    more than the GPU tolerance of 1e-12 of its own maximum; on the rest-state rollout of
    test_api_gpu::test_derivatives_costates_lqr_params (N = 37, seed 3) the same change stays
    below that test's 1e-10 under its old max(1, .) measure -- it could not have been seen."""
    from noc import problems
    from oracle import noc_oracle as O, problems as PR
    pert = dict(pole_length=C.CARTPOLE_CONSTANTS["pole_length"] * (1.0 + 1e-9))
    new = C.generic_case("cartpole")
    f0 = C.reference_derivatives("cartpole")["fxx"][0]
    f1 = C.fxx_only("cartpole", new.X[0], new.U[0], pert)
    seen = C.own_max_error(f1, f0)
    assert seen > 1e-12, seen
    Nold = 37
    x0, u0 = problems.initial_conditions("cartpole", Nold, 3, seed=3)
    prob = O.NumpyProblem(PR.cartpole_ocp(1.0 / Nold))
    X = O.rollout(prob.dynamics, u0[0], x0[0])
    g0 = C.fxx_only("cartpole", X, u0[0], None, dt=1.0 / Nold)
    g1 = C.fxx_only("cartpole", X, u0[0], pert, dt=1.0 / Nold)
    hidden = float(np.max(np.abs(g1 - g0)) / max(1.0, float(np.max(np.abs(g0)))))
    assert hidden < 1e-10, hidden
    # and the reference itself is pinned there: the oracle's fxx at 1e-13 of its own maximum
    assert C.own_max_error(prob.derivatives(X, u0[0], 0.1)[7], g0) < TOL
